"""One dense and one session-table call of 4,096 caltech54 x 12 problems, for a stream-operation count:

    ACNQP_LIBRARY=<libacn_qp_hip.so> rocprofv3 --kernel-trace --memory-copy-trace --stats -d <dir> -- python tools/gpu_stream_ops.py [dense|table]

Run once per library, each in a process of its own; per entry the number of kernel dispatches by name and of copies by
direction must be equal between two builds whose host pipelines claim to do the same work."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(which):
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.backend import SiteHandle, default_options, library_path
    from adacharge_amd.builder import plan_from_table

    infra = sites.caltech54()
    iface = Interface({"infrastructure_info": infra, "period": 5})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    plan = plan_from_table(sites.snapshot_table(infra, 12, 4096, seed=99), infra, iface, obj)
    batch = plan.expand()
    h = SiteHandle(batch.site, 0)
    res = h.solve(batch, default_options()) if which == "dense" else h.solve_table(plan, default_options())
    h.close()
    print(f"[stream_ops] {which} {library_path()}: solved {int((res.status == 1).sum())} of {batch.B}, iterations {int(res.iters.sum())}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "dense")
