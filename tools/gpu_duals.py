"""Dual report (acnqp_duals_device) against the solve of the same batch: HIP-event times of one launch each, five
repetitions after a warm-up, medians.  Shapes: the bench workload (16,384 x 54 x 12) and the large-site one
(2,048 x 512 x 48, bench.py's configs[4] leg).  Writes the JSON it prints to the file given as first argument."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from adacharge_amd import ObjectiveComponent, equal_share, load_flattening, quick_charge, sites
from adacharge_amd.acn import Interface
from adacharge_amd.backend import DeviceBatch, SiteHandle, default_options
from adacharge_amd.builder import ProblemBatch, build_batch, plan_from_table, scenario_batch


def headline():
    infra = sites.caltech54(); iface = Interface({"infrastructure_info": infra, "period": 5})
    obj = [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-12)]
    return plan_from_table(sites.snapshot_table(infra, 12, 16384, seed=424242), infra, iface, obj, "SOC").expand()


def large_site():
    infra = sites.synth512(); iface = Interface({"infrastructure_info": infra, "period": 5})
    T = 48; ext = 150.0 + 100.0 * np.cos(np.arange(T) / T * 2 * np.pi)
    obj = [ObjectiveComponent(load_flattening, 1.0, {"external_signal": ext})]
    rng = np.random.default_rng(5)
    snaps = [sites.random_sessions_general(infra, T, rng, False, False, demand_scale=0.12) for _ in range(8)]
    base = build_batch(snaps, infra, iface, obj, "SOC", True)
    return ProblemBatch.concatenate([scenario_batch(base, rng.lognormal(0.0, 0.05, size=256), problem=p) for p in range(8)])


def timed(fn, reps=5):
    ms = []
    for k in range(reps + 1):   # the first is the warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms[1:])), [round(m, 4) for m in ms[1:]]


out = {}
for name, make in (("bench_16384x54x12", headline), ("large_2048x512x48", large_site)):
    batch = make()
    h = SiteHandle(batch.site, 0)
    dev = DeviceBatch(batch, "cuda:0", want_y=True)
    st = torch.cuda.current_stream().cuda_stream
    o = default_options()
    mu = torch.zeros((batch.B, batch.K, batch.N), dtype=torch.float64, device="cuda:0")
    z = torch.zeros((batch.B, batch.N, batch.Tm), dtype=torch.float64, device="cuda:0")
    res = torch.zeros((batch.B, 4), dtype=torch.float64, device="cuda:0")
    solve_ms, solve_all = timed(lambda: h.solve_device(dev, o, stream=st))
    duals_ms, duals_all = timed(lambda: h.duals_device(dev, mu, res, z=z, options=o, stream=st))
    noz_ms, _ = timed(lambda: h.duals_device(dev, mu, res, options=o, stream=st))
    r, status = res.cpu().numpy(), dev.status.cpu().numpy()
    ok = np.isin(status, (1, 5))
    out[name] = dict(B=batch.B, N=batch.N, Tm=batch.Tm, K=batch.K, solve_ms=solve_ms, duals_ms=duals_ms, duals_without_z_ms=noz_ms,
                     ratio=duals_ms / solve_ms, solve_all=solve_all, duals_all=duals_all, mean_iters=float(dev.iters.float().mean()),
                     solved=int((status == 1).sum()), worst_stat=float(r[ok, 0].max()), worst_energy=float(r[ok, 1].max()),
                     worst_site=float(r[ok, 2].max()), worst_comp=float(r[ok, 3].max()))
    print(name, json.dumps(out[name]), flush=True)
    h.close(); del dev, mu, z, res
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
