"""One-line digest of a bench.py JSON line: python tools/show_bench.py file.json
(the lone launch, roofline and iteration counts only when the line comes from a `--full` run)"""
import json, sys
d = json.load(open(sys.argv[1]))
line = "%s %.0f QP/s  ms/step %.3f" % (d.get("n_gpus"), d["value"], d["ms_per_step"])
r = d.get("roofline")
if r is not None:
    line += "  lone launch %.3f ms (%.0f QP/s kernel-only)  fp64 frac %.4f (dense count %.4f)  iters mean %.0f max %d" % (
        r["launch_ms"], d["kernel_only"]["value"], r["frac"], r["frac_dense_count"], r["iterations_mean"], r["iterations_max"])
print(line + "  solved %d/%d" % (d["solver"]["solved"], d["solver"]["problems"]))
