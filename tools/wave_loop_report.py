"""Instruction classes of the wave kernel's solver loop, segment by segment, from the compiler's assembly (CPU only).

    python tools/wave_loop_report.py [--unit acn_qp_wave_e14] [--csrc DIR] [--asm FILE] [--least N] ARGS [ARGS ...]

ARGS names an instantiation of admm_wave_kernel by its template arguments, e.g. "5,1,12,1,false,2,14,false" (the
headline).  The unit is compiled to assembly with the flags of adacharge_amd/build.py (device pass only; --csrc: the
sources of another checkout, e.g. the parent commit's; --asm: an assembly file made earlier instead of compiling), the
kernel's body is split into segments at labels and behind branches, and the solver loop is taken to be the smallest loop
-- a branch back to a label, with every segment that reaches the branch without passing the label -- that holds an MFMA
(everything inside the loop is unrolled, so no loop within it holds one; the pass loop and the work queue around it are
larger).  Printed as JSON, per instantiation: the
loop's segments in layout order with the number of VALU / MFMA / LDS / scalar / AGPR-copy / memory / other instructions,
where each segment's branches go, and -- for a segment that holds MFMAs -- the VALU instructions before the first MFMA,
between every two consecutive MFMAs and behind the last (`valu_between_mfma`); --least N lists only the segments of at
least N instructions and sums the others (`smaller_segments`).  It counts instruction classes and nothing
else (what stands beside the matrix chains of an iteration)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("valu", "mfma", "lds", "scalar", "agpr_copy", "memory", "other")
_LABEL = re.compile(r"^([.$\w]+):")


def mangled(args):
    """admm_wave_kernel<5,1,12,1,false,2,14,false> -> the piece of its symbol that names the instantiation"""
    out = []
    for a in (a.strip() for a in args.split(",")):
        out.append({"true": "Lb1E", "false": "Lb0E"}.get(a) or f"Li{int(a)}E")
    return "admm_wave_kernelI" + "".join(out) + "E"


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("v_accvgpr"):
        return "agpr_copy"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_"):
        return "scalar"
    if op.split("_")[0] in ("buffer", "global", "scratch", "flat"):
        return "memory"
    return "other"


def kernel_body(asm, piece):
    """the lines of the kernel whose symbol holds `piece`, from its label to the end of the function"""
    lines = asm.splitlines()
    start = [i for i, l in enumerate(lines) if (m := _LABEL.match(l)) and piece in m.group(1) and not m.group(1).startswith(".")]
    if len(start) != 1:
        raise KeyError(f"{piece}: {len(start)} kernels of that name")
    end = next(i for i in range(start[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start[0] + 1:end]


def segments(body):
    """[{label, ops: [mnemonic ...], branches: [label ...]}] in layout order: a new segment at every label and behind every branch"""
    segs = [{"label": "entry", "ops": [], "branches": []}]
    for raw in body:
        line = raw.split(";")[0].strip()
        if not line:
            continue
        m = _LABEL.match(line)
        if m:
            if segs[-1]["ops"] or segs[-1]["label"] != "entry":
                segs.append({"label": m.group(1), "ops": [], "branches": []})
            else:
                segs[-1]["label"] = m.group(1)
            continue
        if line.startswith("."):
            continue
        op = line.split()[0]
        segs[-1]["ops"].append(op)
        if op.startswith("s_cbranch") or op == "s_branch":
            segs[-1]["branches"].append(line.split()[-1])
            segs.append({"label": segs[-1]["label"] + "+", "ops": [], "branches": []})
    return [s for s in segs if s["ops"]]


def solver_loop(segs):
    """indices of the segments of the smallest loop that holds an MFMA.  A loop: a branch back to a label at or before it in
    the layout, with every segment that reaches the branch without passing the label (so a spin loop or the water-filling
    loop whose blocks the layout spread around a chain does not count that chain)"""
    at = {}
    for i, s in enumerate(segs):
        at.setdefault(s["label"], i)
    preds = {i: set() for i in range(len(segs))}
    for i, s in enumerate(segs):
        for target in s["branches"]:
            if target in at:
                preds[at[target]].add(i)
        last = s["ops"][-1]
        if last not in ("s_branch", "s_endpgm", "s_setpc_b64") and i + 1 < len(segs):
            preds[i + 1].add(i)
    best = None
    for j, s in enumerate(segs):
        for target in s["branches"]:
            i = at.get(target)
            if i is None or i > j:
                continue
            body, todo = {i, j}, [j] if j != i else []
            while todo:
                for p in preds[todo.pop()]:
                    if p not in body:
                        body.add(p)
                        todo.append(p)
            ops = [op for k in body for op in segs[k]["ops"]]
            if any(classify(op) == "mfma" for op in ops) and (best is None or len(ops) < best[0]):
                best = (len(ops), sorted(body))
    if best is None:
        raise ValueError("no loop that holds an MFMA")
    return best[1]


def count(seg):
    out = {"label": seg["label"], "instructions": len(seg["ops"])}
    out.update({c: 0 for c in CLASSES})
    gaps, run = [], 0
    for op in seg["ops"]:
        c = classify(op)
        out[c] += 1
        if c == "mfma":
            gaps.append(run)
            run = 0
        elif c == "valu":
            run += 1
    if out["mfma"]:
        out["valu_between_mfma"] = gaps + [run]
    out["branches"] = seg["branches"]
    return out


def report(asm, args, least=1):
    """least: segments of fewer instructions are not listed one by one; `smaller_segments` holds their number and sums"""
    segs = segments(kernel_body(asm, mangled(args)))
    body = solver_loop(segs)
    rows = [count(segs[k]) for k in body]
    total = lambda rs: {c: sum(r[c] for r in rs) for c in ("instructions",) + CLASSES}
    small = [r for r in rows if r["instructions"] < least]
    return {"kernel": f"admm_wave_kernel<{', '.join(a.strip() for a in args.split(','))}>", "segments_in_kernel": len(segs), "loop_segments": len(body),
            "totals": total(rows), "smaller_segments": dict(total(small), segments=len(small), fewer_instructions_than=least),
            "segments": [r for r in rows if r["instructions"] >= least]}


def assembly(unit, csrc):
    sys.path.insert(0, ROOT)
    from adacharge_amd.build import FLAGS, hipcc_path

    inc = os.path.join(os.path.abspath(csrc), "..", "..", "include")   # (<checkout>/adacharge_amd/csrc -> <checkout>/include)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.run([hipcc_path(), *FLAGS, "-I" + inc, "-I" + csrc, "--cuda-device-only", "-S", os.path.join(csrc, unit + ".hip"), "-o", out], check=True)
        return open(out).read()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("instantiations", nargs="+", metavar="ARGS", help='template arguments, e.g. "5,1,12,1,false,2,14,false"')
    ap.add_argument("--unit", default="acn_qp_wave_e14")
    ap.add_argument("--csrc", default=os.path.join(ROOT, "adacharge_amd", "csrc"), help="the sources (another checkout's adacharge_amd/csrc)")
    ap.add_argument("--asm", help="an assembly file of the unit instead of compiling")
    ap.add_argument("--least", type=int, default=1, help="list only segments of at least so many instructions; the others are summed")
    a = ap.parse_args(argv)
    asm = open(a.asm).read() if a.asm else assembly(a.unit, a.csrc)
    out = []
    for args in a.instantiations:   # (one line per segment: a report is read side by side with another)
        r = report(asm, args, a.least)
        rows = ",\n".join("   " + json.dumps(row) for row in r.pop("segments"))
        out.append("  " + json.dumps(r)[:-1] + ', "segments": [\n' + rows + "\n  ]}")
    print('{"unit": ' + json.dumps(a.unit) + ', "instantiations": [\n' + ",\n".join(out) + "\n]}")


if __name__ == "__main__":
    main()
