"""What the two polish kernels share and the host can compile (adacharge_amd/csrc/acn_qp_polish_steps.hpp: the inverse of the
packed-triangle index, the blocking-constraint codes): tests/host/polish_steps.cpp, built with -fsanitize=address,undefined and
run as a program of its own.  No GPU."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_triangle_index_and_codes_of_the_shared_polish_steps(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")) if c), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "polish_steps")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "adacharge_amd", "csrc"), os.path.join(ROOT, "tests", "host", "polish_steps.cpp"), "-o", exe],
                   check=True, timeout=180)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=180)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"[polish-steps] triangle entries checked {out['triangle_entries']}, codes {out['codes']}")
    assert out["failures"] == 0, out
    # every entry of the largest capacitance matrix of each kernel: 128 and 256 session columns
    assert out["triangle_entries"] == [128 * 129 // 2, 256 * 257 // 2], out
    # short: (lb, ub) x EVSE {0, 63} x period {0, 31}, sessions EVSE {0, 63} x slot {0, 3}, rows {0, 31} x period {0, 31};
    # long: the same with periods {0, 31, 255, 256, 287}
    assert out["codes"] == [8 + 4 + 4, 20 + 4 + 10], out
