"""The storage of the long-horizon polish (adacharge_amd/csrc/acn_qp_polslab.hpp: the slab of global memory and the LDS of a
workgroup, sized for the worst case of the shape) on the host: tests/host/polish_long_slab.cpp carves both up as the kernel
does, built with -fsanitize=address,undefined and run as a program of its own.  No GPU."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slab_and_lds_carve_up_under_address_sanitizer(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")) if c), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "polish_long_slab")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "adacharge_amd", "csrc"), os.path.join(ROOT, "tests", "host", "polish_long_slab.cpp"), "-o", exe],
                   check=True, timeout=180)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=180)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"[polish-long] slab per workgroup: 54 x 144 (Mg 16) {out['slab_bytes_54x144']} bytes, 64 x 288 x K 4 (Mg 32) {out['slab_bytes_64x288xK4']} bytes; "
          f"LDS {out['lds_bytes_54x144']} / {out['lds_bytes_64x288xK4']} bytes")
    assert out["failures"] == 0 and out["shapes"] > 1000, out
    # every table at its worst case: the 54 x 144 stress shape stays under 1 MB a workgroup, the offline day under 4 MB
    assert out["slab_bytes_54x144"] < 1 << 20 and out["slab_bytes_64x288xK4"] < 4 << 20, out
