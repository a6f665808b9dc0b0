"""The storage of the wide-site polish (adacharge_amd/csrc/acn_qp_polwide.hpp: the slab of global memory and the LDS of a
workgroup, sized for the worst case of the shape) on the host: tests/host/polish_wide_slab.cpp carves both up as the kernel
does, built with -fsanitize=address,undefined and run as a program of its own.  No GPU."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slab_and_lds_carve_up_under_address_sanitizer(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")) if c), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "polish_wide_slab")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "adacharge_amd", "csrc"), os.path.join(ROOT, "tests", "host", "polish_wide_slab.cpp"), "-o", exe],
                   check=True, timeout=180)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"[polish-wide] slab per workgroup: 512 x 48 x K 2 (Mg 28) {out['slab_bytes_512x48']} bytes, 1,024 x 48 (Mg 48) {out['slab_bytes_1024x48']} bytes; "
          f"LDS {out['lds_bytes_512x48']} / {out['lds_bytes_1024x48']} bytes")
    assert out["failures"] == 0 and out["shapes"] > 1000, out
    # every table at its worst case: the capacitance matrix of 1,024 columns is 4.2 MB of either; the largest shape stays under 9 MB
    assert 4 << 20 < out["slab_bytes_512x48"] < out["slab_bytes_1024x48"] < 9 << 20, out
    assert out["lds_bytes_1024x48"] <= 152 * 1024, out
