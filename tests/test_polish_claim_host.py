"""The claim step of the polish launch alongside the solver (adacharge_amd/csrc/acn_qp_polclaim.hpp) on the host:
tests/host/polish_claim_threads.cpp -- threads as producers and consumers -- built with -fsanitize=thread and run as a
program of its own.  No GPU."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_claim_protocol_under_thread_sanitizer(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++")) if c), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "polish_claim_threads")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-I" + os.path.join(ROOT, "adacharge_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "polish_claim_threads.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe, "6", "4", "3000", "20"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, r.stdout + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["failures"] == 0 and out["alongside"] + out["serial"] > 0, out
