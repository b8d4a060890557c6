"""recentre_base (matching_engine_amd/csrc/me_layout.hpp), the window base a re-centre moves to, in a stand-alone
program (tests/host/recentre_test.cpp) under the host compiler's address and undefined-behaviour sanitizers:
every window size the paths use, targets and best prices at both ends of int64 and around 0, against a spec
in 128-bit arithmetic. Any signed overflow in the function fails the run. Runs on CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM", "/opt/rocm")
HIPCC = os.environ.get("HIPCC", os.path.join(ROCM, "bin", "hipcc"))


def test_recentre_base_under_sanitizers(tmp_path):
    exe = str(tmp_path / "recentre_test")
    cc = [HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function",
          "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
          "-I", os.path.join(ROCM, "include"), "-I", os.path.join(ROOT, "include"),
          "-I", os.path.join(ROOT, "matching_engine_amd", "csrc"),
          os.path.join(ROOT, "tests", "host", "recentre_test.cpp"), "-o", exe]
    b = subprocess.run(cc, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("recentre_base: ok"), r.stdout
    assert not r.stderr, r.stderr
