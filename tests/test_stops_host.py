"""The host's arithmetic of the trigger book (matching_engine_amd/csrc/me_stops.hpp: the validation of an add,
the ascending rule of a cancel, the capacity bound) in a stand-alone program (tests/host/stops_host_test.cpp) under
the host compiler's address and undefined-behaviour sanitizers. Runs on CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc"))


def test_validation_and_capacity_under_sanitizers(tmp_path):
    exe = str(tmp_path / "stops_host_test")
    cc = [HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
          "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
          "-I", os.path.join(ROOT, "matching_engine_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
          os.path.join(ROOT, "tests", "host", "stops_host_test.cpp"), "-o", exe]
    b = subprocess.run(cc, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("trigger book host arithmetic: ok"), r.stdout
    assert not r.stderr, r.stderr
