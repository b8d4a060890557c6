"""The service's arithmetic of stop orders (matching_engine_amd/csrc/me_service_stops.hpp: "SID-<n>" parsing, the
capacity mirror, the runs of a boundary, the hold-back of events stamped ahead) in a stand-alone program
(tests/host/stops_service_host_test.cpp) under the host compiler's address and undefined-behaviour sanitizers.
Runs on CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc"))


def test_sid_capacity_runs_and_hold_back_under_sanitizers(tmp_path):
    exe = str(tmp_path / "stops_service_host_test")
    cc = [HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
          "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
          "-I", os.path.join(ROOT, "matching_engine_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
          os.path.join(ROOT, "tests", "host", "stops_service_host_test.cpp"), "-o", exe]
    b = subprocess.run(cc, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("service stop arithmetic: ok"), r.stdout
    assert not r.stderr, r.stderr
