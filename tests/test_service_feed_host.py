"""What the service's quote, depth and trade streams share (matching_engine_amd/csrc/me_service_feed.hpp) in a
stand-alone program (tests/host/service_feed_test.cpp) under the host compiler's address and
undefined-behaviour sanitizers: ownership hand-over with unread events, unnamed books, first-change order,
take from the middle, names longer than the symbol field, reset. Runs on CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc"))


def test_service_feed_under_sanitizers(tmp_path):
    exe = str(tmp_path / "service_feed_test")
    cc = [HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
          "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
          "-I", os.path.join(ROOT, "matching_engine_amd", "csrc"),
          os.path.join(ROOT, "tests", "host", "service_feed_test.cpp"), "-o", exe]
    b = subprocess.run(cc, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("service feed: ok"), r.stdout
    assert not r.stderr, r.stderr
