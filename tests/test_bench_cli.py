"""bench.py's command line on a small shape (needs an MI355X): a plain run times its steps and leaves
every other leg out, --full brings them back, and --dump-outputs writes the last timed step's results
and tape — equal to the oracle's replay of the same seeded stream, and the same with and without --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, BATCH, STEPS, WARMUP = 64, 4096, 3, 2
SHAPE = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--symbols-per-gpu", str(S),
         "--batch-per-gpu", str(BATCH), "--seq-ring", str(1 << 22)]
RESULT_FIELDS = ("filled_qty", "remaining_qty", "fill_count", "tape_offset", "status", "reason")
FILL_FIELDS = ("taker_seq", "maker_seq", "price_q4", "qty", "symbol")


def run_bench(extra, dump):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SHAPE, "--dump-outputs", dump, *extra],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, "bench.py prints exactly one line on stdout"
    return json.loads(lines[0]), {n: np.load(os.path.join(dump, n + ".npy")) for n in ("results", "fills")}


@pytest.fixture(scope="module")
def plain(built, tmp_path_factory):
    return run_bench([], str(tmp_path_factory.mktemp("plain")))


@pytest.fixture(scope="module")
def last_step_oracle(built):
    """The oracle's results and tape for the last timed batch of the run's stream."""
    import matching_engine_amd as me
    from oracle.oracle import OracleBook

    st = me.Stream(me.preset(2, num_symbols=S, batch=BATCH))
    ob = OracleBook(S)
    try:
        for _ in range(WARMUP + STEPS):
            ro, fo = ob.submit(st.next(BATCH))
    finally:
        ob.close()
    return ro, fo


def test_plain_run_is_lean(plain):
    line, _ = plain
    assert line["full"] is False
    assert line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["unit"] == "orders/s" and line["higher_is_better"] is True and line["dtype"] == "int64"
    assert line["ms_per_step"] > 0
    # value and ms_per_step describe the same STEPS timed batches
    assert line["value"] == pytest.approx(STEPS * BATCH / (line["ms_per_step"] * STEPS / 1e3), rel=1e-9)
    for leg in ("fills_check_rank0", "e2e_host_path_orders_per_s_rank0", "cpu_baseline", "c1_paths", "cluster"):
        assert line[leg] is None, leg


def test_dump_is_the_last_timed_step(plain, last_step_oracle):
    _, dump = plain
    ro, fo = last_step_oracle
    assert dump["results"].dtype == np.float64 and dump["fills"].dtype == np.float64
    assert dump["results"].shape == (BATCH, len(RESULT_FIELDS))
    assert dump["fills"].shape == (len(fo), len(FILL_FIELDS)) and len(fo) > 0
    for k, f in enumerate(RESULT_FIELDS):
        assert np.array_equal(dump["results"][:, k], ro[f].astype(np.float64)), f
    for k, f in enumerate(FILL_FIELDS):
        assert np.array_equal(dump["fills"][:, k], fo[f].astype(np.float64)), f


def test_full_run_adds_the_other_legs(plain, tmp_path):
    line, dump = run_bench(["--full", "--no-cpu-baseline", "--e2e-steps", "4"], str(tmp_path))
    assert line["full"] is True and line["steps"] == STEPS
    fc = line["fills_check_rank0"]
    assert fc["checked"] and fc["mismatched_batches"] == 0 and fc["batches"] >= 1
    assert line["fills_check_mismatched_batches_all_ranks"] == 0
    assert line["e2e_host_path_orders_per_s_rank0"] > 0
    for n in ("results", "fills"):
        assert np.array_equal(dump[n], plain[1][n]), n
