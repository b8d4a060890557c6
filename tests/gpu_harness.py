"""What the GPU tests share to put an engine on a named matching path: the path rows (once), the environment
context manager, the engine builder that asserts Engine.paths(), batches from model arrays, the pipelined
submit/collect loop and the book check. A plain module: tests/test_gpu_harness.py pins it on the CPU with a
stub engine."""
import contextlib
import os

# name -> (levels, environment, expected eng.paths(), grouped); "{hot}" is the table's ME_HOT_MIN
_ROWS = {
    "reg": (128, {"ME_REG_AGG": "0"}, {"grouped_agg": False}, True),
    "gwalk": (128, {"ME_REG_AGG": "1", "ME_GW_CANCEL": "0"}, {"grouped_agg": True, "grouped_cancels": False}, True),
    "gwalk_cx": (128, {"ME_REG_AGG": "1", "ME_GW_CANCEL": "1"}, {"grouped_agg": True, "grouped_cancels": True}, True),
    "deep256": (256, {"ME_HOT_MIN": "0"}, {"hot_agg": False}, False),
    "deep": (1024, {"ME_HOT_MIN": "0"}, {"hot_agg": False}, False),
    "hot_agg": (1024, {"ME_HOT_MIN": "{hot}", "ME_HOT_AGG": "1"}, {"hot_agg": True}, False),
    "hot": (2048, {"ME_HOT_MIN": "{hot}", "ME_HOT_AGG": "0"}, {"hot_agg": False}, False),
}


def path_table(hot_min, deep256=True):
    """The rows with the hot paths' ME_HOT_MIN = `hot_min`, with or without the L = 256 generic row."""
    return {name: (L, {k: v.format(hot=hot_min) for k, v in env.items()}, dict(expect), grouped)
            for name, (L, env, expect, grouped) in _ROWS.items() if deep256 or name != "deep256"}


PATHS = path_table(64)                       # seven rows
FEED_PATHS = path_table(200, deep256=False)  # the six rows of the feed, TIF, cancel-target and book-reader tests
SMALL = tuple(p for p in PATHS if PATHS[p][3])  # the L = 128 paths: launch groups


@contextlib.contextmanager
def env(vars):
    old = {k: os.environ.get(k) for k in vars}
    os.environ.update(vars)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def engine_on(me, path, S, base, batches, *, table=PATHS, levels=None, ring=1 << 22, env_over=None, group=None, **kw):
    """An engine on `path` of `table` for `batches` (anything with len()): the row's environment, overlaid by
    `env_over`, holds while the constructor runs; the row's expected paths() is asserted. A caller's keyword wins
    over the defaults; `group` becomes batches_per_launch on a grouped path."""
    L, row_env, expect, grouped = table[path]
    if "max_batch" not in kw:
        kw["max_batch"] = max(len(b) for b in batches)
    if "max_resting" not in kw:
        kw["max_resting"] = sum(len(b) for b in batches) + 1024
    kw.setdefault("seq_ring", ring)
    if grouped and group is not None:
        kw.setdefault("batches_per_launch", group)
    with env(dict(row_env, **(env_over or {}))):
        eng = me.Engine(S, levels or L, base, **kw)
    p = eng.paths()
    for k, v in expect.items():
        assert p[k] == v, f"{path}: paths() {p}"
    return eng


def feed_engine(me, path, S, base, max_batch, max_resting, **kw):
    """The feed tests' engine: a FEED_PATHS row and sizes of the test's own."""
    return engine_on(me, path, S, base, (), table=FEED_PATHS, max_batch=max_batch, max_resting=max_resting, **kw)


def as_batch(me, a):
    return me.Batch(a.seq, a.price_q4, a.qty, a.symbol, a.kind)


def pipelined(eng, batches, lag, stage=None):
    """Host batches with at most `lag` in flight, collected in submission order; -> outputs indexed by batch.
    `stage(k, batch)` returns what is submitted in batch k's place."""
    out, tickets = [None] * len(batches), []
    for k, b in enumerate(batches):
        tickets.append((k, eng.submit_host(stage(k, b) if stage else b)))
        while len(tickets) > lag:
            j, t = tickets.pop(0)
            out[j] = eng.collect(t)
    for j, t in tickets:
        out[j] = eng.collect(t)
    return out


def check_books(eng, model, ctx):
    from tests._parity import assert_books_equal

    assert_books_equal(eng, model, range(eng.num_symbols), ctx)
    assert eng.resting_count() == eng.admission()["resting"] == model.resting(), f"{ctx}: resting counters"
