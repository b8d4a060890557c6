"""What the GPU tests of the two feeds (tests/test_quotes_gpu.py, tests/test_depth_gpu.py,
tests/test_feed_ring_gpu.py) share: the matching paths, an engine on a named path, scripted records, the
config-5-style stream. tests/test_tif_gpu.py takes its path table from here too."""
import contextlib
import os

import numpy as np

BUY, SELL = 1, 2
BIG = 2_147_483_647

# name -> (levels, environment, expected eng.paths(), grouped)
PATHS = {
    "reg": (128, {"ME_REG_AGG": "0"}, {"grouped_agg": False}, True),
    "gwalk": (128, {"ME_REG_AGG": "1", "ME_GW_CANCEL": "0"}, {"grouped_agg": True, "grouped_cancels": False}, True),
    "gwalk_cx": (128, {"ME_REG_AGG": "1", "ME_GW_CANCEL": "1"}, {"grouped_agg": True, "grouped_cancels": True}, True),
    "deep": (1024, {"ME_HOT_MIN": "0"}, {"hot_agg": False}, False),
    "hot_agg": (1024, {"ME_HOT_MIN": "200", "ME_HOT_AGG": "1"}, {"hot_agg": True}, False),
    "hot": (2048, {"ME_HOT_MIN": "200", "ME_HOT_AGG": "0"}, {"hot_agg": False}, False),
}
SMALL = ("reg", "gwalk", "gwalk_cx")


@contextlib.contextmanager
def _env(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _engine(me, path, S, base, max_batch, max_resting, **kw):
    L, env, expect, _ = PATHS[path]
    with _env(env):
        eng = me.Engine(S, L, base, max_batch=max_batch, max_resting=max_resting, seq_ring=1 << 22, **kw)
    p = eng.paths()
    for k, v in expect.items():
        assert p[k] == v, f"{path}: paths() {p}"
    return eng


class Rows:
    """Scripted records in stream order: (symbol, side, price, qty) LIMITs, MARKETs and cancels."""

    def __init__(self, me, seq0=1):
        self.me, self.seq, self.r = me, seq0, []

    def limit(self, s, side, px, q):
        self.r.append((self.seq, px, q, s, self.me.kind(side)))
        self.seq += 1
        return self.seq - 1

    def market(self, s, side, q):
        self.r.append((self.seq, 0, q, s, self.me.kind(side, 1)))
        self.seq += 1

    def cancel(self, s, target):
        self.r.append((self.seq - 1, target, 0, s, self.me.kind(BUY, 0, 1)))

    def batch(self):
        b = self.me.Batch(*[[x[i] for x in self.r] for i in range(5)])
        self.r = []
        return b


def _same(got, exp, ctx):
    assert got.dtype == exp.dtype
    assert np.array_equal(got, exp), f"{ctx}: events differ\n got {got}\n exp {exp}"


def _c5_stream(me, S, L, nb, batch):
    sc = me.preset(5, num_symbols=S, levels=L, batch=batch, cancel_pct=30, market_pct=15, market_qty_mult=4,
                   far_pct=3, zipf_s=1.1, seed=11)
    st = me.Stream(sc)
    return st.base_prices(), [st.next(batch) for _ in range(nb)]
