"""What the GPU tests of the feeds (tests/test_quotes_gpu.py, tests/test_depth_gpu.py, tests/test_trades_gpu.py,
tests/test_stops_gpu.py, tests/test_feed_ring_gpu.py) share: scripted records, the event comparison, the
config-5-style stream. The matching paths and the engine on one are tests/gpu_harness.py's."""
import numpy as np

BUY, SELL = 1, 2
BIG = 2_147_483_647


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
