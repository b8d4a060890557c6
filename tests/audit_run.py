"""One engine against ReduceBook with the resident book audited after every launch group (tests/book_audit.py):
what tests/test_book_audit_gpu.py and tests/test_price_edges_gpu.py drive their streams through."""
import numpy as np

from tests._parity import assert_fills_equal, assert_results_equal
from tests.book_audit import audit, names
from tests.gpu_harness import as_batch
from tests.reduce_model import ReduceBook


def _same(a, b):
    return len(a) == len(b) and bool(np.all(a == b))


class Run:
    """One engine against one model; `group` runs a launch group through both and audits the resident book."""

    def __init__(self, me, eng, S, grouped, ctx):
        self.me, self.eng, self.S, self.grouped, self.ctx = me, eng, S, grouped, ctx
        self.model = ReduceBook(S)
        self.last_seq = 0
        self.raws = []     # the figures of every checkpoint
        self.problems = []

    def group(self, arrays, tag):
        bs = [as_batch(self.me, a) for a in arrays]
        if self.grouped:
            tickets = [self.eng.submit_host(b) for b in bs]
            outs = [self.eng.collect(t) for t in tickets]
        else:
            outs = [self.eng.submit_batch(b) for b in bs]
        res = []
        for k, (a, (r, f)) in enumerate(zip(arrays, outs)):
            ro, fo = self.model.submit(a)
            assert_results_equal(r, ro, f"{self.ctx} {tag} batch {k}")
            assert_fills_equal(f, fo, f"{self.ctx} {tag} batch {k}")
            if a.seq.max():
                self.last_seq = max(self.last_seq, int(a.seq.max()))
            res.append(ro)
        return res, self.checkpoint(tag)

    def checkpoint(self, tag):
        raw = self.eng.debug_export()
        v, books = audit(raw, last_seq=self.last_seq)
        if v:
            self.problems.append(f"{tag}: {len(v)} violations {names(v)}; first {v[:4]}")
        for s in range(self.S):
            want = self.model.dump(s)
            if not _same(books[s], want):
                self.problems.append(f"{tag}: symbol {s}: the book rebuilt from raw memory is not the model's")
            if not _same(self.eng.dump(s), want):
                self.problems.append(f"{tag}: symbol {s}: eng.dump is not the model's")
        if self.eng.resting_count() != self.model.resting():
            self.problems.append(f"{tag}: resting count")
        win, far = [], []  # per symbol: the prices of its occupied window levels / of its far levels
        for s in range(self.S):
            y = raw["sym"][s]
            win.append(set((int(y["base"]) + np.nonzero(raw["levels"][s]["total"] > 0)[0]).tolist()))
            far.append({int(p) for k in range(2) for p in
                        raw["far"]["price"][int(raw["fdir"][s, k]["off"]):][:int(y["nfar"][k])]})
        fig = dict(audit.last, base=raw["sym"]["base"].copy(), nfar=int(raw["sym"]["nfar"].sum()),
                   nfar_sides=raw["sym"]["nfar"].copy().reshape(-1), win=win, far=far,
                   moved=int((raw["fdir"]["off"] >= raw["info"]["far_inline"]).sum()),
                   multi=int(((raw["levels"]["head"] != raw["levels"]["tail"])).sum()))
        self.raws.append(fig)
        return raw

    def done(self):
        assert not self.problems, f"{self.ctx}: " + "\n".join(self.problems[:12])
