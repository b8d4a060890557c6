"""The book auditor (tests/book_audit.py) is not vacuous: canonical raw images of model books audit clean and
rebuild to the model's dump, and every single-field corruption is reported under its own invariant's name.
Runs on CPU: the images are laid out here from a `ReduceBook`, no engine is involved.
The images and the corruptions are tests/audit_images.py's.
"""
import functools

import numpy as np
import pytest

from tests import book_audit as ba
from tests import reduce_model as rm
from tests import tif_model as tm
from tests.audit_images import CORRUPTIONS, Targets, build_image, corrupt
from tests.book_audit import NIL, audit, names

SEEDS = (1, 2, 3, 4, 5, 6)
S_IMG, L_IMG = 4, 128


@functools.lru_cache(maxsize=None)
def _image(seed):
    base, arrays = rm.reduce_stream(400 + seed, S_IMG, L_IMG, 3, 600, far_pct=8, drift=(0, 3)[seed % 2], convert_pct=50,
                                    mix=(62, 8, 4, 6, 8, 12), spread=5)
    model = rm.ReduceBook(S_IMG)
    for a in arrays:
        model.submit(a)
    # deep queues: 40 orders at one passive price on each side of every symbol (three chunks), then the middle
    # chunk of the bids and the last order of each queue cancelled (an unlinked chunk, a dead slot below tend)
    q = max(int(a.seq.max()) for a in arrays) + 1
    rec, cx = [], []
    for s in range(S_IMG):
        mid = int(base[s]) + L_IMG // 2
        for side, px in ((1, mid - 25), (2, mid + 25)):
            first = q
            for _ in range(40):
                rec.append((q, px, 5, s, side))
                q += 1
            cx += [(first + j, s) for j in (range(16, 32) if side == 1 else ())] + [(first + 39, s)]
    rec += [(q - 1, t, 0, s, 9) for t, s in cx]
    model.submit(tm.Arrays(*[[r[i] for r in rec] for i in range(5)]))
    last = q - 1
    return build_image(model, L_IMG, base, last, seed=seed), model, last


@pytest.mark.parametrize("seed", SEEDS)
def test_canonical_image_audits_clean(seed):
    raw, model, last = _image(seed)
    v, books = audit(raw, last_seq=last)
    assert not v, v[:5]
    st = audit.last
    assert st["old_orders"] > 0 and st["live_orders"] == model.resting() > 300
    assert raw["sym"]["nfar"].sum() > 0 and (raw["fdir"]["off"] >= raw["info"]["far_inline"]).any()
    assert len(Targets(raw).multi) >= 2 * S_IMG and raw["sym"]["free_head"][0] != NIL and raw["sym"]["nfree"][1] > 0
    assert raw["chunk_top"][0] < raw["cpool"][0]
    for s in range(S_IMG):
        want = model.dump(s)
        assert len(books[s]) == len(want) and np.all(books[s] == want), s


def test_every_invariant_has_a_corruption():
    assert {inv for inv, _ in CORRUPTIONS.values()} == set(ba.INVARIANTS)
    assert len(CORRUPTIONS) >= 20


@pytest.mark.parametrize("name", list(CORRUPTIONS))
def test_corruption_is_reported_under_its_name(name):
    raw, _, last = _image(1)
    bad, inv = corrupt(raw, name)
    v, _ = audit(bad, last_seq=last)
    assert inv in names(v), (name, inv, names(v))
    assert all(x.where for x in v)
    # and the image it came from is still clean (the corruption changed the copy alone)
    assert not audit(raw, last_seq=last)[0]


def test_authority_table_is_well_formed():
    fields = {r.field for r in ba.AUTHORITY}
    assert {"Level.total", "tend", "occ", "best_bid / best_ask", "loc", "old"} <= fields
    for r in ba.AUTHORITY:
        assert r.strength in ("exact", "bound", "unread") and r.when in (ba.ANY, "L > 128", "L <= 128")
        assert r.writers and r.readers and r.argument
    for L in (128, 1024):
        assert ba.strength("occ", {"levels": L}) in ("exact", "bound", "unread")


def test_design_holds_the_same_rows():
    """DESIGN.md §3 states the table the auditor runs on: every (field, condition, strength) is there."""
    import os

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    table = text[text.index("**Authority table."):]
    table = table[table.index("| Field |"):].split("\n\n")[0]
    rows = [[c.strip() for c in ln.strip("|").split("|")] for ln in table.splitlines() if ln.startswith("| `")]
    got = {(r[0].replace("`", ""), r[3], r[4]) for r in rows}
    want = {(r.field, r.strength, r.when) for r in ba.AUTHORITY}
    assert got == want, (sorted(got - want), sorted(want - got))
