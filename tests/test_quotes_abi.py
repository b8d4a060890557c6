"""The quote feed's C-ABI surface (include/me_engine.h me_quote, me_quotes_*) and the test model of the
feed (tests/quote_model.py) over the CPU oracle. Runs on CPU."""
import ctypes as C
import os
import re

import numpy as np

from tests import quote_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_me_quote_is_48_bytes_and_matches_the_header(built):
    from matching_engine_amd import _abi

    assert _abi.QUOTE_DTYPE.itemsize == 48 and _abi.QUOTE_DTYPE == qm.QUOTE_DTYPE
    src = open(os.path.join(ROOT, "include", "me_engine.h")).read()
    body = re.search(r"typedef struct me_quote \{(.*?)\} me_quote;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\b([a-z_0-9]+)\s*(?:,|$)", decl.strip())]
    assert names == list(_abi.QUOTE_DTYPE.names)
    assert (_abi.QUOTE_HAS_BID, _abi.QUOTE_HAS_ASK) == (1, 2)


def test_library_exports_the_feed(built):
    from matching_engine_amd import _abi

    lib = C.CDLL(_abi.LIB_PATH)
    for name in ("me_quotes_enable", "me_quotes_read", "me_quotes_stats"):
        assert hasattr(lib, name), name
        assert name in _abi.PROTOTYPES
    # a null engine is refused, not dereferenced
    lib = _abi.load()
    assert lib.me_quotes_enable(None, 16) == _abi.ME_E_INVALID
    assert lib.me_quotes_read(None, None, 0, None, None) == _abi.ME_E_INVALID
    assert lib.me_quotes_stats(None, None, None, None) == _abi.ME_E_INVALID


def test_model_over_the_oracle(built):
    """The model's own arithmetic: first-change events, conflation between two expects, absent sides,
    int64 level totals, and replay of every event giving the books' tops."""
    from matching_engine_amd import _abi
    from oracle import oracle
    from tests.tif_model import Arrays

    S = 5
    ob = oracle.OracleBook(S)
    m = qm.QuoteModel(ob, S)
    assert len(m.expect(0)) == 0
    k = _abi.kind
    big = 2_147_483_647
    ob.submit(Arrays([1, 2, 3, 4, 5], [100, 100, -7, 0, 90], [big, big, 5, 6, 1], [1, 1, 3, 4, 1],
                     [k(1), k(1), k(2), k(1), k(1)]))
    ev = m.expect(1)
    assert ev["symbol"].tolist() == [1, 3, 4] and (ev["batches"] == 1).all()
    assert ev[0]["bid_qty"] == 2 * big and ev[0]["flags"] == qm.HAS_BID
    assert ev[1]["ask_price_q4"] == -7 and ev[1]["flags"] == qm.HAS_ASK and ev[1]["bid_price_q4"] == 0
    assert ev[2]["bid_price_q4"] == 0 and ev[2]["flags"] == qm.HAS_BID
    # two batches, one expect: the intermediate quote of symbol 3 is not seen; symbol 4 ends as it began
    ob.submit(Arrays([6, 7], [-9, 1], [2, 1], [3, 4], [k(2), k(1)]))
    ob.submit(Arrays([7, 7, 8], [6, 7, 0], [0, 0, 5], [3, 4, 3], [k(1, 0, 1), k(1, 0, 1), k(1, 1)]))
    assert len(m.peek()) == 1
    ev2 = m.expect(3)
    assert ev2["symbol"].tolist() == [3] and ev2[0]["flags"] == 0 and ev2[0]["ask_price_q4"] == 0
    table = qm.replay(qm.tops(qm._Empty(), S), np.concatenate([ev, ev2]))
    assert qm.same_quotes(table, qm.tops(ob, S))
