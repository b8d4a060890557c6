"""tests/gpu_harness.py on the CPU, against a stub engine: the path tables written out, env, engine_on and
pipelined. Needs no build and no GPU."""
import os
import types

import pytest

from tests import gpu_harness as gh

# ---- the tables, literally: a change to what selects a path shows up here ------------------------------------------

PATHS_64 = {
    "reg": (128, {"ME_REG_AGG": "0"}, {"grouped_agg": False}, True),
    "gwalk": (128, {"ME_REG_AGG": "1", "ME_GW_CANCEL": "0"}, {"grouped_agg": True, "grouped_cancels": False}, True),
    "gwalk_cx": (128, {"ME_REG_AGG": "1", "ME_GW_CANCEL": "1"}, {"grouped_agg": True, "grouped_cancels": True}, True),
    "deep256": (256, {"ME_HOT_MIN": "0"}, {"hot_agg": False}, False),
    "deep": (1024, {"ME_HOT_MIN": "0"}, {"hot_agg": False}, False),
    "hot_agg": (1024, {"ME_HOT_MIN": "64", "ME_HOT_AGG": "1"}, {"hot_agg": True}, False),
    "hot": (2048, {"ME_HOT_MIN": "64", "ME_HOT_AGG": "0"}, {"hot_agg": False}, False),
}
FEED_PATHS_200 = {
    "reg": (128, {"ME_REG_AGG": "0"}, {"grouped_agg": False}, True),
    "gwalk": (128, {"ME_REG_AGG": "1", "ME_GW_CANCEL": "0"}, {"grouped_agg": True, "grouped_cancels": False}, True),
    "gwalk_cx": (128, {"ME_REG_AGG": "1", "ME_GW_CANCEL": "1"}, {"grouped_agg": True, "grouped_cancels": True}, True),
    "deep": (1024, {"ME_HOT_MIN": "0"}, {"hot_agg": False}, False),
    "hot_agg": (1024, {"ME_HOT_MIN": "200", "ME_HOT_AGG": "1"}, {"hot_agg": True}, False),
    "hot": (2048, {"ME_HOT_MIN": "200", "ME_HOT_AGG": "0"}, {"hot_agg": False}, False),
}


def test_the_two_tables_are_what_they_were():
    assert gh.PATHS == PATHS_64 and list(gh.PATHS) == list(PATHS_64)
    assert gh.FEED_PATHS == FEED_PATHS_200 and list(gh.FEED_PATHS) == list(FEED_PATHS_200)
    assert gh.SMALL == ("reg", "gwalk", "gwalk_cx")


def test_tables_share_no_dict():
    a, b = gh.path_table(64), gh.path_table(64)
    a["reg"][1]["ME_REG_AGG"] = "x"
    a["reg"][2]["grouped_agg"] = "x"
    assert b == PATHS_64 and gh.PATHS == PATHS_64


# ---- env -------------------------------------------------------------------------------------------------------------

@pytest.fixture
def clean(monkeypatch):
    """ME_T_SET = "old", ME_T_UNSET absent, no other ME_* variable; restored after the test."""
    for k in [k for k in os.environ if k.startswith("ME_")]:
        monkeypatch.delenv(k)
    monkeypatch.setenv("ME_T_SET", "old")


def _me_env():
    return {k: v for k, v in os.environ.items() if k.startswith("ME_")}


def test_env_sets_and_restores(clean):
    with gh.env({"ME_T_SET": "new", "ME_T_UNSET": "1"}):
        assert _me_env() == {"ME_T_SET": "new", "ME_T_UNSET": "1"}
    assert _me_env() == {"ME_T_SET": "old"}


def test_env_restores_when_the_body_raises(clean):
    with pytest.raises(KeyError):
        with gh.env({"ME_T_SET": "new", "ME_T_UNSET": "1"}):
            raise KeyError("body")
    assert _me_env() == {"ME_T_SET": "old"}


def test_env_nests(clean):
    with gh.env({"ME_T_SET": "a", "ME_T_UNSET": "a"}):
        with gh.env({"ME_T_SET": "b", "ME_T_OTHER": "b"}):
            assert _me_env() == {"ME_T_SET": "b", "ME_T_UNSET": "a", "ME_T_OTHER": "b"}
        assert _me_env() == {"ME_T_SET": "a", "ME_T_UNSET": "a"}
    assert _me_env() == {"ME_T_SET": "old"}


# ---- engine_on -------------------------------------------------------------------------------------------------------

def _stub(paths):
    """A stand-in for the package: Engine records its arguments and the ME_* environment it was built under."""
    made = []

    class Engine:
        def __init__(self, *args, **kw):
            self.args, self.kw, self.env = args, kw, _me_env()
            made.append(self)

        def paths(self):
            return dict(paths)

    return types.SimpleNamespace(Engine=Engine, made=made)


ALL_PATHS = {"grouped_agg": True, "grouped_cancels": True, "hot_agg": False}
BATCHES = [range(5), range(9), range(2)]


def test_engine_on_defaults_and_environment(clean):
    me = _stub(ALL_PATHS)
    eng = gh.engine_on(me, "gwalk_cx", 4, "base", BATCHES)
    assert me.made == [eng]
    assert eng.args == (4, 128, "base")
    assert eng.kw == {"max_batch": 9, "max_resting": 16 + 1024, "seq_ring": 1 << 22}
    assert eng.env == {"ME_T_SET": "old", "ME_REG_AGG": "1", "ME_GW_CANCEL": "1"}
    assert _me_env() == {"ME_T_SET": "old"}


def test_engine_on_env_over_overlays_the_row(clean):
    me = _stub({"hot_agg": True})
    eng = gh.engine_on(me, "hot_agg", 1, "b", BATCHES, table=gh.FEED_PATHS, env_over={"ME_HOT_MIN": "64", "ME_T_SET": "x"})
    assert eng.env == {"ME_HOT_MIN": "64", "ME_HOT_AGG": "1", "ME_T_SET": "x"}
    assert _me_env() == {"ME_T_SET": "old"}
    assert gh.engine_on(me, "hot_agg", 1, "b", BATCHES, table=gh.FEED_PATHS).env["ME_HOT_MIN"] == "200"
    assert gh.engine_on(me, "hot_agg", 1, "b", BATCHES).env["ME_HOT_MIN"] == "64"


def test_engine_on_explicit_keywords_win(clean):
    me = _stub(ALL_PATHS)
    eng = gh.engine_on(me, "gwalk_cx", 2, "b", BATCHES, ring=64, max_batch=4096, max_resting=7, far_levels=8,
                       batches_per_launch=3, group=5)
    assert eng.kw == {"max_batch": 4096, "max_resting": 7, "seq_ring": 64, "far_levels": 8, "batches_per_launch": 3}
    assert gh.engine_on(me, "gwalk_cx", 2, "b", BATCHES, ring=64, seq_ring=128).kw["seq_ring"] == 128
    # with both sizes given the batches are not looked at
    assert gh.engine_on(me, "gwalk_cx", 2, "b", (), max_batch=1, max_resting=2).kw == \
        {"max_batch": 1, "max_resting": 2, "seq_ring": 1 << 22}
    assert gh.feed_engine(me, "gwalk_cx", 2, "b", 300, 2048, batches_per_launch=4).kw == \
        {"max_batch": 300, "max_resting": 2048, "seq_ring": 1 << 22, "batches_per_launch": 4}


def test_engine_on_levels_override(clean):
    me = _stub(ALL_PATHS)
    assert gh.engine_on(me, "deep", 2, "b", BATCHES, levels=8192).args == (2, 8192, "b")
    assert gh.engine_on(me, "deep", 2, "b", BATCHES).args == (2, 1024, "b")


@pytest.mark.parametrize("path", list(PATHS_64))
def test_engine_on_group_only_on_grouped_paths(clean, path):
    me = _stub({"grouped_agg": PATHS_64[path][2].get("grouped_agg", False), "grouped_cancels": path == "gwalk_cx",
                "hot_agg": path == "hot_agg"})
    grouped = path in ("reg", "gwalk", "gwalk_cx")
    assert gh.engine_on(me, path, 2, "b", BATCHES, group=8).kw.get("batches_per_launch") == (8 if grouped else None)
    assert "batches_per_launch" not in gh.engine_on(me, path, 2, "b", BATCHES).kw
    assert me.made[-1].env == dict(PATHS_64[path][1], ME_T_SET="old")


def test_engine_on_asserts_paths(clean):
    me = _stub({"grouped_agg": True, "grouped_cancels": False})
    gh.engine_on(me, "gwalk", 2, "b", BATCHES)
    with pytest.raises(AssertionError, match=r"^gwalk_cx: paths\(\) \{"):
        gh.engine_on(me, "gwalk_cx", 2, "b", BATCHES)
    assert _me_env() == {"ME_T_SET": "old"}


def test_as_batch_passes_the_five_columns():
    me = types.SimpleNamespace(Batch=lambda *a: a)
    a = types.SimpleNamespace(seq=1, price_q4=2, qty=3, symbol=4, kind=5)
    assert gh.as_batch(me, a) == (1, 2, 3, 4, 5)


# ---- pipelined -------------------------------------------------------------------------------------------------------

class _Pipe:
    def __init__(self):
        self.log, self.open = [], []

    def submit_host(self, b):
        self.log.append(("submit", b, tuple(self.open)))
        self.open.append(b)
        return ("ticket", b)

    def collect(self, t):
        assert t[0] == "ticket"
        self.log.append(("collect", t[1]))
        self.open.remove(t[1])
        return ("out", t[1])


@pytest.mark.parametrize("n,lag", [(7, 1), (7, 3), (3, 5), (0, 2), (5, 5)])
def test_pipelined_keeps_lag_batches_in_flight(n, lag):
    eng = _Pipe()
    batches = [f"b{k}" for k in range(n)]
    outs = gh.pipelined(eng, batches, lag)
    assert outs == [("out", b) for b in batches]
    subs = [e for e in eng.log if e[0] == "submit"]
    for k, (_, b, uncollected) in enumerate(subs):
        assert b == batches[k]
        assert list(uncollected) == batches[max(0, k - lag):k]  # exactly batches k-lag .. k-1
    assert [e[1] for e in eng.log if e[0] == "collect"] == batches  # in submission order
    assert eng.open == []


def test_pipelined_stage_sees_each_batch_once():
    eng, seen = _Pipe(), []

    def stage(k, b):
        seen.append((k, b))
        return b.upper() if k % 3 == 0 else b

    batches = [f"b{k}" for k in range(7)]
    outs = gh.pipelined(eng, batches, 2, stage)
    assert seen == list(enumerate(batches))
    want = ["B0", "b1", "b2", "B3", "b4", "b5", "B6"]
    assert [e[1] for e in eng.log if e[0] == "submit"] == want
    assert outs == [("out", w) for w in want]
