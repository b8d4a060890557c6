"""The depth feed, the trade feed, the order query and the order preview over the cluster (include/me_cluster.h:
me_cluster_depth*, me_cluster_trades*, me_cluster_order_query, me_cluster_order_preview), through the plain
calls, through me_cluster_matcher's hooks (slice-number stamps) and behind the service. The checks live in
tests/parity_cluster_worker.py; every comparison there is exact, against one oracle book holding every symbol.
Ranks are fresh child processes, each under its own timeout."""
import json
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(kind, world, tmp_path, timeout=180, env_extra=None):
    out = str(tmp_path / f"parity_{kind}_{world}.json")
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), **(env_extra or {}))
        # child processes (never exec over a GPU-initialised interpreter)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "parity_cluster_worker.py"), kind, out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        logs.append(o.decode(errors="replace")[-3000:])
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return json.load(open(out))


def _whole(r):
    assert r["ok"], r["msg"]
    assert r["depth_events"] > 100 and r["trade_events"] > 50, r
    assert r["found"] > 20 and r["previews"] > 1024, r
    assert r["restamped"] > 500, r
    assert r["svc_books"] > 20 and r["svc_trades"] > 20 and r["svc_previews"] > 100, r
    assert r["slices"] >= 6 + 6 + 8 + 3, r


def test_new_entry_points_are_declared_and_exported(built):
    from matching_engine_amd import _abi

    lib = _abi.load()
    for name in ("me_cluster_depth_enable", "me_cluster_depth", "me_cluster_trades_enable", "me_cluster_trades",
                 "me_cluster_order_query", "me_cluster_order_preview"):
        assert name in _abi.PROTOTYPES and hasattr(lib, name), name
    hooks = ["depth_enable", "depth", "trades_enable", "trades", "order_query", "order_preview"]
    for struct in (_abi.MeMatcher, _abi.MeShardOps):
        names = [f[0] for f in struct._fields_]
        assert names[names.index("quotes") + 1:] == hooks, names  # appended after `quotes`, in this order


def test_objects_without_the_methods_get_null_hooks(built):
    """The hasattr rule: an object that lacks a method leaves that hook NULL, so existing matchers and shards
    behave as before."""
    from matching_engine_amd.cluster import ShardOps, python_matcher

    class Plain:
        num_symbols, max_batch, max_resting = 4, 16, 64

        def match(self, b):
            raise NotImplementedError

        def book_orders(self, s, d):
            raise NotImplementedError

    class WithPreview(Plain):
        def order_preview(self, symbol, kind, price_q4, qty):
            raise NotImplementedError

    m, mp, so = python_matcher(Plain()), python_matcher(WithPreview()), ShardOps(Plain(), 64).struct
    for name in ("quotes", "depth_enable", "depth", "trades_enable", "trades", "order_query", "order_preview"):
        assert not getattr(m, name) and not getattr(so, name), name
        assert bool(getattr(mp, name)) == (name == "order_preview"), name


@pytest.mark.parametrize("world", [2, 3])
def test_cluster_parity_tcp_oracle_shards(built, tmp_path, world):
    _whole(_run("oracle", world, tmp_path))


def test_missing_depth_hook_is_invalid_and_not_sticky(built, tmp_path):
    """A shard without `depth` makes me_cluster_depth_enable ME_E_INVALID on rank 0; the following slices match
    and collect normally and the other hooks still work."""
    r = _run("nohook", 2, tmp_path)
    assert r["ok"], r["msg"]
    assert r["slices"] == 3


@pytest.mark.gpu
def test_cluster_parity_tcp_gpu_engines(built, tmp_path):
    """Two ranks, each with its own HIP engine on the box's GPU, protocol over TCP."""
    _whole(_run("gpu", 2, tmp_path))


@pytest.mark.gpu
def test_cluster_parity_rccl_single_rank(built, tmp_path):
    """World size 1 over RCCL with rank 0's part, feeds and queries forced through the transport."""
    _whole(_run("rccl", 1, tmp_path, env_extra={"ME_CLUSTER_DIRECT": "0"}))


@pytest.mark.gpu
def test_cluster_parity_rccl_single_rank_direct(built, tmp_path):
    """World size 1 as deployed: rank 0 asks its engine directly, no pack copy and no transport."""
    _whole(_run("rccl", 1, tmp_path))
