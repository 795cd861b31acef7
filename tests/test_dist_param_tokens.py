"""dist.request_param_tokens_tensor: the PARAM_FLOW twin of request_tokens_tensor.

Every rank hands in its A.PARAM_TOKEN_REQ_DTYPE rows and the uint64 values they name as tensors, with value_off
counted from its own values; the server rank rebases the offsets, orders the merged rows by (ts, rank, index) and
decides them in one pointer call.  CPU: gloo, world 2, the oracle's array entry point behind rank 0, one rank's batch
empty in one round.  GPU (-m gpu): a one-rank RCCL group with Engine.cluster_request_param_ptr on device tensors (one
GPU on the box, as test_dist.test_request_tokens_tensor_rccl).  Both compare with one oracle fed the merged stream.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from test_dist import ROOT, T0, _port

PLAN = [[260, 190], [0, 150], [120, 0]]  # PLAN[round][rank]: batch sizes (an empty batch in rounds 1 and 2)
FIDS = list(range(31, 37))


def _rules(A):
    shapes = [(10, 1000), (5, 500), (2, 1000), (1, 200)]
    return [A.param_rule("abc", 0, 3 + i, cluster_mode=True, cluster_flow_id=f,
                         cluster_threshold_type=A.CLUSTER_THRESHOLD_GLOBAL, cluster_sample_count=shapes[i % 4][0],
                         cluster_window_interval_ms=shapes[i % 4][1]) for i, f in enumerate(FIDS)]


def _batch(A, rank, rnd):
    """This rank's rows and values: one or two values a request, value_off counted from the rank's own values, which
    start with `rank + 1` words no request names (so the two ranks' bases differ)."""
    n = PLAN[rnd][rank]
    rng = np.random.default_rng(500 * rnd + 3 + rank)
    out = np.zeros(n, dtype=A.PARAM_TOKEN_REQ_DTYPE)
    out["ts"] = T0 + 3_000 * rnd + np.cumsum(rng.integers(0, 5, n))
    out["flow_id"] = rng.choice(FIDS + [99], n)  # (99: no rule)
    out["acquire_count"] = rng.integers(1, 3, n)
    out["n_values"] = np.where(rng.random(n) < 0.15, 2, 1)
    pad = rank + 1
    out["value_off"] = pad + np.concatenate([[0], np.cumsum(out["n_values"])[:-1]]) if n else 0
    vals = np.concatenate([np.full(pad, 0xDEAD, dtype=np.uint64),
                           rng.integers(1, 9, int(out["n_values"].sum())).astype(np.uint64)])
    return out, vals


def _merged(A, world, rnd):
    """The whole round as one server sees it: rows in (ts, rank, index) order, offsets into the concatenated values."""
    rows, vals, base = [], [], 0
    for r in range(world):
        q, v = _batch(A, r, rnd)
        q = q.copy()
        q["value_off"] += base
        base += len(v)
        rows.append(q)
        vals.append(v)
    cat = np.concatenate(rows)
    src = np.concatenate([np.full(len(q), r) for r, q in enumerate(rows)])
    loc = np.concatenate([np.arange(len(q)) for q in rows])
    return cat, np.concatenate(vals), np.lexsort((loc, src, cat["ts"])), [len(q) for q in rows]


def _oracle_ptr(O, orc):
    def decide(req_ptr, n, values_ptr, n_values, out_ptr):
        assert O.lib().or_cluster_request_param_tokens(orc.h, C.c_void_p(req_ptr), n, C.c_void_p(values_ptr), n_values,
                                                       C.c_void_p(out_ptr)) == 0
    return decide


def _w_param_tensor(rank, world, port, backend):
    import torch
    import torch.distributed as dist
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    if backend == "nccl":
        torch.cuda.set_device(0)
    dist.init_process_group(backend, init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    import pyoracle as O
    from sentinel_amd import _abi as A
    from sentinel_amd import dist as D
    dev = torch.device("cuda", 0) if backend == "nccl" else torch.device("cpu")
    decide = None
    if rank == 0:
        if backend == "nccl":
            from sentinel_amd import engine as E
            eng = E.Engine(max_resources=64, cluster_max_allowed_qps=100_000)
            eng.register("abc")
            eng.load_param_rules(_rules(A))
            decide = eng.cluster_request_param_ptr
        else:
            srv = O.Oracle(cluster_max_allowed_qps=100_000)
            srv.register("abc")
            srv.load_param_rules(_rules(A))
            decide = _oracle_ptr(O, srv)
    ref = O.Oracle(cluster_max_allowed_qps=100_000)  # one server on the merged stream
    ref.register("abc")
    ref.load_param_rules(_rules(A))
    seen = set()
    for rnd in range(len(PLAN)):
        mine, vals = _batch(A, rank, rnd)
        t = torch.from_numpy(mine.view(np.uint8).copy()).to(dev)
        v = torch.from_numpy(vals.view(np.int64).copy()).to(dev)
        got = D.request_param_tokens_tensor(t, v, decide)
        assert got.device.type == dev.type
        got = got.cpu().numpy().view(A.TOKEN_RES_DTYPE)
        cat, allv, order, sizes = _merged(A, world, rnd)
        q = np.ascontiguousarray(cat[order])
        want = np.zeros(len(cat), dtype=A.TOKEN_RES_DTYPE)
        out = np.zeros(len(cat), dtype=A.TOKEN_RES_DTYPE)
        assert O.lib().or_cluster_request_param_tokens(ref.h, q.ctypes.data, len(q), allv.ctypes.data, len(allv),
                                                       out.ctypes.data) == 0
        want[order] = out
        off = sum(sizes[:rank])
        assert np.array_equal(got, want[off: off + len(mine)]), (rank, rnd)
        seen |= set(int(s) for s in want["status"])
    assert seen >= {A.TOKEN_OK, A.TOKEN_BLOCKED, A.TOKEN_NO_RULE_EXISTS}, seen
    dist.barrier()
    dist.destroy_process_group()


def test_request_param_tokens_tensor_gloo():
    mp.spawn(_w_param_tensor, args=(2, _port(), "gloo"), nprocs=2, join=True)


@pytest.mark.gpu
def test_request_param_tokens_tensor_rccl():
    mp.spawn(_w_param_tensor, args=(1, _port(), "nccl"), nprocs=1, join=True)
