"""The late handoff of sg_submit_async: a batch's group-stage verdict and its decide stage are the next call's.

Every trace is a Workload(4, ...) one cut into batches of 6,000-40,000 events (above k_tiny's 256 and one 4,096-event
tile), run with the default SG_RADIX_BELOW (radix group stage) and with SG_RADIX_BELOW=0 (hot / cold stage, several
tiles).  The oracle replays each trace once (module fixtures) and is only read afterwards.
"""
import numpy as np
import pytest

import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import engine as E
from sentinel_amd import tracegen as T

N_BATCH = 8        # more than the rotation of two slots and the event sets can hide
MAX_RES = 4096
RADIX = [pytest.param(None, id="radix"), pytest.param("0", id="hotcold")]


def _trace():
    w = T.Workload(4, n_entries=64_000, n_res=3_000)
    ev = w.events
    cuts = np.linspace(0, len(ev), N_BATCH + 1).astype(np.int64)
    return w, [np.ascontiguousarray(ev[a:b]) for a, b in zip(cuts[:-1], cuts[1:])], cuts


def _refs(ev):
    """Global index an EXIT / TRACE names (-1: none, or an ENTRY)."""
    r = (ev["aux"] & np.uint64(A.REF_NONE)).astype(np.int64)
    return np.where((ev["kind"] != A.EV_ENTRY) & (r != A.REF_NONE), r, -1)


def _sample(ev, n_res):
    cnt = np.bincount(ev["res_id"], minlength=n_res)
    return np.unique(np.concatenate([np.argsort(-cnt)[:25], np.nonzero(cnt)[0][::101]]))


def _nodes(x, res):
    out = []
    for r in res:
        s = x.read_node(int(r))
        out.append((s["has_chain"], s["thread"], s["second"][:2].copy(), s["minute"].copy()))
    return out


def _same_nodes(a, b):
    for (ca, ta, sa, ma), (cb, tb, sb, mb) in zip(a, b):
        assert ca == cb and ta == tb
        np.testing.assert_array_equal(sa, sb)
        np.testing.assert_array_equal(ma, mb)


def _engine(w):
    eng = E.Engine(max_resources=MAX_RES, max_slot_chain_size=0, status_ring_log2=24)
    w.install(eng)
    return eng


def _oracle(w):
    orc = O.Oracle(max_slot_chain_size=0)
    w.install(orc)
    return orc


@pytest.fixture(scope="module")
def rotation():
    w, parts, cuts = _trace()
    orc = _oracle(w)
    do = np.concatenate([orc.submit(p) for p in parts])
    res = _sample(w.events, w.n_res)
    return {"w": w, "parts": parts, "cuts": cuts, "do": do, "res": res, "nodes": _nodes(orc, res)}


def _bad_batch(parts, cuts, why):
    """parts[1] with one ENTRY that no later event names made invalid: (batch, index in it)."""
    b = parts[1].copy()
    named = set(_refs(b).tolist())
    j = next(i for i in range(len(b) // 2, len(b))
             if b["kind"][i] == A.EV_ENTRY and int(cuts[1]) + i not in named and b["ts"][i - 1] > b["ts"][0])
    if why == "res":
        b["res_id"][j] = MAX_RES
    else:
        b["ts"][j] = b["ts"][j - 1] - 1
    return b, j


@pytest.fixture(scope="module")
def verdict():
    """A = batch 0, C = batch 1 (A's continuation by index), B = C made invalid; the oracle sees A then C."""
    w, parts, cuts = _trace()
    orc = _oracle(w)
    do = [orc.submit(parts[0]), orc.submit(parts[1])]
    ev = w.events[:cuts[2]]
    res = _sample(ev, w.n_res)
    return {"w": w, "parts": parts, "cuts": cuts, "do": do, "res": res, "nodes": _nodes(orc, res)}


def test_traces_hold_what_the_gpu_tests_need():
    """CPU only: EXITs name ENTRYs of the batch before, and each invalid batch is invalid for one reason."""
    w, parts, cuts = _trace()
    for k in range(1, N_BATCH):
        assert 6_000 <= len(parts[k]) <= 40_000
        r = _refs(parts[k])
        cross = (r >= cuts[k - 1]) & (r < cuts[k])
        assert cross.sum() > 100, k  # k_resolve reads what the previous batch's post wrote
    for why in ("res", "ts"):
        b, j = _bad_batch(parts, cuts, why)
        c = parts[1]
        same = np.ones(len(b), dtype=bool)
        same[j] = False
        assert np.array_equal(b[same], c[same]) and b["kind"][j] == A.EV_ENTRY
        assert cuts[1] + j not in set(_refs(b).tolist())  # no EXIT / TRACE is left naming another resource's ENTRY
        back = np.nonzero(np.diff(b["ts"]) < 0)[0]
        if why == "res":
            assert (b["res_id"] >= MAX_RES).sum() == 1 and len(back) == 0
        else:
            assert (b["res_id"] < MAX_RES).all() and list(back) == [j - 1]
            assert b["ts"][j] >= parts[0]["ts"][-1]  # not before the batch that was decided
        assert int(b["ts"][-1] - b["ts"].min()) < 2 ** 31
    assert (w.events["res_id"] < MAX_RES).all() and (np.diff(w.events["ts"]) >= 0).all()


def _run_async(eng, parts, device):
    """Every part with sg_submit_async back to back, then sg_sync: the decisions."""
    if device:
        import torch
        ins = [torch.from_numpy(p.view(np.uint8).copy()).cuda() for p in parts]
        outs = [torch.zeros(len(p), dtype=torch.int32, device="cuda") for p in parts]
        torch.cuda.synchronize()
        for p, i, o in zip(parts, ins, outs):
            eng.submit_ptr(i.data_ptr(), len(p), o.data_ptr(), sync=False)
        eng.sync()
        return np.concatenate([o.cpu().numpy().view(np.uint32) for o in outs])
    outs = [np.zeros(len(p), dtype=np.uint32) for p in parts]
    for p, o in zip(parts, outs):
        eng.submit_ptr(p.ctypes.data, len(p), o.ctypes.data, sync=False)
    eng.sync()
    return np.concatenate(outs)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("radix_below", RADIX)
def test_rotation(rotation, radix_below, device, monkeypatch):
    if radix_below is not None:
        monkeypatch.setenv("SG_RADIX_BELOW", radix_below)
    R = rotation
    eng = _engine(R["w"])
    dg = _run_async(eng, R["parts"], device)
    np.testing.assert_array_equal(dg, R["do"])
    tl, gl = eng.timing_log(), eng.gap_log()
    assert tl.shape == (N_BATCH, 4) and (tl > 0).all()
    # the log holds the elapsed times as measured (NaN where an event was not recorded): a wrong pairing of event sets
    # gives a negative or missing gap.  From the second batch on both gaps are real intervals -- the host acts between
    # the two group events, k_resolve and k_chain run between the two decide events -- and the whole test runs in far
    # less than a second.
    assert gl.shape == (N_BATCH, 2) and (gl >= 0).all()
    assert (gl[1:] > 0).all() and (gl[1:] < 1000.0).all()
    ng = _nodes(eng, R["res"])
    _same_nodes(ng, R["nodes"])
    eng.close()
    # the same batches with sg_submit
    eng = _engine(R["w"])
    ds = np.concatenate([eng.submit(p) for p in R["parts"]])
    np.testing.assert_array_equal(dg, ds)
    _same_nodes(ng, _nodes(eng, R["res"]))
    eng.close()
    # ... and handed off inside the submitting call
    monkeypatch.setenv("SG_HANDOFF", "0")
    eng = _engine(R["w"])
    dh = _run_async(eng, R["parts"], device)
    np.testing.assert_array_equal(dg, dh)
    gh = eng.gap_log()
    assert len(eng.timing_log()) == N_BATCH and gh.shape == (N_BATCH, 2)
    assert (gh[1:] > 0).all() and (gh[1:] < 1000.0).all()
    _same_nodes(ng, _nodes(eng, R["res"]))
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("next_call", ["submit", "sync", "log_then_sync"])
@pytest.mark.parametrize("why", ["res", "ts"])
@pytest.mark.parametrize("radix_below", RADIX)
def test_deferred_verdict(verdict, radix_below, why, next_call, monkeypatch):
    if radix_below is not None:
        monkeypatch.setenv("SG_RADIX_BELOW", radix_below)
    V = verdict
    a, c = V["parts"][0], V["parts"][1]
    b, _ = _bad_batch(V["parts"], V["cuts"], why)
    eng = _engine(V["w"])
    oa, ob = np.zeros(len(a), dtype=np.uint32), np.zeros(len(b), dtype=np.uint32)
    eng.submit_ptr(a.ctypes.data, len(a), oa.ctypes.data, sync=False)  # both return OK
    eng.submit_ptr(b.ctypes.data, len(b), ob.ctypes.data, sync=False)
    with pytest.raises(E.SentinelError) as ei:  # B's verdict: the next call's, which takes no batch of its own
        if next_call == "submit":
            eng.submit(c)
        else:
            if next_call == "log_then_sync":  # a diagnostics export cannot return the verdict: it keeps it
                assert len(eng.timing_log()) == 1
            eng.sync()
    assert ei.value.code == A.SG_EINVAL
    assert ("res_id" if why == "res" else "non-decreasing") in str(ei.value)
    eng.sync()  # exactly once
    np.testing.assert_array_equal(oa, V["do"][0])
    dc = eng.submit(c)
    np.testing.assert_array_equal(dc, V["do"][1])
    _same_nodes(_nodes(eng, V["res"]), V["nodes"])
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("radix_below", RADIX)
def test_implicit_handoff(verdict, radix_below, monkeypatch):
    if radix_below is not None:
        monkeypatch.setenv("SG_RADIX_BELOW", radix_below)
    V = verdict
    a, c = V["parts"][0], V["parts"][1]
    # async, then read_node without a sync
    orc = _oracle(V["w"])
    orc.submit(a)
    r = int(np.argmax(np.bincount(a["res_id"])))
    eng = _engine(V["w"])
    oa = np.zeros(len(a), dtype=np.uint32)
    eng.submit_ptr(a.ctypes.data, len(a), oa.ctypes.data, sync=False)
    _same_nodes(_nodes(eng, [r]), _nodes(orc, [r]))
    np.testing.assert_array_equal(oa, V["do"][0])
    # async, then sg_submit of the next batch: in order, both exact
    dc = eng.submit(c)
    np.testing.assert_array_equal(dc, V["do"][1])
    _same_nodes(_nodes(eng, V["res"]), V["nodes"])
    eng.close()
    # async, then close
    eng = _engine(V["w"])
    oa = np.zeros(len(a), dtype=np.uint32)
    eng.submit_ptr(a.ctypes.data, len(a), oa.ctypes.data, sync=False)
    eng.close()
    assert eng.h is None
