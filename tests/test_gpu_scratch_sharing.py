"""Callers that share a batch slot's arrays, interleaved on one engine.

A token call (sg_cluster_request_tokens, sg_cluster_request_param_tokens), a metrics snapshot and a tiny synchronous
batch each use arrays of a batch slot while sg_submit_async keeps the two slots rotating; a token call larger than the
slots reallocates both.  Every call drains the pipeline first, so the batch decisions, the node states, the token
results and the snapshot rows must be what the oracle gives for the batch stream and the token streams replayed
separately (embedded mode is off: the two states are independent).

The batch stream is test_gpu_handoff's trace, the token requests are test_gpu_cluster's and test_gpu_ptok_device's
generators, the namespaces' expected results test_gpu_cluster_ns's one-oracle-a-namespace helper.  The oracle side of
every case is computed once (module fixtures) and only read afterwards.
"""
import ctypes as C

import numpy as np
import pytest

import pyoracle as O
import test_gpu_cluster as TC
import test_gpu_cluster_ns as NS
import test_gpu_handoff as H
import test_gpu_ptok_device as PT
from counts_util import sorted_snapshot
from sentinel_amd import _abi as A
from sentinel_amd import engine as E

TINY = 64                       # events of the synchronous call (k_tiny: at most 256)
N_TOK = 3000                    # requests of a token call in case (a)
TOK_FIDS = list(range(201, 251))
LIMITS = {"default": 1200, "other": 250}   # qps: the plain calls run at ~670 requests a second, the param calls at ~2,000
TT0 = 1_700_000_000_000
BIG_CALL = (1 << 20) + 1        # one more request than ensure_batch()'s floor: both slots are reallocated


def _cluster_rules():
    flow = [TC._rule(f, float(20 + 7 * (i % 9)), res="r%d" % f, cluster_sample_count=(1, 2, 5, 10)[i % 4],
                     cluster_window_interval_ms=(500, 1000, 2000)[i % 3]) for i, f in enumerate(TOK_FIDS)]
    return flow, PT._base_rules()


def _flow_ns():
    return {f: ("other" if f & 1 else "default") for f in TOK_FIDS + PT.FIDS}


def _install(x, w, flow, param):
    """The workload's resources and rules with the cluster rules (on resources of their own, which no event names)
    in the same lists: a rule load replaces the list."""
    x.register_ptrs(w.names_ptr, w.n_res)
    x.register("abc")
    wf = list((A.SgFlowRule * w.flow[1]).from_address(w.flow[0])) if w.flow[1] else []
    wp = list((A.SgParamRule * w.param[1]).from_address(w.param[0])) if w.param[1] else []
    x.load_flow_rules(wf + flow)
    if w.degrade[1]:
        x.load_degrade_rules((C.c_void_p(w.degrade[0]), w.degrade[1]))
    if wp or param:
        x.load_param_rules(wp + param)


def _steps_a():
    """Case (a): the 8 parts, and between consecutive parts, in rotation, a token call, a param-token call, a snapshot
    and a synchronous call of the next part's first TINY events."""
    w, parts, _ = H._trace()
    rng = np.random.default_rng(20241021)
    steps = []
    for k, p in enumerate(parts):
        if k:
            kind = ("tok", "ptok", "snap", "tiny")[(k - 1) % 4]
            t = TT0 + 6000 * k  # every token call later than the one before: the namespaces' limiters share the clock
            if kind == "tok":
                steps.append(("tok", TC._random_requests(rng, N_TOK, TOK_FIDS, t)))
            elif kind == "ptok":
                steps.append(("ptok",) + PT._call(rng, t, n=N_TOK + 1))
            elif kind == "snap":
                # (the whole trace spans 65 ms: 1.5 s on, the second the events so far lie in has rows)
                steps.append(("snap", int(parts[k - 1]["ts"][-1]) + 1500))
            else:
                steps.append(("tiny", np.ascontiguousarray(p[:TINY])))
                p = p[TINY:]
        steps.append(("batch", np.ascontiguousarray(p)))
    return w, steps


def _ptok_list(arr, vals):
    return [(int(r["ts"]), int(r["flow_id"]), int(r["acquire_count"]),
             [int(v) for v in vals[int(r["value_off"]):int(r["value_off"]) + int(r["n_values"])]]) for r in arr]


def _triples(res):
    return [(int(o["status"]), int(o["remaining"]), int(o["wait_in_ms"])) for o in res]


def _case_a():
    w, steps = _steps_a()
    flow, param = _cluster_rules()
    orc = H._oracle(w)
    tok = NS.NsOracles(LIMITS, _flow_ns())
    tok.load_flow_rules(flow)
    tok.load_param_rules(param)
    want = []
    for s in steps:
        if s[0] in ("batch", "tiny"):
            want.append(orc.submit(s[1]))
        elif s[0] == "tok":
            want.append(_triples(tok.request_array(s[1])))
        elif s[0] == "ptok":
            want.append(tok.request_param(_ptok_list(s[1], s[2])))
        else:
            want.append(sorted_snapshot(orc.snapshot(s[1], cap=1 << 18)))
    res = H._sample(w.events, w.n_res)
    return {"w": w, "steps": steps, "want": want, "res": res, "nodes": H._nodes(orc, res), "flow": flow, "param": param}


def _case_b():
    w, parts, _ = H._trace()
    flow, _ = _cluster_rules()
    reqs = TC._random_requests(np.random.default_rng(20241021 + 1), BIG_CALL, TOK_FIDS, TT0)
    orc = H._oracle(w)
    do = [orc.submit(p) for p in parts[:3]]
    tok = O.Oracle(cluster_max_allowed_qps=400)
    tok.register("abc")
    tok.load_flow_rules(flow)
    ev = np.concatenate(parts[:3])
    res = H._sample(ev, w.n_res)
    return {"w": w, "parts": parts[:3], "do": do, "reqs": reqs, "tokens": tok.cluster_request_array(reqs), "res": res,
            "nodes": H._nodes(orc, res), "flow": flow}


@pytest.fixture(scope="module")
def case_a():
    return _case_a()


@pytest.fixture(scope="module")
def case_b():
    return _case_b()


def test_traces_hold_what_the_gpu_tests_need():
    """CPU only: the batches stay above k_tiny and a tile, the synchronous piece is a k_tiny one that continues the
    trace, and the token requests of every call, and from call to call, are in time order."""
    w, steps = _steps_a()
    kinds = [s[0] for s in steps]
    assert kinds.count("batch") == H.N_BATCH and {"tok", "ptok", "snap", "tiny"} <= set(kinds)
    ev = np.concatenate([s[1] for s in steps if s[0] in ("batch", "tiny")])
    assert np.array_equal(ev, w.events) and (np.diff(ev["ts"]) >= 0).all()
    last = 0
    for s in steps:
        if s[0] == "batch":
            assert 6_000 <= len(s[1]) <= 40_000
        elif s[0] == "tiny":
            assert len(s[1]) == TINY <= 256 and (np.diff(s[1]["ts"]) >= 0).all()
        elif s[0] in ("tok", "ptok"):
            ts = s[1]["ts"].astype(np.int64)
            assert len(ts) >= N_TOK and (np.diff(ts) >= 0).all() and ts[0] > last
            last = int(ts[-1])
            assert len(set(s[1]["flow_id"].tolist())) >= 10
    flow_ns = _flow_ns()
    assert {flow_ns[f] for f in TOK_FIDS} == set(LIMITS) == {flow_ns[f] for f in PT.FIDS}  # the grouped limiter
    assert BIG_CALL == (1 << 20) + 1 and max(len(p) for p in H._trace()[1]) < (1 << 20)


def _engine(w, flow, param, limits=None, **cfg):
    eng = E.Engine(max_resources=H.MAX_RES, max_slot_chain_size=0, status_ring_log2=24, **cfg)
    for ns, lim in (limits or {}).items():
        if ns != "default":
            eng.cluster_namespace(ns, lim)
    _install(eng, w, flow, param)
    for ns in (limits or {}):
        if ns != "default":
            eng.cluster_assign_flows(ns, [f for f, n in _flow_ns().items() if n == ns])
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("radix_below", H.RADIX)
def test_interleaved_calls(case_a, radix_below, monkeypatch):
    if radix_below is not None:
        monkeypatch.setenv("SG_RADIX_BELOW", radix_below)
    R = case_a
    eng = _engine(R["w"], R["flow"], R["param"], LIMITS, cluster_max_allowed_qps=LIMITS["default"])
    got = []
    for s in R["steps"]:
        if s[0] == "batch":
            out = np.zeros(len(s[1]), dtype=np.uint32)
            eng.submit_ptr(s[1].ctypes.data, len(s[1]), out.ctypes.data, sync=False)
            got.append(out)  # (final after the sync below)
        elif s[0] == "tiny":
            got.append(eng.submit(s[1]))
        elif s[0] == "tok":
            got.append(_triples(eng.cluster_request_array(s[1])))
        elif s[0] == "ptok":
            got.append(_triples(eng.cluster_request_param_array(s[1], s[2])))
        else:
            got.append(sorted_snapshot(eng.snapshot(s[1], cap=1 << 18)))
    eng.sync()
    for k, (s, g, want) in enumerate(zip(R["steps"], got, R["want"])):
        if s[0] in ("tok", "ptok"):
            bad = [i for i, (a, b) in enumerate(zip(g, want)) if a != b]
            assert not bad, (k, s[0], bad[0], g[bad[0]], want[bad[0]], len(bad))
        else:
            np.testing.assert_array_equal(g, want, err_msg="step %d (%s)" % (k, s[0]))
    H._same_nodes(H._nodes(eng, R["res"]), R["nodes"])
    # the synchronous call took k_tiny (tiny_impl, which borrows slot[cur]): a batch that falls back to the batched
    # path is collected and leaves a row in the timing log, a k_tiny one does not
    assert len(eng.timing_log()) == H.N_BATCH
    # the calls did what they are here for: requests of both kinds passed and were refused, a snapshot had rows
    for kind in ("tok", "ptok"):
        st = [t[0] for s, w_ in zip(R["steps"], R["want"]) if s[0] == kind for t in w_]
        assert st.count(A.TOKEN_OK) > 100 and len(st) - st.count(A.TOKEN_OK) > 100, kind
    assert all(len(w_) > 0 for s, w_ in zip(R["steps"], R["want"]) if s[0] == "snap")
    eng.close()


@pytest.mark.gpu
def test_token_call_regrows_both_slots(case_b):
    R = case_b
    eng = _engine(R["w"], R["flow"], [], cluster_max_allowed_qps=400)
    d0 = eng.submit(R["parts"][0])
    tokens = eng.cluster_request_array(R["reqs"])
    outs = [np.zeros(len(p), dtype=np.uint32) for p in R["parts"][1:]]
    for p, o in zip(R["parts"][1:], outs):
        eng.submit_ptr(p.ctypes.data, len(p), o.ctypes.data, sync=False)
    eng.sync()
    NS._assert_same(tokens, R["tokens"])
    for g, want in zip([d0] + outs, R["do"]):
        np.testing.assert_array_equal(g, want)
    H._same_nodes(H._nodes(eng, R["res"]), R["nodes"])
    eng.close()
