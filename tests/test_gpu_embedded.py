"""The embedded token server on the decision path (sg_cluster_embedded; DESIGN.md §5 "Embedded token server").

With the mode on, an ENTRY that reaches FlowSlot on a resource whose only flow rule is a cluster rule asks the engine's
own token server and obeys the answer (FlowRuleChecker.passClusterCheck / applyTokenResult,
core/slots/block/flow/FlowRuleChecker.java:126-187).  tests/embedded_util.py builds the expected result from the
unchanged oracle (its docstring has the steps); tests/test_embedded_host.py (CPU) shows that every trace reaches what
its case is about.  Compared here: all 32 bits of every decision word, read_node of every resource, the token state
(one more external request per flowId on both sides: status, remaining, wait), and the read-back of the last batch
(requests issued, answers by status, placement).

Rules with cluster_fallback_to_local (the issue's Part B) are refused while the mode is on: test_refusals.
"""
import numpy as np
import pytest

import embedded_util as X
import pyoracle as O
import test_gpu_counts as GC
from sentinel_amd import _abi as A
from sentinel_amd import engine as E

pytestmark = pytest.mark.gpu

ENTRY = A.EV_ENTRY
OWNER_SETS = {
    "J1": GC.OWNERS["J1"], "J4": GC.OWNERS["J4"], "J16": GC.OWNERS["J16"],
    "coop": GC.BIN_MODES["coop"], "skip": GC.BIN_MODES["skip"], "hot": GC.HOT_BINS,
    "default": {}, "lane": GC.OWNERS["lane"], "hot_cold": {"SG_RADIX_BELOW": "0"},
}


def _engine(c, embedded=True, **kw):
    kw.setdefault("max_resources", 64)
    kw.setdefault("max_slot_chain_size", 0)
    limits = getattr(c, "limits", None)
    eng = E.Engine(status_ring_log2=22, **kw)
    for nm in c.names:
        eng.register(nm)
    for k in range(getattr(c, "n_contexts", 0)):
        eng.intern_context("filler%d" % k)
    for k in range(getattr(c, "n_origins", 0)):
        eng.intern_origin("app-%d" % k)
    if limits:
        for ns, lim in limits.items():
            eng.cluster_namespace(ns, lim)
            eng.cluster_assign_flows(ns, [f for f, n in c.flow_ns.items() if n == ns])
    eng.load_flow_rules(c.flow_rules)
    if c.degrade_rules:
        eng.load_degrade_rules(c.degrade_rules)
    if getattr(c, "auth_tuples", None):
        eng.load_authority_rules([A.authority_rule(*t) for t in c.auth_tuples])
    for f, n in getattr(c, "connected", {}).items():
        eng.cluster_set_connected(f, n)
    if embedded:
        eng.cluster_embedded(True)
    return eng


def _device_replay(eng, c):
    """Every batch from device buffers, back to back through the pipeline, one sync at the end."""
    import torch
    dev = torch.device("cuda", 0)
    ev, ext = c.ev, getattr(c, "ext", None)
    d_ev = torch.from_numpy(np.ascontiguousarray(ev).view(np.uint8).copy()).to(dev)
    d_out = torch.zeros(len(ev), dtype=torch.int32, device=dev)
    d_ext = None if ext is None else torch.from_numpy(np.ascontiguousarray(ext).view(np.uint8).copy()).to(dev)
    for a, b in zip(c.cuts[:-1], c.cuts[1:]):
        a, b = int(a), int(b)
        if ext is None:
            eng.submit_ptr(d_ev.data_ptr() + a * 24, b - a, d_out.data_ptr() + a * 4, sync=False)
        else:
            eng.submit_ex_ptr(d_ev.data_ptr() + a * 24, d_ext.data_ptr() + a * 16, b - a, d_out.data_ptr() + a * 4,
                              sync=False)
    eng.sync()
    return d_out.cpu().numpy().view(np.uint32)


def _submit(eng, c, k):
    a, b = int(c.cuts[k]), int(c.cuts[k + 1])
    ext = getattr(c, "ext", None)
    return eng.submit(c.ev[a:b]) if ext is None else eng.submit_ex(c.ev[a:b], ext[a:b])


def _same_stats(st, c, k, what=""):
    want = X.answer_counts(c.answers[k])
    assert st["requests"] == len(c.reqs[k]), (what, k, st, len(c.reqs[k]))
    assert {n: st[n] for n in want} == want, (what, k, st, want)
    assert st["late_segments"] == 0


def _same_state(eng, c, dg, what=""):
    GC._same_words(dg, c.want, c.ev)
    for r in range(len(c.names)):
        GC._same_node(eng.read_node(r), c.nodes[r], "%s res %d" % (what, r))
    got = eng.cluster_request_array(c.probe)
    for f in ("status", "remaining", "wait_in_ms"):
        np.testing.assert_array_equal(got[f], c.probe_answers[f], err_msg="%s token state: %s" % (what, f))


def _eligible_segments(c, k, longer_than):
    cnt = np.bincount(c.ev["res_id"][c.cuts[k]:c.cuts[k + 1]], minlength=len(c.names))
    return [r for r in c.eligible if cnt[r] > longer_than], [r for r in c.eligible if 0 < cnt[r] <= longer_than]


# ---------------------------------------------------------------- 1. owners
@pytest.mark.parametrize("owner", sorted(OWNER_SETS))
def test_owners(owner, monkeypatch):
    GC._setenv(monkeypatch, OWNER_SETS[owner])
    c = X.owners_case()
    eng = _engine(c)
    dg = _device_replay(eng, c)
    st = eng.cluster_embedded_stats()
    _same_stats(st, c, 2, owner)
    _same_state(eng, c, dg, owner)
    if owner == "lane":  # SG_DEBUG_FLAGS=2: every segment on a lane
        long_, short = [], list(c.eligible)
    else:  # a batch below the shard size: the lane bins end at 128 events unless SG_LANE_MAX says otherwise
        long_, short = _eligible_segments(c, 2, 0 if "SG_LANE_MAX" in OWNER_SETS[owner] else 128)
    assert (st["coop_segments"], st["lane_segments"]) == (len(long_), len(short)), (owner, st)
    a, b = int(c.cuts[2]), int(c.cuts[3])
    ahead = int((c.blocked[a:b] & np.isin(c.ev["res_id"][a:b], long_)).sum())
    assert st["words_ahead"] == ahead and (ahead > 0 or owner == "lane"), (owner, st, ahead)
    eng.close()


# ---------------------------------------------------------------- 2. one long segment
@pytest.mark.parametrize("env", [dict(GC.HOT_BINS, SG_SKIP_MIN="16"), dict(GC.HOT_BINS, SG_SKIP_MIN="1000"), {},
                                 dict(GC.HOT_BINS, SG_SKIP_MIN="16", SG_RADIX_BELOW="0")],
                         ids=["skip16", "skip1000", "default", "hot_cold"])
def test_one_long_segment(env, monkeypatch):
    # BLOCKED ENTRYs inside the owner's frozen stretches and skipped spans (k_fill leaves their words alone)
    GC._setenv(monkeypatch, env)
    c = X.long_case()
    eng = _engine(c)
    dg = []
    for k in range(len(c.cuts) - 1):
        dg.append(_submit(eng, c, k))
        st = eng.cluster_embedded_stats()
        _same_stats(st, c, k)
        assert (st["coop_segments"], st["lane_segments"]) == (1, 0)
        assert st["words_ahead"] == int(c.blocked[c.cuts[k]:c.cuts[k + 1]].sum())
    _same_state(eng, c, np.concatenate(dg))
    print("spans recorded (%s): %d" % (env.get("SG_SKIP_MIN"), eng.spans_total()))
    if env.get("SG_SKIP_MIN") == "16":
        assert eng.spans_total() > 0  # the owner skipped spans of the cut stretch; k_fill wrote around the BLOCKED words
    eng.close()


# ---------------------------------------------------------------- 3. requests not made
@pytest.mark.parametrize("variant", ["flags", "chain", "nullctx", "off"])
def test_requests_not_made(variant):
    c = X.not_made_case(variant)
    eng = _engine(c, aux_node_capacity=1 << 14, **c.oracle_cfg)
    dg = []
    for k in range(len(c.cuts) - 1):
        dg.append(_submit(eng, c, k))
        _same_stats(eng.cluster_embedded_stats(), c, k, variant)  # the reference's request list, no more, no fewer
    _same_state(eng, c, np.concatenate(dg), variant)
    eng.close()


# ---------------------------------------------------------------- 4. answers other than OK and BLOCKED
@pytest.mark.parametrize("case", ["prio", "avg_local", "zero", "limiter"])
@pytest.mark.parametrize("bins", ["default", "coop"])
def test_answers(case, bins, monkeypatch):
    # prio: SHOULD_WAIT words with their waits (a prioritized resource is a lane's); avg_local: a threshold times the
    # connected count; zero: BAD_REQUEST for a count of 0; limiter: TOO_MANY_REQUEST in the middle of every batch, in
    # two namespaces.  A refused ENTRY of a rule without fallback passes FlowSlot
    GC._setenv(monkeypatch, OWNER_SETS[bins])
    c = getattr(X, case + "_case")()
    eng = _engine(c)
    dg = []
    for k in range(len(c.cuts) - 1):
        dg.append(_submit(eng, c, k))
        _same_stats(eng.cluster_embedded_stats(), c, k, case)
    _same_state(eng, c, np.concatenate(dg), case)
    if case == "limiter":
        t = int(c.probe["ts"][0])
        for ns, q in c.ns_qps.items():
            assert eng.cluster_namespace_qps(ns, t)[0] == q, (ns, eng.cluster_namespace_qps(ns, t), q)
    eng.close()


# ---------------------------------------------------------------- 5. one token state
def test_interleaved_external_requests():
    c = X.interleaved_case()
    eng = _engine(c)
    dg = []
    for k in range(len(c.cuts) - 1):
        got = eng.cluster_request_array(c.external[k])
        for f in ("status", "remaining", "wait_in_ms"):
            np.testing.assert_array_equal(got[f], c.ext_answers[k][f], err_msg="external call %d: %s" % (k, f))
        dg.append(_submit(eng, c, k))
        _same_stats(eng.cluster_embedded_stats(), c, k)
    _same_state(eng, c, np.concatenate(dg))
    eng.close()


def test_rejected_batch_takes_no_token():
    # batch 1 with a malformed last event is rejected: no token consumed, no limiter bucket moved; the same batch,
    # mended, and the next one are answered as the reference, which never saw the rejected one
    c = X.owners_case()
    eng = _engine(c)
    dg = [_submit(eng, c, 0)]
    bad = c.ev[c.cuts[1]:c.cuts[2]].copy()
    bad["res_id"][-1] = 1 << 30
    with pytest.raises(E.SentinelError) as ei:
        eng.submit(bad)
    assert ei.value.code == A.SG_EINVAL
    dg += [_submit(eng, c, 1), _submit(eng, c, 2)]
    _same_stats(eng.cluster_embedded_stats(), c, 2)
    _same_state(eng, c, np.concatenate(dg))
    eng.close()


@pytest.mark.parametrize("tiny", ["1", "0"])
def test_small_synchronous_batches(tiny, monkeypatch):
    # synchronous batches of 250 events: without an eligible rule they are k_tiny's (one workgroup, which knows nothing of
    # the class); with one loaded they take the batched path and ask for their tokens like any other batch
    monkeypatch.setenv("SG_TINY", tiny)
    c = X.small_case()
    eng = _engine(c)
    dg = []
    for k in range(len(c.cuts) - 1):
        dg.append(_submit(eng, c, k))
        _same_stats(eng.cluster_embedded_stats(), c, k, "small")
    _same_state(eng, c, np.concatenate(dg), "small")
    eng.close()


# ---------------------------------------------------------------- 6. the switch
def test_mode_off_is_todays_decision():
    # the same engine and trace without the switch, and with the switch turned on and off again before the trace
    c = X.owners_case()
    for flip in (False, True):
        eng = _engine(c, embedded=False)
        if flip:
            eng.cluster_embedded(True)
            eng.cluster_embedded(False)
        dg = _device_replay(eng, c)
        GC._same_words(dg, c.w0, c.ev)
        st = eng.cluster_embedded_stats()
        assert all(v == 0 for v in st.values()), st
        eng.close()


def test_toggling_keeps_node_and_token_state():
    c = X.toggled_case()
    eng = _engine(c, embedded=False)
    dg = [_submit(eng, c, 0)]
    assert eng.cluster_embedded_stats()["requests"] == 0
    eng.cluster_embedded(True)
    eng.cluster_embedded(True)  # (idempotent)
    for k in (1, 2):
        dg.append(_submit(eng, c, k))
        _same_stats(eng.cluster_embedded_stats(), c, k)
    _same_state(eng, c, np.concatenate(dg))
    eng.close()


# ---------------------------------------------------------------- 7. refusals
def _refused(fn, *a):
    with pytest.raises(E.SentinelError) as ei:
        fn(*a)
    assert ei.value.code == A.SG_ENOTSUP, ei.value
    return str(ei.value)


def _bad_rule_sets(c):
    """Flow-rule lists that hold a cluster rule outside the supported shape, each with the resource it must name.  (A
    cluster rule with strategy RELATE or CHAIN is not among them: the loader drops it as invalid in either mode.)"""
    el = sorted(c.eligible)
    a, b = c.names[el[0]], c.names[el[1]]
    other = next(nm for r, nm in enumerate(c.names) if r not in c.eligible)
    base = [r for r in c.flow_rules if r.resource.decode() != a]
    fid = c.eligible[el[0]]
    mk = lambda **kw: X.cluster_rule(a, fid, 20, **kw)
    return {
        "beside a local rule": base + [mk(), A.flow_rule(a, 100)],
        "two cluster rules": base + [mk(), X.cluster_rule(a, fid + 500, 30)],
        "THREAD grade": base + [mk(grade=A.FLOW_GRADE_THREAD)],
        "an origin": base + [mk(limit_app="app-1")],
        "a shared flowId": base + [X.cluster_rule(a, c.eligible[el[1]], 20)],
        "named by a RELATE rule": [r for r in base if r.resource.decode() != other] +
                                  [mk(), A.flow_rule(other, 100, strategy=A.STRATEGY_RELATE, ref_resource=a)],
        "fallback to local": base + [mk(cluster_fallback_to_local=True)],
    }, a, b


def test_refusals():
    # every shape outside the supported one: SG_ENOTSUP naming the rule's resource, nothing changed -- the batches
    # between the refused calls are decided as before them
    c = X.owners_case()
    eng = _engine(c)
    sets, a, b = _bad_rule_sets(c)
    names = sorted(sets)
    dg = []
    for k in range(3):
        for nm in names[k::3]:
            msg = _refused(eng.load_flow_rules, sets[nm])
            assert a in msg or b in msg, (nm, msg)
        msg = _refused(eng.load_param_rules, [A.param_rule(b, 0, 20)])
        assert b in msg, msg
        dg.append(_submit(eng, c, k))
        _same_stats(eng.cluster_embedded_stats(), c, k)
    _same_state(eng, c, np.concatenate(dg))
    eng.close()


def test_switching_on_over_unsupported_rules_is_refused():
    # loaded with the mode off (accepted, decided as today: the fallback rule as a local one), the switch is refused
    # and the trace is decided as the oracle decides these rules
    c = X.owners_case()
    sets, a, _ = _bad_rule_sets(c)
    for nm in ("fallback to local", "beside a local rule", "a shared flowId"):
        eng = E.Engine(max_resources=64, max_slot_chain_size=0, status_ring_log2=22)
        orc = O.Oracle(max_slot_chain_size=0)
        for x in (eng, orc):
            for r in c.names:
                x.register(r)
            x.load_flow_rules(sets[nm])
            x.load_degrade_rules(c.degrade_rules)
        assert a in _refused(eng.cluster_embedded, True), nm
        k = 0
        ev = c.ev[c.cuts[k]:c.cuts[k + 1]]
        GC._same_words(eng.submit(ev), orc.submit(ev), ev)
        assert eng.cluster_embedded_stats()["requests"] == 0
        eng.close()
        orc.close()
