"""Rule reloads on live state, on every decide owner.

Rule lists change while traffic runs.  A load must be a no-op for an equal list, install fresh controller / breaker
state for any other list, keep the node statistics and the state of the kinds that were not reloaded, keep a
ParameterMetric while its resource keeps a param rule (include/sentinel_gpu.h), and leave the engine as it was when it
is refused.  Each script of reload_util.py plays loads, batches and asynchronous batches on an engine and on the
oracle and compares every decision word, every node and the final snapshot exactly; each runs in every owner mode:

    default   the engine's own bin thresholds
    coop      lite <= 16 < k_jac<1> <= 40 < k_jac<4> <= 400 < the wider owners and k_head
    skip      coop, frozen-stretch skipping from 16 events on (asserted: the owners recorded skipped spans)
    lane      every segment on one lane (k_lane)
    hotcold   coop, the hot / cold group stage with its radix passes at every batch size
    headoff   coop without the head owner

The CPU test at the end keeps the device tests from being vacuous: it plays the oracle again with every reload step
replaced by its counterfactual (the load omitted, the permuted list for a no-op, a load that also resets the other
kinds for a carry) and asserts that the decisions after the step differ on the resources the step is about.
"""
import numpy as np
import pytest

import reload_util as U
from sentinel_amd import _abi as A

gpu = pytest.mark.gpu

# the asynchronous script's switches: the late handoff of a grouped batch, the pipeline, both group stages
ASYNC_ENV = [{"SG_HANDOFF": h, "SG_PIPELINE": p, **({"SG_RADIX_BELOW": "0"} if r else {})}
             for h in ("1", "0") for p in ("1", "0") for r in (False, True)]


def _run(name, env, monkeypatch):
    sc, want = U.script(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return U.engine_play(sc, want)


@gpu
@pytest.mark.parametrize("mode", sorted(U.MODES))
@pytest.mark.parametrize("name", sorted(U.SCRIPTS))
def test_reload(name, mode, monkeypatch):
    sc, _ = U.script(name)
    if mode in sc.skip_modes:
        pytest.skip(sc.skip_modes[mode])
    spans = _run(name, U.MODES[mode], monkeypatch)
    if mode == "skip" and sc.once:  # (a batch in which two TRACEs name one ENTRY skips nothing: carry, async)
        assert spans > 0, "no frozen stretch was skipped"


@gpu
@pytest.mark.parametrize("env", ASYNC_ENV, ids=lambda e: "-".join("%s=%s" % (k[3:].lower(), v) for k, v in e.items()))
def test_reload_async_switches(env, monkeypatch):
    _run("async", {**U.COOP, **env}, monkeypatch)


# ---------------------------------------------------------------- CPU: the scripts reach what they are about
def _batches(steps, out):
    """[(step index, events, decisions)] of the batch and async steps."""
    res = []
    for i, st in enumerate(steps):
        if st[0] in ("batch", "async"):
            ev = st[1] if st[0] == "batch" else np.concatenate(st[1])
            res.append((i, ev, out[i][0]))
    return res


def _differ(steps, a, b, frm):
    """The resources with a decision that differs between two plays, in the batches from step frm on (up to the next
    load that resets the same state for both: simply all later batches)."""
    res = set()
    for (i, ev, da), (_, _, db) in zip(_batches(steps, a), _batches(steps, b)):
        if i > frm:
            res |= set(int(r) for r in np.unique(ev["res_id"][da != db]))
    return res


@pytest.mark.parametrize("name", sorted(U.SCRIPTS))
def test_reload_scripts_shape(name):
    """(CPU, oracle only) every reload step of the script matters, and its batches have the sizes, spans, verdicts and
    references that the module's docstring names."""
    sc, want = U.script(name)
    steps = sc.steps
    assert len(sc.skip_modes) <= 1, "a script exempts no more owner modes than it documents as unreachable"
    bs = _batches(steps, want)
    # sizes: a batch is 6,000 .. 10,000 events over 1.2 .. 2 s; every class reaches its segment length in every batch
    n_total = 0
    for i, ev, dec in [(i, p, None) for i, st in enumerate(steps) if st[0] in ("batch", "async")
                       for p in ([st[1]] if st[0] == "batch" else st[1])]:
        n_total += len(ev)
        assert 6_000 <= len(ev) <= 10_000, (i, len(ev))
        assert 1_150 <= int(ev["ts"][-1] - ev["ts"][0]) <= 2_000, (i, int(ev["ts"][-1] - ev["ts"][0]))
        cnt = np.bincount(ev["res_id"], minlength=len(U.NAMES))
        for c, rs in U.CLASSES.items():
            lo, hi = U.LIMITS[c]
            assert all(lo <= cnt[r] <= hi for r in rs), (i, c, cnt[list(rs)])
        assert set(np.unique(ev["count"])) == {1, 2, 3}
    assert n_total <= 66_000, n_total
    # verdicts
    st = np.concatenate([dec[ev["kind"] == A.EV_ENTRY] & 0xFF for _, ev, dec in bs])
    need = [A.PASS, A.BLOCK_FLOW, A.BLOCK_DEGRADE] + ([A.BLOCK_PARAM] if sc.has_param else [])
    for s in need:
        assert int((st == s).sum()) > 0, (name, s, np.bincount(st, minlength=8))
    if sc.has_rl:
        assert any(int((A.decision_wait(dec[ev["kind"] == A.EV_ENTRY]) > 0).sum()) for _, ev, dec in bs), "no wait word"
    # an EXIT after every reload names an ENTRY from before it
    base, seen = {}, 0
    for i, ev, _ in bs:
        base[i] = seen
        seen += len(ev)
    for k, stp in enumerate(steps):
        if stp[0] not in U.LOADS or not any(i < k for i in base):
            continue
        nxt = [(i, ev) for i, ev, _ in bs if i > k]
        if not nxt:
            continue
        i, ev = nxt[0]
        ex = ev[ev["kind"] == A.EV_EXIT]
        ref = (ex["aux"] & np.uint64(A.REF_NONE)).astype(np.int64)
        assert int(((ref != A.REF_NONE) & (ref < base[i])).sum()) > 0, (name, k)
        assert int((ref == A.REF_NONE).sum()) > 0 and int(((ref != A.REF_NONE) & (ref >= base[i])).sum()) > 0
    # the counterfactual of every reload step
    reloads = [k for k, stp in enumerate(steps) if stp[0] in U.LOADS and any(i < k for i in base)]
    for k in reloads:  # (sc.same: the list its kind loaded last, loaded again beside another kind's change)
        assert k in sc.cf or k in sc.same, "%s: load at step %d has no counterfactual" % (name, k)
    for k, (repl, about) in sorted(sc.cf.items()):
        other = U.oracle_play(steps[:k] + list(repl) + steps[k + 1:])
        other = other[:k] + [None] + other[k + len(repl):]
        diff = _differ(steps, want, other, k)
        for c, rs in U.CLASSES.items():
            mine = [r for r in about if r in rs]
            assert not mine or diff & set(mine), "%s: step %d changes no decision on the %s resources %s it is about " \
                "(it does on %s)" % (name, k, c, mine, sorted(diff))
    if name == "failed_load":  # the origin rule of the old list decides after the refused load
        i, ev, dec = [b for b in bs if len(steps[b[0]]) == 3][0]
        for r in steps[i][2]:
            m = (ev["res_id"] == r) & (ev["kind"] == A.EV_ENTRY)
            assert int(((dec[m] & 0xFF) == A.BLOCK_FLOW).sum()) > 0, r

