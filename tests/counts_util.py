"""Traces with acquire / exit / trace counts other than 1, and their oracle results (helper of test_gpu_counts.py).

tracegen writes count = 1 into every event; with_counts() redraws the counts of a finished trace.  reference() replays
such a trace through the oracle once per process and keeps what the device is compared with (the decision words, the
ClusterNode state of the sampled resources, the metric snapshots, the param thread counts), so the bin modes and
switches of one trace share one oracle run.
"""
import functools

import numpy as np

import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import tracegen as T

T0 = 1_700_000_000_000  # a multiple of 60 s: the "wide" events at T0 .. T0 + 399 share one 500 ms bucket

MIXES = {
    "MIXED": ((1, 2, 3, 7), (0.55, 0.25, 0.15, 0.05)),
    "ZERO": ((0, 1, 2, 5), (0.02, 0.58, 0.30, 0.10)),   # a zero-count ENTRY raises BF_ZERO_CNT
    "BIG": ((1, 2, 60, 65535), (0.70, 0.20, 0.08, 0.02)),
}
COUNT_SEED = 7
SIZE_CYCLE = (1, 2, 3, 64, 65, 127, 1000, 4097, 4096, 4095)  # test_many_small_batches_and_single_events


def with_counts(events, choices, p, seed, exit_own=0.0, trace_choices=None, zero_in=None):
    """A copy of the trace with one count per event drawn from choices (probabilities p).  An EXIT that names an ENTRY
    of the trace gets that ENTRY's count (Entry.exit() releases what the entry acquired), except a fraction exit_own of
    them, which keep their own draw (Entry.exit(count) with another count: addRtAndSuccess(rt, count) while the
    thread count moves by 1).  trace_choices: the TRACE counts are drawn from these instead, uniformly.  zero_in: batch
    boundaries; a batch that holds ENTRYs and drew no zero-count one gets its first ENTRY's count set to 0 (so that
    every batch, down to a call of one ENTRY, raises BF_ZERO_CNT)."""
    ev = np.array(events, dtype=A.EVENT_DTYPE, copy=True)
    n = len(ev)
    rng = np.random.default_rng(seed)
    cnt = rng.choice(np.asarray(choices, dtype=np.int64), size=n, p=np.asarray(p, dtype=np.float64))
    own = rng.random(n) < exit_own
    if trace_choices is not None:
        tdraw = rng.choice(np.asarray(trace_choices, dtype=np.int64), size=n)
        cnt = np.where(ev["kind"] == A.EV_TRACE, tdraw, cnt)
    if zero_in is not None:
        ent = ev["kind"] == A.EV_ENTRY
        for a, b in zip(zero_in[:-1], zero_in[1:]):
            if ent[a:b].any() and not (ent[a:b] & (cnt[a:b] == 0)).any():
                cnt[a + int(np.argmax(ent[a:b]))] = 0
    ref = (ev["aux"] & np.uint64(A.REF_NONE)).astype(np.int64)
    named = (ev["kind"] == A.EV_EXIT) & (ref != A.REF_NONE) & (ref < n)
    named[named] = ev["kind"][ref[named]] == A.EV_ENTRY
    follow = named & ~own
    cnt[follow] = cnt[ref[follow]]  # (an ENTRY's count is its own draw: no chain of copies)
    ev["count"] = cnt.astype(np.uint16)
    return ev


# name -> (config, Workload kwargs, fraction of ENTRYs prioritized)
TRACES = {
    "c2": (2, dict(n_entries=400_000), 0.0),
    "c3": (3, dict(n_entries=400_000, n_res=20_000, variant=T.V_WARM_RL), 0.0),
    "c4": (4, dict(n_entries=400_000, n_res=50_000), 0.0),
    "c2hot": (2, dict(n_entries=300_000, n_res=12), 0.0),
    "c4hot": (4, dict(n_entries=300_000, n_res=12), 0.0),
    "c5": (5, dict(n_entries=400_000, n_param_values=50_000, variant=T.V_HOT | T.V_THREAD), 0.0),
    "c5evict": (5, dict(n_entries=400_000, n_res=16, n_param_values=200_000,
                        variant=T.V_UNIFORM | T.V_HOT | T.V_THREAD), 0.0),
    "c6": (6, dict(n_entries=300_000, n_res=2_000, n_param_values=20_000), 0.0),
    "c4long": (4, dict(n_entries=300_000, n_res=3_000, rate=2000.0), 0.0),
    "c4small": (4, dict(n_entries=20_000, n_res=2_000), 0.0),
    "prio1": (1, dict(), 0.3),
    "prio2": (2, dict(n_entries=200_000), 0.2),
}
PARAM_TRACES = ("c5", "c5evict", "c6")


@functools.lru_cache(maxsize=None)
def workload(name):
    """The generated workload; a prioritized trace has its ENTRYs picked as test_gpu_parity._run_prioritized picks."""
    config, kw, frac = TRACES[name]
    w = T.Workload(config, **kw)
    if frac:
        ev = w.events
        rng = np.random.default_rng(11 + config)
        pick = (ev["kind"] == A.EV_ENTRY) & (rng.random(len(ev)) < frac)
        ev["flags"] = np.where(pick, ev["flags"] | A.F_PRIORITIZED, ev["flags"])
    return w


def cuts_of(n, batches):
    """Batch boundaries: np.linspace as test_gpu_parity._replay, or the size cycle of the small-call test."""
    if batches != "cycle":
        return np.linspace(0, n, batches + 1).astype(np.int64)
    c, k = [0], 0
    while c[-1] < n:
        c.append(min(n, c[-1] + SIZE_CYCLE[k % len(SIZE_CYCLE)]))
        k += 1
    return np.asarray(c, dtype=np.int64)


def sample(ev, n_res, k=300, seed=0):
    """The hottest 50 and k random touched resources (test_gpu_parity._sample)."""
    cnt = np.bincount(ev["res_id"], minlength=n_res)
    hot = np.argsort(-cnt)[:50]
    rng = np.random.default_rng(seed)
    touched = np.nonzero(cnt)[0]
    rnd = rng.choice(touched, size=min(k, len(touched)), replace=False)
    return np.unique(np.concatenate([hot, rnd]))


def hot_values(ev, n_res, n_hot=8, n_val=10):
    """[(resource, its n_val most frequent args[0] keys)] of the n_hot hottest resources."""
    cnt = np.bincount(ev["res_id"], minlength=n_res)
    out = []
    for r in np.argsort(-cnt)[:n_hot]:
        m = (ev["res_id"] == r) & (ev["kind"] == A.EV_ENTRY) & ((ev["flags"] & A.F_HAS_ARG) != 0)
        keys, c = np.unique(ev["aux"][m], return_counts=True)
        out.append((int(r), [int(k) for k in keys[np.argsort(-c, kind="stable")[:n_val]]]))
    return out


class Ref:
    """One trace and what the oracle made of it."""


def reference(name, mix, batches=3, exit_own=0.0, trace_choices=None, snapshots=False):
    """The trace `name` with the counts of `mix`, replayed through the oracle in `batches` (once per process)."""
    return _reference(name, mix, batches, exit_own, trace_choices, snapshots)


@functools.lru_cache(maxsize=None)
def _reference(name, mix, batches, exit_own, trace_choices, snapshots):
    w = workload(name)
    choices, p = MIXES[mix]
    r = Ref()
    r.w = w
    r.cuts = cuts_of(len(w.events), batches)
    r.ev = with_counts(w.events, choices, p, COUNT_SEED, exit_own=exit_own, trace_choices=trace_choices,
                       zero_in=r.cuts if mix == "ZERO" else None)
    orc = O.Oracle(max_slot_chain_size=0)
    w.install(orc)
    r.do = np.concatenate([orc.submit(r.ev[a:b]) for a, b in zip(r.cuts[:-1], r.cuts[1:])])
    r.sample = sample(r.ev, w.n_res)
    r.nodes = {int(x): orc.read_node(int(x)) for x in r.sample}
    r.snapshots = {}
    if snapshots:
        for now in (w.t_end + 10, w.t_end + 1500, w.t_end + 70000):
            r.snapshots[now] = sorted_snapshot(orc.snapshot(now, cap=1 << 18))
    r.threads = []
    if name in PARAM_TRACES:  # last: the oracle's get moves the value in its LRU order
        r.threads = [(res, keys, [orc.param_thread_count(res, 0, k) for k in keys])
                     for res, keys in hot_values(r.ev, w.n_res)]
    orc.close()
    return r


def sorted_snapshot(a):
    return a[np.lexsort((a["timestamp"], a["res_id"]))]  # as test_snapshot_matches_oracle sorts


def entry_status(r):
    return r.do[r.ev["kind"] == A.EV_ENTRY] & 0xFF


# ---------------------------------------------------------------- sums past 2^32: one resource, one bucket
WIDE_COUNT = 65535
# n ENTRYs, the QPS rule's count.  "block" (count 1): 0 + 65,535 > 1 blocks every ENTRY, yet an acquire of 1 would pass, so the
# round is not saturated and the Jacobi iteration decides it; "block_sat": the first ENTRY fits (0 + 65,535 > 65,535 is
# false) and saturates the round, the other 299,999 block in one frozen stretch
WIDE_CASES = {"pass": (70_000, 1e13), "block": (300_000, 1.0), "block_sat": (300_000, 65535.0)}


def wide_events(n):
    ev = np.zeros(n, dtype=A.EVENT_DTYPE)
    ev["ts"] = T0 + (np.arange(n, dtype=np.int64) * 400 // n)
    ev["count"] = WIDE_COUNT
    ev["kind"] = A.EV_ENTRY
    return ev


def wide_rules(case, origin=False):
    rules = [A.flow_rule("wide", WIDE_CASES[case][1])]
    if origin:  # a rule of origin app-0: FlowRuleChecker reads the origin node, so it exists
        rules.append(A.flow_rule("wide", WIDE_CASES[case][1], limit_app="app-0"))
    return rules


@functools.lru_cache(maxsize=None)
def wide_reference(case, origin=False):
    r = Ref()
    r.ev = wide_events(WIDE_CASES[case][0])
    orc = O.Oracle(max_slot_chain_size=0)
    assert orc.register("wide") == 0
    orc.load_flow_rules(wide_rules(case, origin))
    r.ext = None
    if origin:
        r.ext = np.zeros(len(r.ev), dtype=A.EXT_DTYPE)
        r.ext["origin_id"] = orc.intern_origin("app-0")
        r.ext["context_id"] = orc.intern_context("ctx-0")
        r.do = orc.submit_ex(r.ev, r.ext)
        r.origin_node = orc.read_origin_node(0, "app-0")
        r.context_node = orc.read_default_node(0, "ctx-0")
    else:
        r.do = orc.submit(r.ev)
    r.node = orc.read_node(0)
    orc.close()
    return r
