"""The reference for the global inbound node (Constants.ENTRY_NODE; helper of test_inbound_host.py and
test_gpu_inbound.py).

The oracle has no ENTRY_NODE and needs none: ENTRY_NODE is a ClusterNode with no rules that sees a derived stream.
derive() builds that stream from a trace and the *oracle's* decisions of it (never the device's):

    an IN ENTRY that passed          -> a plain ENTRY of resource 0
    a blocked ENTRY (2, 3, 4, 6, 7)  -> an ENTRY with SG_F_BLOCKED_UPSTREAM (the replay oracle counts the block)
    an SG_PASS_WAIT ENTRY            -> an ENTRY with count 0 (the thread alone; its pass of 0 adds nothing)
    SG_NO_CHECK ENTRY, OUT event, TRACE -> dropped
    an EXIT                          -> kept iff its ENTRY passed, its reference renumbered

Replay cuts the stream at the trace's batch boundaries and feeds a second pyoracle.Oracle with one registered resource
and no rules; that oracle's read_node(0), snapshot and metric(0, now, which) are the reference.

The count-0 stand-in of an SG_PASS_WAIT touches a window (LeapArray.currentWindow) where the real node would not, so
derive() asserts that every 500 ms and 1 s window holding one also holds a counted update: a condition on the input.
"""
import numpy as np

import pyoracle as O
from sentinel_amd import _abi as A

BLOCKS = (A.BLOCK_FLOW, A.BLOCK_DEGRADE, A.BLOCK_PARAM, A.BLOCK_UPSTREAM, A.BLOCK_AUTHORITY)
NAME = "__total_inbound_traffic__"


def mark_out(ev, n_res, frac=0.3, seed=5, out_res=None):
    """A copy of the trace with SG_F_ENTRY_OUT on every ENTRY and EXIT of a random `frac` of the resources (an EXIT
    carries the flag iff its ENTRY did); returns (events, the OUT resources)."""
    ev = np.array(ev, dtype=A.EVENT_DTYPE, copy=True)
    if out_res is None:
        rng = np.random.default_rng(seed)
        out_res = np.nonzero(rng.random(n_res) < frac)[0]
    is_out = np.zeros(n_res, dtype=bool)
    is_out[np.asarray(out_res, dtype=np.int64)] = True
    m = is_out[ev["res_id"]] & (ev["kind"] != A.EV_TRACE)
    ev["flags"] = np.where(m, ev["flags"] | A.F_ENTRY_OUT, ev["flags"]).astype(np.uint8)
    return ev, np.asarray(out_res)


class Derived:
    """events: the derived stream; cuts: its batch boundaries; waits / updates: what it holds."""


def derive(ev, do, cuts, null_ctx=None, check=True):
    """ev: the whole trace in submission order from the engine's first event on (an EXIT's aux names its ENTRY by
    that index); do: the oracle's decision words; cuts: the trace's batch boundaries; null_ctx: per event, its
    context is a NullContext (no statistics)."""
    n = len(ev)
    st = (np.asarray(do) & 0xFF).astype(np.int64)
    kind = ev["kind"]
    out = (ev["flags"] & A.F_ENTRY_OUT) != 0
    if null_ctx is not None:
        out = out | np.asarray(null_ctx, dtype=bool)
    ref = (ev["aux"] & np.uint64(A.REF_NONE)).astype(np.int64)
    entry = kind == A.EV_ENTRY
    passed = entry & ((st == A.PASS) | (st == A.PASS_WAIT))
    # a resource has its chain from its first checked ENTRY on (an SG_REF_NONE EXIT is effective iff it has one)
    first_chain = {}
    for i in np.nonzero(entry & (st != A.NO_CHECK))[0]:
        first_chain.setdefault(int(ev["res_id"][i]), int(i))
    keep = np.zeros(n, dtype=bool)
    keep |= entry & ~out & (st != A.NO_CHECK)
    ex = np.nonzero((kind == A.EV_EXIT) & ~out)[0]
    named = ex[ref[ex] != A.REF_NONE]
    ok = named[(ref[named] < named) & (ref[named] >= 0)]
    keep[ok[passed[ref[ok]]]] = True
    for i in ex[ref[ex] == A.REF_NONE]:
        keep[i] = first_chain.get(int(ev["res_id"][i]), n) < i
    idx = np.nonzero(keep)[0]
    new_of = np.full(n, -1, dtype=np.int64)
    new_of[idx] = np.arange(len(idx))
    d = np.zeros(len(idx), dtype=A.EVENT_DTYPE)
    d["ts"] = ev["ts"][idx]
    d["res_id"] = 0
    d["kind"] = kind[idx]
    s = st[idx]
    is_e = kind[idx] == A.EV_ENTRY
    wait = is_e & (s == A.PASS_WAIT)
    d["count"] = np.where(wait, 0, ev["count"][idx])
    d["flags"] = np.where(is_e & np.isin(s, BLOCKS), A.F_BLOCKED_UPSTREAM, 0).astype(np.uint8)
    r = ref[idx]
    nref = np.where(r == A.REF_NONE, A.REF_NONE, new_of[np.minimum(r, n - 1)])
    rt_raw = (ev["aux"][idx] >> np.uint64(48)).astype(np.uint64)
    d["aux"] = np.where(is_e, np.uint64(0), (rt_raw << np.uint64(48)) | nref.astype(np.uint64))
    assert not ((~is_e) & (r != A.REF_NONE) & (nref < 0)).any(), "a kept EXIT names a dropped ENTRY"
    assert len(d) == 0 or d["kind"][0] == A.EV_ENTRY, "the stream must open with an ENTRY (the replay node's chain)"
    if check:
        for wlen in (500, 1000):
            w_wait = np.unique(d["ts"][wait] // wlen)
            w_real = np.unique(d["ts"][~wait] // wlen)
            lone = np.setdiff1d(w_wait, w_real)
            assert len(lone) == 0, "%d %d-ms windows hold an SG_PASS_WAIT and no counted update (first %d)" % (
                len(lone), wlen, lone[0] * wlen)
    x = Derived()
    x.events = d
    x.cuts = np.searchsorted(idx, np.asarray(cuts, dtype=np.int64))
    x.waits = int(wait.sum())
    x.updates = len(d)
    x.blocks = int((d["flags"] != 0).sum())
    x.exits = int((~is_e).sum())
    return x


class Replay:
    """The replay oracle, fed batch by batch: feed(k) submits the derived events of the trace's batch k."""

    def __init__(self, derived, **cfg):
        self.d = derived
        self.orc = O.Oracle(max_slot_chain_size=0, **cfg)
        assert self.orc.register(NAME) == 0

    def feed(self, k):
        a, b = int(self.d.cuts[k]), int(self.d.cuts[k + 1])
        if b > a:
            self.orc.submit(self.d.events[a:b])

    def node(self):
        return self.orc.read_node(0)

    def close(self):
        self.orc.close()


def assert_node_equal(got, want, msg=""):
    """got: Engine.read_inbound_node (or the model's dict); want: the replay oracle's read_node(0)."""
    np.testing.assert_array_equal(got["second"][:2], want["second"][:2], err_msg="second window " + msg)
    np.testing.assert_array_equal(got["minute"], want["minute"], err_msg="minute window " + msg)
    np.testing.assert_array_equal(got["borrow"], want["borrow"], err_msg="borrow ring " + msg)
    assert got["thread"] == want["thread"], "curThreadNum %d != %d %s" % (got["thread"], want["thread"], msg)
