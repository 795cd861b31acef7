"""inbound_util's reference for the global inbound node against a sequential model (no GPU).

The helper derives a one-resource stream from a trace and the oracle's decisions and replays it through a second
oracle.  Here that node is compared with a small event-by-event Python model of what StatisticSlot does on
Constants.ENTRY_NODE (StatisticSlot.java:72-76, 89-92, 107-110, 158-161) over LeapArray.currentWindow
(LeapArray.java:117-208), on the traces the GPU tests use; and the helper's precondition (every window that holds an
SG_PASS_WAIT stand-in also holds a counted update) is shown to fire on a counter-example.
"""
import numpy as np
import pytest

import counts_util as CU
import inbound_util as IU
import pyoracle as O
from sentinel_amd import _abi as A
from sentinel_amd import tracegen as T

MAX_RT = 4900


class Model:
    """ENTRY_NODE, one event at a time: buckets are [ws, pass, block, exc, succ, rt, occ, minRt]."""

    def __init__(self):
        self.sec, self.minute, self.thread, self.chain = [None] * 2, [None] * 60, 0, set()

    @staticmethod
    def _cur(arr, t, wlen):
        ws = t - t % wlen
        b = arr[(t // wlen) % len(arr)]
        if b is None or ws > b[0]:
            b = arr[(t // wlen) % len(arr)] = [ws, 0, 0, 0, 0, 0, 0, MAX_RT]
        return b if ws == b[0] else [ws, 0, 0, 0, 0, 0, 0, MAX_RT]  # the clock went back: a detached bucket

    def add(self, t, field, v, rt=None):
        for arr, wlen in ((self.sec, 500), (self.minute, 1000)):
            b = self._cur(arr, t, wlen)
            b[field] += v
            if rt is not None:
                b[5] += rt
                b[7] = min(b[7], rt)

    def run(self, ev, do, a, b):
        st = do & 0xFF
        chain = self.chain
        for i in range(a, b):
            k, t, c, res = int(ev["kind"][i]), int(ev["ts"][i]), int(ev["count"][i]), int(ev["res_id"][i])
            s = int(st[i])
            if k == A.EV_ENTRY and s != A.NO_CHECK:
                chain.add(res)
            if k == A.EV_TRACE or (int(ev["flags"][i]) & A.F_ENTRY_OUT):
                continue
            if k == A.EV_ENTRY:
                if s == A.PASS:
                    self.add(t, 1, c)
                if s in (A.PASS, A.PASS_WAIT):
                    self.thread += 1
                elif s != A.NO_CHECK:
                    self.add(t, 2, c)
            else:
                ref = int(ev["aux"][i]) & A.REF_NONE
                eff = res in chain if ref == A.REF_NONE else int(st[ref]) in (A.PASS, A.PASS_WAIT)
                if eff:
                    self.add(t, 4, c, rt=min(int(ev["aux"][i]) >> 48, MAX_RT))
                    self.thread -= 1

    def state(self):
        def arr(bs, n):
            out = np.zeros((n, 8), dtype=np.int64)
            out[:, 0] = -1
            for j, b in enumerate(bs):
                if b is not None:
                    out[j] = b
            return out
        bor = np.zeros((8, 8), dtype=np.int64)
        bor[:, 0] = -1
        return {"second": arr(self.sec, 8), "minute": arr(self.minute, 60), "borrow": bor, "thread": self.thread}


def _c4_60k():
    w = T.Workload(4, n_entries=60_000, n_res=2_000)
    return w, w.events


def _named(name):
    w = CU.workload(name)
    return w, w.events


@pytest.mark.parametrize("trace", ["c4_60k", "prio2", "prio1"])
def test_replayed_stream_equals_the_sequential_model(trace):
    w, ev0 = _c4_60k() if trace == "c4_60k" else _named(trace)
    ev, out_res = IU.mark_out(ev0, w.n_res, frac=0.3 if w.n_res > 1 else 0.0)
    cuts = CU.cuts_of(len(ev), 3)
    orc = O.Oracle(max_slot_chain_size=0)
    w.install(orc)
    do = np.concatenate([orc.submit(ev[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    orc.close()
    d = IU.derive(ev, do, cuts)
    assert d.updates > 0 and d.exits > 0 and (w.n_res == 1 or len(out_res) > 0)
    if trace == "prio1":
        assert d.waits > 100
    rp = IU.Replay(d)
    m = Model()
    for k in range(3):
        rp.feed(k)
        m.run(ev, do, int(cuts[k]), int(cuts[k + 1]))
        IU.assert_node_equal(m.state(), rp.node(), "%s after batch %d" % (trace, k))
    if trace == "prio1":  # a 100 s span: the minute slots wrapped
        assert int(ev["ts"][-1] - ev["ts"][0]) > 60_000
    rp.close()


def test_a_lone_priority_wait_trips_the_precondition():
    # two ENTRYs 10 s apart; the second is declared SG_PASS_WAIT and is alone in its windows: the count-0 stand-in
    # would create buckets the real node never has, so the helper refuses the input
    ev = np.zeros(2, dtype=A.EVENT_DTYPE)
    ev["ts"] = [CU.T0, CU.T0 + 10_000]
    ev["count"] = 1
    do = np.array([A.PASS, A.PASS_WAIT | (100 << 16)], dtype=np.uint32)
    with pytest.raises(AssertionError, match="SG_PASS_WAIT and no counted update"):
        IU.derive(ev, do, [0, 2])
    d = IU.derive(ev, do, [0, 2], check=False)
    assert d.waits == 1 and d.updates == 2
    # ... and with a counted update in the same 500 ms window it is accepted
    ev3 = np.zeros(3, dtype=A.EVENT_DTYPE)
    ev3["ts"] = [CU.T0, CU.T0 + 10_000, CU.T0 + 10_001]
    ev3["count"] = 1
    d = IU.derive(ev3, np.array([A.PASS, A.PASS_WAIT, A.PASS], dtype=np.uint32), [0, 3])
    assert d.waits == 1 and d.updates == 3
