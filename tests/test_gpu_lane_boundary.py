"""The lane / J1 boundary (engine.cpp lane_max / lite_max, decide.hip k_seg_bin; DESIGN.md §5 "The lane / J1
boundary"): in a batch of at least SHARD_BATCH events with no bin pinned, on an engine without THREAD-grade /
rate-limiter head programs, a segment of k_lite's programs without param rules stays on a lane up to 512 events (256
before, and 256 still for every other program); the one-wave owner k_jac<1> takes it from 513 on.

Each child process replays a seeded trace through the engine and the oracle and requires equal decisions for every
batch and equal minute and second windows for the 30 busiest resources and every 997th touched one.  It runs with
SG_DEBUG=1 SG_PROF_BIN=2, so that the engine counts the segments k_jac<1> decided, and replays the trace through a
second engine with another limit to check the placement itself:

  SG_LANE_MAX=512, SG_LANE_MAX=1024    C4, 600,000 entries over 3,000 resources in three batches: every lane bin keeps
                                       segments of up to 512 / 1,024 events, which k_lite decides where k_jac<1> did.
                                       Every C4 program is k_lite<false>'s and SG_J1_MAX stays 4,096, so k_jac<1>
                                       decides exactly the resources with more events than the limit and at most 4,096
  SG_LITE_MAX=512                      C3 (2,000 resources, V_WARM_RL) in three batches: k_lite's programs up to 512
                                       events, k_lane's and k_head's up to 256, side by side.  Against SG_LITE_MAX=256
                                       k_jac<1> decides fewer segments, and at most the 257..512-event ones fewer
  no switch, "full"                    C4, one batch above SHARD_BATCH (3.2M entries over 30,000 resources): the default
                                       bins of a full batch, which a smaller batch (shard-sized bins) never gets:
                                       k_jac<1> decides exactly the resources with 513..4,096 events, and with
                                       SG_LITE_MAX=256 exactly those with 257..4,096
  no switch, "fullext"                 the same batch through sg_submit_ex with contexts and origins: the 257..512-event
                                       segments are lane ones on the long aux list (aux_early reads the smaller limit)
  no switch, "c3full"                  C3 in one batch above SHARD_BATCH: an engine with head programs keeps 256 for
                                       every lane bin, so k_jac<1> decides as many segments as with SG_LITE_MAX=256

Before any GPU work the child counts each resource's events per batch on the host and requires segments of 257..512
events (and of 513..1,024 for the C4 shapes) in every batch; the CPU test checks the same here.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARD_BATCH = 3 << 21  # engine.cpp: below it, the shard-sized bins
J1_MAX = 4096          # engine.cpp j1_max: the one-wave owner's longest segment
# config, entries, resources, batches
SHAPES = {"small": (4, 600_000, 3_000, 3), "c3": (3, 300_000, 2_000, 3), "full": (4, 3_200_000, 30_000, 1),
          "fullext": (4, 3_200_000, 30_000, 1), "c3full": (3, 3_200_000, 30_000, 1)}


def trace(shape):
    """(workload, batch cuts) of a shape."""
    from sentinel_amd import tracegen as T
    cfg, n_entries, n_res, nb = SHAPES[shape]
    w = T.Workload(cfg, n_entries=n_entries, n_res=n_res, **({"variant": T.V_WARM_RL} if cfg == 3 else {}))
    return w, np.linspace(0, len(w.events), nb + 1).astype(np.int64)


def segments_between(ev, cuts, n_res, lo, hi):
    """Over all batches: (resource, batch) pairs with more than lo and at most hi events."""
    n = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        cnt = np.bincount(ev["res_id"][a:b], minlength=n_res)
        n += int(((cnt > lo) & (cnt <= hi)).sum())
    return n


def holds_boundary_segments(shape, ev, cuts, n_res):
    c3 = SHAPES[shape][0] == 3
    for a, b in zip(cuts[:-1], cuts[1:]):  # half a wave of lanes of each class at the least, in every batch
        assert segments_between(ev, [a, b], n_res, 256, 512) >= 32
        assert c3 or segments_between(ev, [a, b], n_res, 512, 1024) >= 32
    if shape in ("full", "fullext", "c3full"):
        assert cuts[1] - cuts[0] >= SHARD_BATCH
    else:
        assert (np.diff(cuts) < SHARD_BATCH).all()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_traces_hold_boundary_segments(shape):
    w, cuts = trace(shape)
    holds_boundary_segments(shape, w.events, cuts, w.n_res)


CHILD = r"""
import ctypes as C
import os
import sys
sys.path[:0] = [%(root)r, %(root)r + '/oracle', %(root)r + '/tests']
import numpy as np
import pyoracle as O
from sentinel_amd import engine as E
from sentinel_amd import tracegen as T
import test_gpu_lane_boundary as L
shape, other = %(shape)r, %(other)r
w, cuts = L.trace(shape)
ev = w.events
L.holds_boundary_segments(shape, ev, cuts, w.n_res)
parts = list(zip(cuts[:-1], cuts[1:]))
ext_on = shape == "fullext"


def replay(x, ext):
    if ext_on:
        return [x.submit_ex(ev[a:b], ext[a:b]) for a, b in parts]
    return [x.submit(ev[a:b]) for a, b in parts]


def engine(env):
    # the library reads the switches once per engine
    for k in ("SG_LANE_MAX", "SG_LITE_MAX"):
        os.environ.pop(k, None)
    for kv in env.split():
        k, v = kv.split("=")
        os.environ[k] = v
    eng = E.Engine(max_resources=w.n_res, max_slot_chain_size=0, status_ring_log2=24, max_batch_events=1 << 23,
                   **({"aux_node_capacity": 1 << 20} if ext_on else {}))
    w.install(eng)
    ext = None
    if ext_on:
        io, ic = w.intern_names(eng)
        ext = T.ext_for(ev, io, ic, seed=T.SEED_BASE + 78)
    return eng, ext


def j1_segments(eng):
    # SG_DEBUG=1 SG_PROF_BIN=2: [4] counts the segments k_jac<1> decided (decide.hip k_jac)
    fn = E.lib().sgx_debug_counters
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    buf = (C.c_ulonglong * 64)()
    assert fn(eng.h, buf, 64) == 64
    return int(buf[4])


eng, ext = engine(%(env)r)
if len(parts) == 1:  # a full batch: eight oracles, resources partitioned among them (seconds instead of ten)
    orc = O.PartitionedOracle(w, 8, max_slot_chain_size=0)
    if ext_on:
        for o in orc.orcs:
            w.intern_names(o)
else:
    orc = O.Oracle(max_slot_chain_size=0)
    w.install(orc)
dg, do = replay(eng, ext), replay(orc, ext)
for (a, b), g, o in zip(parts, dg, do):
    bad = np.nonzero(g != o)[0]
    assert not len(bad), ("mismatch", int(a + bad[0]), len(bad))
cnt = np.bincount(ev["res_id"], minlength=w.n_res)
for r in list(np.argsort(-cnt)[:30]) + list(np.nonzero(cnt)[0][::997]):
    g, o = eng.read_node(int(r)), orc.read_node(int(r))
    assert np.array_equal(g["minute"], o["minute"]) and np.array_equal(g["second"][:2], o["second"][:2]), r
n_this = j1_segments(eng)
eng.close()
# the placement: the same trace with the other limit
eng2, ext2 = engine(other)
d2 = replay(eng2, ext2)
assert all(np.array_equal(g, h) for g, h in zip(dg, d2))
n_other = j1_segments(eng2)
eng2.close()
print("j1 segments", n_this, n_other)
between = lambda lo: L.segments_between(ev, cuts, w.n_res, lo, L.J1_MAX)
if shape == "small":  # every program k_lite<false>'s: the limit alone places a segment
    assert n_this == between(int(%(env)r.split("=")[1])) and n_other == between(256), (n_this, n_other)
elif shape in ("full", "fullext"):
    assert n_this == between(512) and n_other == between(256), (n_this, n_other, between(512), between(256))
elif shape == "c3":  # some programs are k_lite's, some are not
    assert 0 < n_other - n_this <= L.segments_between(ev, cuts, w.n_res, 256, 512), (n_this, n_other)
else:  # c3full: head programs, the longer limit is off
    assert n_this == n_other > 0, (n_this, n_other)
print("ok", len(ev))
"""

# (environment, shape, environment of the second engine)
CASES = [("SG_LANE_MAX=512", "small", "SG_LANE_MAX=256"), ("SG_LANE_MAX=1024", "small", "SG_LANE_MAX=256"),
         ("SG_LITE_MAX=512", "c3", "SG_LITE_MAX=256"), ("", "full", "SG_LITE_MAX=256"),
         ("", "fullext", "SG_LITE_MAX=256"), ("", "c3full", "SG_LITE_MAX=256")]


@pytest.mark.gpu
@pytest.mark.parametrize("env,shape,other", CASES)
def test_lane_boundary_parity(env, shape, other):
    child_env = dict(os.environ)
    for k in ("SG_LANE_MAX", "SG_LITE_MAX", "SG_J1_MAX", "SG_J4_MAX", "SG_J1_STREAM", "SG_DEBUG_FLAGS"):
        child_env.pop(k, None)
    child_env.update({"SG_DEBUG": "1", "SG_PROF_BIN": "2"})
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "shape": shape, "env": env, "other": other}],
                       env=child_env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0 and "\nok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
