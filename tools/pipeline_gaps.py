#!/usr/bin/env python3
"""How long the two pipeline streams stand empty between batches (Engine.gap_log) on the C4 trace as bench.py runs
it: base batches of 2^25 events in HBM, one untimed batch, then sg_submit_async back to back and one sg_sync.

  python tools/pipeline_gaps.py [--steps 24] [--base-batches 4] [--batch-events 33554432]

SG_LIB_PATH selects the library (it needs the sgx_gap_log export), SG_HANDOFF / SG_PIPELINE the order of the handoff.
Prints mean / median / max of the group-stream idle time, the decide-stream idle time and the three stage times, in
ms a batch, and the wall time a batch."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=24)
    p.add_argument("--base-batches", type=int, default=4)
    p.add_argument("--batch-events", type=int, default=1 << 25)
    p.add_argument("--resources", type=int, default=1 << 20)
    a = p.parse_args()
    import torch
    import bench
    from sentinel_amd import engine as E
    from sentinel_amd import tracegen as T

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gb, B = a.batch_events, a.base_batches
    w, ev = bench.make_trace(a.resources, gb, B, T.SEED_BASE + 4)
    eng = E.Engine(device=0, max_resources=a.resources, max_slot_chain_size=0, param_table_log2=16,
                   status_ring_log2=28, max_batch_events=gb)
    w.install(eng)
    tspan = int(ev["ts"][-1] - ev["ts"][0]) + 1000
    base = torch.from_numpy(np.ascontiguousarray(ev).view(np.uint8)).to(dev)
    base64 = base.view(torch.int64).view(-1, 3)
    n_base = len(ev)
    n = 1 + a.steps
    buf = torch.empty((n * gb, 3), dtype=torch.int64, device=dev)
    out = torch.empty(gb, dtype=torch.int32, device=dev)
    for g in range(n):
        b, k = g % B, g // B
        bench.shifted_batch(base64, b * gb, (b + 1) * gb, k, tspan, n_base, buf[g * gb:(g + 1) * gb])
    torch.cuda.synchronize()
    ptr = buf.data_ptr()
    eng.submit_ptr(ptr, gb, out.data_ptr(), sync=True)  # untimed
    eng.timing_log()
    eng.gap_log()
    t0 = time.perf_counter()
    for g in range(1, n):
        eng.submit_ptr(ptr + g * gb * 24, gb, out.data_ptr(), sync=False)
    eng.sync()
    wall = (time.perf_counter() - t0) * 1e3 / a.steps
    st, gp = eng.timing_log(), eng.gap_log()
    # the first timed batch's gaps hold the host's pause after the untimed batch
    gp = gp[1:]
    print("library %s  SG_HANDOFF=%s SG_PIPELINE=%s" % (os.path.relpath(E.LIB_PATH, ROOT),
                                                        os.environ.get("SG_HANDOFF", "(unset)"),
                                                        os.environ.get("SG_PIPELINE", "(unset)")))
    print("%d batches of %d events, wall %.3f ms a batch" % (a.steps, gb, wall))

    def line(name, x):
        x = x[np.isfinite(x)]
        if len(x) == 0:
            print("%-24s (no samples)" % name)
            return
        print("%-24s mean %.3f  median %.3f  max %.3f  ms  (%d batches)" % (name, x.mean(), np.median(x), x.max(), len(x)))

    line("group-stream idle", gp[:, 0])
    line("decide-stream idle", gp[:, 1])
    line("group stage", st[:, 0])
    line("decide stage", st[:, 1])
    line("post stage", st[:, 2])
    eng.close()
    w.close()


if __name__ == "__main__":
    main()
