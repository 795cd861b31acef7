"""bench.py's plain run and --dump-outputs: what a plain run leaves out, and what the dump holds.

CPU: dump_outputs on a stand-in engine -- every word of a small batch, a seeded sample of a large one, float64
files.  GPU (-m gpu): one plain `bench.py --gpus 1` at a small C4 shape with --dump-outputs: the result line keeps
its headline fields, the --full fields are null, and the dumped decisions and node state are the oracle's for the
same batches (the bench's stream rebuilt on the host).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from sentinel_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Nodes:
    def read_node(self, r):
        return {"second": np.full((8, 8), r, np.int64), "minute": np.full((60, 8), -r, np.int64)}


def _events(n, n_res):
    ev = np.zeros(n, dtype=A.EVENT_DTYPE)
    ev["res_id"] = np.random.default_rng(1).integers(0, n_res, n)
    return ev


def test_dump_small_batch_is_whole(tmp_path):
    import torch
    out = torch.arange(100, dtype=torch.int32) - 50  # words above 2^31 are negative in the int32 tensor
    ev = _events(100, 300)
    bench.dump_outputs(str(tmp_path), _Nodes(), out, 60, ev, 300)
    dec = np.load(tmp_path / "decisions.npy")
    assert dec.dtype == np.float64
    assert np.array_equal(dec, (np.arange(60) - 50).astype(np.int32).view(np.uint32).astype(np.float64))
    sec, mnt = np.load(tmp_path / "node_second.npy"), np.load(tmp_path / "node_minute.npy")
    assert sec.dtype == mnt.dtype == np.float64
    _, first = np.unique(ev["res_id"], return_index=True)
    lead = ev["res_id"][np.sort(first)]  # the trace's distinct resources in order of appearance
    assert sec.shape == (len(lead) + bench.DUMP_NODES, 8, 8) and mnt.shape == (len(sec), 60, 8)
    assert np.array_equal(sec[:len(lead), 0, 0], lead)
    assert np.array_equal(mnt[:, 0, 0], -sec[:, 0, 0])


def test_dump_large_batch_is_a_fixed_sample(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    out = torch.arange(50_000, dtype=torch.int32)
    ev = _events(10, 5)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), _Nodes(), out, 40_000, ev, 5, "_rank1")
    a, b = np.load(tmp_path / "a" / "decisions_rank1.npy"), np.load(tmp_path / "b" / "decisions_rank1.npy")
    assert np.array_equal(a, b) and a.shape == (1000,)
    assert (np.diff(a) >= 0).all() and a.max() < 40_000 and len(np.unique(a)) > 900  # spread positions of [0, m)


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs == "" and (a.steps, a.warmup) == (3, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_dumps_the_oracles_outputs(tmp_path):
    import pyoracle as O
    from sentinel_amd import tracegen as T
    n_res, gb, B, S, steps, warmup = 20_000, 1 << 18, 2, 2, 2, 1
    env = dict(os.environ)
    for key in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(key, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--resources", str(n_res),
                        "--batch-events", str(gb), "--base-batches", str(B), "--sub-batches", str(S), "--steps",
                        str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-4000:]
    j = json.loads(lines[0])
    assert j["metric"].startswith("decided entries/sec") and j["unit"] == "entries/s" and j["higher_is_better"] is True
    assert j["dtype"] == "int64/f64" and (j["steps"], j["warmup"], j["n_gpus"]) == (steps, warmup, 1)
    assert j["value"] > 0 and j["ms_per_step"] > 0
    assert abs(j["value"] * j["ms_per_step"] / 1e3 - j["config"]["entries_per_step"]) < 1e-6 * j["config"]["entries_per_step"]
    assert j["full"] is False and j["cpu_baseline"] is None and j["configs"] is None
    assert j["roofline"]["stream_copy_GBps"] is None and j["roofline"]["frac"] > 0

    # the bench's stream on the host: (warmup + steps) * S batches, batch g = base batch g % B shifted by g // B spans
    w, ev = bench.make_trace(n_res, gb, B, T.SEED_BASE + 4)
    tspan = int(ev["ts"][-1] - ev["ts"][0]) + 1000
    orc = O.Oracle(max_slot_chain_size=0)
    w.install(orc)
    for g in range((warmup + steps) * S):
        b, k = g % B, g // B
        e = ev[b * gb:(b + 1) * gb].copy()
        e["ts"] += k * tspan
        isref = (e["kind"] != A.EV_ENTRY) & ((e["aux"] & np.uint64(A.REF_NONE)) != np.uint64(A.REF_NONE))
        e["aux"] = np.where(isref, e["aux"] + np.uint64(k * len(ev)), e["aux"])
        want = orc.submit(e)
    assert np.array_equal(np.load(tmp_path / "decisions.npy"), want.astype(np.float64))
    head = ev["res_id"][:1 << 16]
    _, first = np.unique(head, return_index=True)
    sec, mnt = np.load(tmp_path / "node_second.npy"), np.load(tmp_path / "node_minute.npy")
    for i, r in enumerate(head[np.sort(first)][:bench.DUMP_NODES]):
        node = orc.read_node(int(r))
        # (rows 0-1 of `second` are the two buckets of the second window, as the parity tests compare it)
        assert np.array_equal(sec[i][:2], node["second"][:2]) and np.array_equal(mnt[i], node["minute"]), int(r)
