"""The value-parallel param owner's walk on the CPU (no GPU needed): tests/ptok_host.cpp compiles
sentinel_amd/csrc/ptok.h (the per-value walk pt_step, the stamp merge pt_merge and the eligibility predicate
pt_clock_ok, all __host__ __device__: the very code k_ptok_chain / k_ptok_keys / k_ptok_elig run) and drives random
calls through it next to a literal serial restatement of k_ptok_flow's loop over a host value table: hot items,
AVG_LOCAL, a threshold of 0, acquire 1 to 3, idle gaps of whole intervals, values that return at w + interval - 1
and at w + interval.  After every call the results, the flows' stamps and the live (flow, value) pairs with their
stamps and counts are equal.  With a clock that goes back between calls, or multi-value requests, the predicate must
refuse exactly the flows concerned (they then take the serial loop on both sides).
ClusterParamFlowChecker.acquireClusterToken: csrv/flow/ClusterParamFlowChecker.java:42-88."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ptok_host.cpp")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("ptok") / "ptok_host")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-o", out, SRC], check=True,
                   capture_output=True)
    return out


# (sampleCount, windowIntervalMs): one bucket, two, the common ten, the device bound of sixteen
SHAPES = [(1, 200), (1, 1000), (2, 1000), (2, 60), (10, 1000), (10, 100), (5, 500), (16, 1600), (16, 160)]
SEEDS = [1, 2, 3, 4]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-i%d" % s)
def test_walk_by_value_equals_the_serial_owner(binary, shape):
    for seed in SEEDS:
        r = subprocess.run([binary, str(shape[0]), str(shape[1]), str(seed * 7919 + shape[1]), "0"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("mode", [1, 2], ids=["clock-back", "multi-value"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-i%d" % s)
def test_predicate_refuses_exactly_the_coupled_flows(binary, shape, mode):
    for seed in SEEDS:
        r = subprocess.run([binary, str(shape[0]), str(shape[1]), str(seed * 104729 + shape[0]), str(mode)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
