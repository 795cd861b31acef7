"""The token server's value table code on the CPU (no GPU needed): tests/pvtab_host.cpp compiles
sentinel_amd/csrc/pvtab.h (slot hash, probe, dead-slot rule and capacity policy, all __host__ __device__) and
drives a host table next to a brute-force map that never forgets a (flow, key), with the same random stream of
calls, window advances and rehashes.  After every rehash every live pair is found with equal stamps and counts
and no dead one remains; every sum read equals the brute-force map's; the policy never leaves more than half
the slots claimed and refuses exactly when the maximum capacity cannot hold 2 * (live + V).
ClusterParameterLeapArray's per-bucket value maps: csrv/flow/statistic/metric/ClusterParameterLeapArray.java:30-58."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pvtab_host.cpp")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("pvtab") / "pvtab_host")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-o", out, SRC], check=True,
                   capture_output=True)
    return out


# (initial capacity, maximum capacity, calls): tables that only reclaim (initial == maximum) and tables that grow
SIZES = [(16, 16, 4000), (16, 64, 4000), (64, 64, 3000), (256, 256, 2000), (64, 1024, 1500), (1024, 1024, 1200),
         (16, 4096, 600), (4096, 4096, 600)]
SAMPLE_COUNTS = [1, 2, 10, 16]


@pytest.mark.parametrize("n", SAMPLE_COUNTS, ids=lambda n: "n%d" % n)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "cap%d-max%d" % (s[0], s[1]))
def test_rehash_keeps_live_pairs_and_policy_holds(binary, size, n):
    cap, cap_max, calls = size
    r = subprocess.run([binary, str(cap), str(cap_max), str(n), str(cap * 131 + cap_max * 7 + n), str(calls)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
