"""The parameter key dictionary on the CPU (no GPU needed): tests/pkeys_host.cpp compiles
sentinel_amd/csrc/pkeys.h with a hash of 4 to 8 bits injected, so that pure keys collide constantly, and checks
random interns, pins and sweeps against a std::map reference after every operation (injectivity, key stability,
first owner keeps the pure key, tags, the sweep's candidate and drop sets, an intern racing a sweep), then eight
threads interning overlapping values.  The second build runs the same program under the host AddressSanitizer and
UBSan where those runtimes link; it is a stand-alone program, nothing loaded into Python is sanitized."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pkeys_host.cpp")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["-O2", "-std=c++17", "--offload-arch=gfx950", "-pthread"]


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("pkeys") / "pkeys_host")
    subprocess.run([HIPCC] + FLAGS + ["-o", out, SRC], check=True, capture_output=True)
    return out


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("pkeys_san") / "pkeys_host_san")
    r = subprocess.run([HIPCC] + FLAGS + ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-o", out, SRC],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the host sanitizer runtimes do not link here: " + r.stderr[-300:])
    return out


# (hash bits, operations, values, seed): value spaces far above 2^bits, so nearly every value is stepped off its
# pure key, and small ones where values come back after being dropped
CASES = [(4, 60_000, 300, 1), (6, 120_000, 2_000, 2), (8, 120_000, 5_000, 3), (5, 60_000, 40, 4), (60, 60_000, 500, 5)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "bits%d-values%d" % (c[0], c[2]))
def test_dictionary_matches_reference(binary, case):
    r = subprocess.run([binary] + [str(x) for x in case], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "churn ok" in r.stdout and "threads ok" in r.stdout, r.stdout


def test_dictionary_under_host_sanitizers(sanitized):
    r = subprocess.run([sanitized, "6", "40000", "1000", "9"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
