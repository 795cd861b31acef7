"""The model behind the cluster metrics tests (tests/cmetrics_util.py) is pinned to the oracle, without a GPU.

The oracle has no metric read, so nothing can compare the model's rows directly.  What can be compared is what the
rows are made of: on every stream test_gpu_cluster_metrics.py uses, the model re-derives from its own windows the
verdict of every non-prioritized FLOW request (nextRemaining >= 0 against the status, (int) nextRemaining against
`remaining`; ClusterFlowChecker.java:67-80) and of every PARAM request (ClusterParamFlowChecker.java:60-84; `remaining`
for single-value requests), and every derived value must equal the oracle's.  A model that counted a pass in the wrong
bucket, kept a bucket too long, or missed an occupy transfer would derive another verdict within these streams."""
import numpy as np
import pytest

import pyoracle as O
from sentinel_amd import _abi as A

import cmetrics_util as U


def _oracle():
    orc = O.Oracle(cluster_max_allowed_qps=U.BIG)
    orc.register("abc")
    return orc


@pytest.mark.parametrize("name", sorted(U.SCENARIOS))
def test_model_derives_the_oracles_verdicts(name):
    steps = U.SCENARIOS[name]()
    model, _, results = U.run(steps, _oracle())
    assert model.derived > 0
    assert not model.mismatches, (name, len(model.mismatches), model.mismatches[:3])
    st = np.concatenate([r["status"] for r in results])
    print("%s: %d verdicts derived, statuses %s" % (name, model.derived, dict(zip(*np.unique(st, return_counts=True)))))


def test_streams_decide_both_ways():
    """The streams are not ones on which everything passes: a wrong sum would change a verdict."""
    for name in ("edges-10-1000", "edges-2-500", "owners", "occupy", "reloads"):
        _, _, results = U.run(U.SCENARIOS[name](), _oracle())
        st = np.concatenate([r["status"] for r in results])
        assert (st == A.TOKEN_OK).sum() >= 0.1 * len(st) and (st == A.TOKEN_BLOCKED).sum() >= 0.1 * len(st), (name, st)
    _, _, results = U.run(U.occupy(), _oracle())
    assert any((r["status"] == A.TOKEN_SHOULD_WAIT).any() for r in results)


def test_read_rule_on_a_hand_made_window():
    """The read-back rule, bucket by bucket, on numbers small enough to check by eye."""
    m = U.FlowMetric(n=2, interval=1000, count=100.0)
    m.feed(10_000, 3, A.TOKEN_OK)        # bucket 0, start 10000
    m.feed(10_500, 2, A.TOKEN_BLOCKED)   # bucket 1, start 10500
    m.feed(10_600, 4, A.TOKEN_SHOULD_WAIT)
    assert m.read(10_999) == (3, 2)
    assert m.read(11_000) == (4, 2)      # bucket 0 reset on the copy: the occupied pass moves in
    assert m.read(11_499) == (4, 2)
    assert m.read(11_500) == (4, 0)      # bucket 1 reset on the copy too; bucket 0 (start 10000) is deprecated: 1500 > 1000
    assert m.read(9_000) == (3, 2)       # the clock before every window: taken as they are
    assert m.has_occ and m.occ_pass == 4 and m.b[0]["ws"] == 10_000  # nothing moved
    m.feed(11_000, 1, A.TOKEN_OK)        # the request that makes the transfer
    assert m.read(11_000) == (5, 2) and not m.has_occ
    p = U.ParamMetric(n=2, interval=1000, count=100.0)
    p.feed(10_010, 2, [5, 6, 5], A.TOKEN_OK)  # bucket 0, start 10000; the duplicate counts twice
    p.feed(10_700, 1, [7], A.TOKEN_OK)        # bucket 1, start 10500
    assert p.read(10_700, 5) == [(5, 4), (6, 2), (7, 1)]
    assert p.read(10_999, 1) == [(5, 4)]
    assert p.read(11_000, 5) == [(7, 1)]      # bucket 0 emptied on the copy at its start + interval
    assert p.read(11_499, 5) == [(7, 1)]
    assert p.read(11_500, 5) == [] and p.ws == [10_000, 10_500]
    p.feed(10_800, 3, [9], A.TOKEN_OK)
    p.feed(10_801, 3, [8], A.TOKEN_OK)
    assert p.read(10_900, 3) == [(5, 4), (8, 3), (9, 3)]  # 9 came first, 8 is listed first: (sum desc, key asc)
    assert p.read(10_900, 2) == [(5, 4), (8, 3)]          # the tie across the end of the list
