"""The preconditions of the target score kernels' suite, on the CPU: every
case of tests/score_cases.py shows in fp64 that float32 itself stays a
factor ten inside both bounds (a), that the prior does not drown the data
term (b), and that its inputs would notice a dropped data row, a dropped
weight column or a label taken for its sign by 100 x ROW_TOL (c); at most
one case in five of a group skips a mutation, and only by rule.  Also the
tables' own coverage claims, and dsvgd_logreg_small -- the one predicate
LogisticRegression.score and csrc/logreg.hip now share -- against the rule
include/dsvgd.h documents."""
import os

import numpy as np
import pytest

import score_cases as SC
from test_gpu_range import ROW_TOL

ALL = SC.all_cases()
IDS = [SC.case_id(c) for c in ALL]


def test_case_ids_are_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_preconditions(c):
    k = SC.checked(c, ROW_TOL)
    if c.p > 1:
        assert k.rows.sum() >= c.n - (1 if c.variant == "sat" else 0)
    if c.variant == "sat":
        assert k.rows[1] and np.abs(k.P.Z[1]).max() > 88 and np.abs(k.P.Z[2]).max() > 1000
    if c.variant == "wellfit":
        # (b) fails by design: that is why the case has its own measure
        ratio = k.P.a * np.sqrt((k.P.W ** 2).sum(1)) / np.sqrt((k.P.g ** 2).sum(1))
        assert np.median(ratio) > SC.PRIOR_RATIO


@pytest.mark.parametrize("group", sorted(SC.GROUPS))
def test_skip_share(group):
    cases = [c for c in SC.GROUPS[group]() if c.variant != "wellfit"]
    skipping = [c for c in cases if SC.mutations(c)[1]]
    assert len(skipping) <= SC.SKIP_CAP * len(cases), (len(skipping), len(cases))
    for c in skipping:
        assert c.p == 1 or c.N == 1


def test_tables_reach_what_they_claim():
    A = SC.cases_A()
    for c in A:
        assert SC.small_rule(c.n, c.N, c.p) == (c.path != "edge"), c
        assert (c.p <= 32) == (c.path == "reg") or c.path == "edge", c
    for vals, field in (((1, 2, 31, 32, 33, 64, 65, 255, 1023), "p"),
                        ((1, 3, 4, 5, 63, 255, 256, 257, 1025, 8192, 8193), "N"), ((1, 32, 33), "n")):
        assert set(vals) <= {getattr(c, field) for c in A}
    B = SC.cases_B()
    for e in (0, 1, 2):
        assert {c.p for c in B if c.engine == e and c.variant == "plain"} >= set(SC.B_P)
    assert all(not c.fused and not SC.small_rule(c.n, c.N, c.p) for c in B)
    C = SC.cases_C()
    assert all(SC.fused_rule(c.n, c.N, c.p) for c in C)
    assert {SC.fused_splits_rule(c.n, c.N) for c in C} == {1, 2, 4, 8}
    assert [SC.fused_splits_rule(300, N) for N in (256, 1024, 2048, 4096)] == [1, 2, 4, 8]
    n, N, p = SC.D_SHAPES[0][:3]
    assert SC.fused_rule(n, N, p) and SC.fused_splits_rule(n, N) == 4
    for axis, vals in ((0, SC.PREDICT_N), (1, SC.PREDICT_N), (2, SC.PREDICT_P)):
        seen = [s[axis] for s in SC.predict_cases()]
        assert all(seen.count(v) >= 2 for v in vals), (axis, seen)
    assert {n * d > 256 for n, d in SC.ELEMENTWISE_SHAPES} == {False, True}


def _lib():
    from dsvgd import _native
    return _native.load()


def test_small_predicate_matches_the_documented_rule():
    lib = _lib()
    for n in (1, 32, 33):
        for p in (1, 32, 33, 1023):
            for N in (1, 8192, 8193):
                assert lib.dsvgd_logreg_small(n, N, p) == int(n <= 32 and (p <= 32 or N <= 8192)), (n, N, p)


def test_targets_asks_the_library():
    """LogisticRegression.score no longer restates the rule."""
    import dsvgd.targets as T
    src = open(os.path.splitext(T.__file__)[0] + ".py").read()
    assert "dsvgd_logreg_small" in src and "8192" not in src
