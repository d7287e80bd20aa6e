"""w2_reference.py on the CPU: the fp64 side of test_gpu_w2_kernels.py and its
inputs can tell a wrong answer from a right one.

- scipy's assignment on R-times replicated rows is the optimum (brute force
  over all permutations, n <= 7, R = 1, 2, 3, costs with and without ties);
- every case a GPU test takes scipy's plan for: that plan passes the
  permutation and cost checks with gap 0;
- every case whose row sets a GPU test compares is decisive: the cheapest
  exchange of two slots' columns costs >= 16 x the cost bound n eps_final;
- the dual certificate accepts the prices of an fp64 Bertsekas auction in
  plain numpy, rejects the plan with two columns exchanged and rejects the
  prices with one entry lowered by 4 eps_final;
- the gradient bound (R + 3) 2^-24 A holds for the kernel's order of
  operations done in numpy fp32 and not for a plan with one slot changed.
"""
import numpy as np
import pytest

import w2_reference as W

F32 = np.float32
IDS = W.case_id


@pytest.mark.parametrize("m,R", [(1, 1), (2, 1), (5, 1), (7, 1), (1, 2), (2, 2), (3, 2), (1, 3),
                                 (2, 3)])
@pytest.mark.parametrize("kind", ["uniform", "int03"])
def test_scipy_on_replicated_rows_is_brute_force(m, R, kind):
    rs = np.random.RandomState(100 * m + R)
    n = m * R
    C = (rs.rand(m, n) if kind == "uniform" else rs.randint(0, 4, (m, n))).astype(F32)
    plan = W.O.w2_plan(C.astype(np.float64))
    assert W.is_permutation(plan, n)
    best = W.brute_force(C)
    assert abs(W.plan_cost(C, plan) - best) <= 1e-12 * max(best, 1.0)


@pytest.mark.parametrize("case", W.SCIPY_CASES, ids=IDS)
def test_scipy_plan_passes_the_checks(case):
    C = W.cost(*case)
    plan, opt = W.optimum(*case)
    assert C.dtype == F32 and C.shape == (case[1], case[1] * case[2])
    assert W.is_permutation(plan, C.shape[1])
    assert W.cost_gap_ratio(C, plan, opt) == 0.0
    if case[0] in ("int01", "int03"):   # the bound is below 1: an integer cost is exactly optimal
        assert 0.0 < W.cost_bound(C) < 1.0


@pytest.mark.parametrize("case", W.ROWSET_CASES, ids=IDS)
def test_rowset_cases_are_decisive(case):
    C = W.cost(*case)
    plan, _ = W.optimum(*case)
    ratio = W.swap_gap(C, plan) / W.cost_bound(C)
    assert ratio >= W.DECISIVE, ratio


def test_swap_gap_is_the_cheapest_exchange():
    """Against the double loop it vectorises (R = 2)."""
    case = ("uniform", 4, 2)
    C = W.cost(*case)
    plan, opt = W.optimum(*case)
    best = np.inf
    for s in range(8):
        for t in range(8):
            if s // 2 != t // 2:
                q = plan.copy()
                q[s], q[t] = plan[t], plan[s]
                best = min(best, W.plan_cost(C, q) - opt)
    assert abs(W.swap_gap(C, plan) - best) < 1e-12


CERT_HOST = [c for c in W.COLD + W.WARM if c[2] == 1 and c[1] <= 65]


@pytest.mark.parametrize("case", CERT_HOST, ids=IDS)
def test_certificate_accepts_fp64_auction_and_rejects_mutations(case):
    C = W.cost(*case)
    n = C.shape[1]
    plan, price = W.auction64(C.astype(np.float64))
    assert W.is_permutation(plan, n)
    worst, eps, slack = W.certificate(C, plan, price)
    assert slack <= eps / 16
    assert worst <= eps + slack, (worst, eps, slack)
    # weak duality: the certificate alone implies the cost bound
    _, opt = W.optimum(*case)
    assert W.plan_cost(C, plan) - opt <= n * (eps + slack)
    np.testing.assert_array_equal(plan, W.optimum(*case)[0])   # decisive, R = 1
    if n == 1:
        return
    # two columns exchanged: at least half the exchange's cost shows in one row
    bad = plan.copy()
    bad[0], bad[n - 1] = plan[n - 1], plan[0]
    worst_bad = W.certificate(C, bad, price)[0]
    assert worst_bad >= W.DECISIVE / 2 * W.cost_bound(C) > eps + slack
    # the tightest (row, other column) pair: the last bidder sits eps below its
    # second best; that column 4 eps cheaper breaks eps-CS
    V = -C.astype(np.float64) - price[None, :]
    own = V[np.arange(n), plan]
    V[np.arange(n), plan] = -np.inf
    k = int(np.argmax((V - own[:, None]).max(0)))
    assert (V[:, k] - own).max() >= 0.5 * eps
    low = price.copy()
    low[k] -= 4 * eps
    worst_low = W.certificate(C, plan, low)[0]
    assert worst_low > eps + slack, (worst_low, eps)


def _grad_fp32(X, Y, plan, h):
    """w2_grad_kernel's order of operations in numpy fp32."""
    m, n = X.shape[0], Y.shape[0]
    R = n // m
    acc = np.zeros_like(X)
    for r in range(R):
        acc += X - Y[plan[r::R]]
    return F32(h) * (acc / F32(n))


@pytest.mark.parametrize("m,R,d", W.GRAD_SHAPES)
@pytest.mark.parametrize("h", [1.0, -2.5])
def test_gradient_reference(m, R, d, h):
    X, Y = W.grad_inputs(m, R, d)
    n = m * R
    for kind in W.GRAD_PLANS:
        plan = W.grad_plan(kind, n)
        assert W.is_permutation(plan, n) and plan.dtype == np.int32
        G = _grad_fp32(X, Y, plan, h)
        assert W.grad_ratio(G, X, Y, plan, h) <= 1.0
        # the project's looser 1e-5 A contains the bound for R <= 32
        assert (R + 3) * 2.0 ** -24 < 1e-5
        if m == 1:
            continue    # one row holds every column: no slot of another row to take
        wrong = plan.copy()
        wrong[0] = plan[n - 1]     # slot 0 (row 0) takes the last row's column
        assert W.grad_ratio(_grad_fp32(X, Y, wrong, h), X, Y, plan, h) > 1.0
