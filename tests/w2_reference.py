"""The fp64 side of the W2 auction's kernel tests (test_w2_host.py proves it,
test_gpu_w2_kernels.py uses it): the case tables, seeded cost matrices that
are uploaded as they are, and the checks of include/dsvgd.h's promise "within
one fp32 ulp of max C of the optimum".  numpy and scipy only.

A case is (family, m, R): an m x n fp32 cost matrix, n = R m, slot s of the
plan belonging to row s // R.  With C64 the fp32 matrix cast to fp64,
cmax = C.max() and eps_final = max(cmax 2^-24 / n, cmax 1e-13)
(w2_start_kernel):

  cost         C64[rows, plan].sum() - opt <= n eps_final, opt from scipy's
               exact assignment on the R-times replicated rows
               (oracle.svgd_oracle.w2_plan), once per case;
  certificate  R = 1, without scipy: with the solve's fp64 prices p every row
               holds a column within eps_final + slack of its best value
               -C64 - p.  By weak duality that alone bounds the cost gap by
               n (eps_final + slack);
  decisive     the cheapest exchange of the columns of two slots of different
               rows costs at least DECISIVE x the cost bound, so a plan within
               the bound has scipy's row sets and comparing them is fair;
  gradient     dsvgd_w2_grad of a given plan, entry by entry.
"""
import functools
import itertools

import numpy as np

from oracle import svgd_oracle as O

F32 = np.float32
MAX_ROUNDS = 1 << 18
DECISIVE = 16.0
UP, DOWN = 2.0 ** 40, 2.0 ** -40

# ------------------------------------------------------------ case tables --
# n <= kTailMax = 64: the whole solve is w2_tail_kernel's
TAIL_ONLY = [(1, 1), (2, 1), (64, 1), (1, 32), (2, 32), (21, 3), (7, 9), (3, 17)]
# the first n at which the bid kernels run, one per K template / cache branch
FIRST_BID = [(65, 1), (33, 2), (13, 5), (9, 8), (8, 9), (5, 13), (5, 16), (4, 17), (3, 24),
             (3, 32)]
# block_topk's batched path needs t + 7 NT < n: 1792 at the bid kernels' 256 threads
SCAN_EDGE = [(1793, 1), (2047, 1), (2048, 1), (2049, 1), (683, 3), (64, 32), (65, 32)]
# the tail's row table is indexed i & 511: m = 513 is the first shared entry (cached, R = 2)
TAIL_TABLE = [(513, 2)]
COLD_SHAPES = TAIL_ONLY + FIRST_BID + SCAN_EDGE + TAIL_TABLE
COLD = [(f, m, R) for (m, R) in COLD_SHAPES for f in ("uniform", "svgd")]
# certificate only (no scipy run): the 512-thread tail scan's batched edge
# (3584), the first shared column entry of its c & 4095 table, every entry shared
CERT_ONLY = [("uniform", 3585, 1), ("uniform", 4097, 1), ("svgd4", 8192, 1)]

TIE_SHAPES = [(65, 1), (13, 5), (3, 32)]
TIE_FAMILIES = ["int01", "int03", "rows", "const", "zeros"]
SCALED_FAMILIES = ["up40", "down40"]

LAYOUT_SHAPES = [(13, 5), (65, 1), (2049, 1), (683, 3)]
# n % 4 == 0, so that the aligned copy takes the rows4 passes (w2_scan_first_kernel
# at R = 1, w2_violation_rows_kernel at R = 4) and the unaligned one w2_violation_kernel
LAYOUT_ROWS4_SHAPES = [(2048, 1), (17, 4)]
LAYOUTS = ["ldc5", "off1", "plain"]

WARM_SHAPES = [(65, 1), (2048, 1), (13, 5), (683, 3), (65, 32)]
WARM_STEPS = [1e-4, 0.3]
WARM = [("moved%g" % s, m, R) for (m, R) in WARM_SHAPES for s in WARM_STEPS]

KEEP_SHAPES = [(65, 1), (13, 5), (2049, 1), (65, 32)]
THETA_SHAPES = [(65, 1), (13, 5), (65, 32)]
STALL_SHAPES = [(65, 1), (13, 5)]

GRAD_SHAPES = [(1, 1, 1), (3, 32, 3), (85, 3, 3), (65, 1, 257), (5, 13, 40)]

# every case whose scipy plan a GPU test compares with
SCIPY_CASES = (COLD + WARM + [(f, m, R) for (m, R) in TIE_SHAPES
                              for f in TIE_FAMILIES + SCALED_FAMILIES]
               + [("svgd", m, R) for (m, R) in LAYOUT_ROWS4_SHAPES])
# ... and those whose row sets it compares too (test_w2_host.py: all decisive)
ROWSET_CASES = COLD + WARM + [("svgd", m, R) for (m, R) in LAYOUT_ROWS4_SHAPES]

_FAMILY_ID = {"uniform": 1, "svgd": 2, "svgd4": 3, "int01": 4, "int03": 5, "rows": 6,
              "const": 7, "zeros": 8}
# seeds are 131 m + R + 7 family + 100003 k with k = 0 unless listed here: the
# first k at which the reference alone makes the case decisive
SEED_STEP = {("svgd", 683, 3): 3, ("moved0.0001", 683, 3): 1, ("moved0.3", 683, 3): 3}


def case_id(case):
    return "%s-%dx%d" % case


def _seed(family, m, R):
    if family.startswith("first"):     # the problem that "moved<step>" moves on from
        family = "moved" + family[5:]
    base = "svgd" if family.startswith("moved") else "uniform" if family in SCALED_FAMILIES \
        else family
    return 131 * m + R + 7 * _FAMILY_ID[base] + 100003 * SEED_STEP.get((family, m, R), 0)


def sqdist32(X, P):
    """||x_i - p_j||^2 accumulated in fp32 one dimension at a time."""
    C = np.zeros((X.shape[0], P.shape[0]), F32)
    for k in range(X.shape[1]):
        df = X[:, k, None] - P[None, :, k]
        C += df * df
    return C


@functools.lru_cache(maxsize=None)
def points(family, m, R):
    """(X, P) of the svgd families: the owned rows' previous copies lead the
    columns; "moved<step>" is the next step's problem, rows and columns moved
    by step * randn, "first<step>" the problem it moves on from."""
    d = 4 if family == "svgd4" else 3
    n = m * R
    rs = np.random.RandomState(_seed(family, m, R))
    X = rs.randn(m, d).astype(F32)
    P = rs.randn(n, d).astype(F32)
    P[:m] = X - F32(1e-3) * rs.randn(m, d).astype(F32)
    if family.startswith("moved"):
        step = float(family[5:])
        X = (X + step * rs.randn(m, d)).astype(F32)
        P = (P + step * rs.randn(n, d)).astype(F32)
    return X, P


@functools.lru_cache(maxsize=None)
def cost(family, m, R):
    """The case's m x n fp32 cost matrix (read-only, shared)."""
    n = m * R
    rs = np.random.RandomState(_seed(family, m, R))
    if family == "uniform":
        C = rs.rand(m, n).astype(F32)
    elif family == "up40":
        C = cost("uniform", m, R) * F32(UP)
    elif family == "down40":
        C = cost("uniform", m, R) * F32(DOWN)
    elif family in ("svgd", "svgd4") or family[:5] in ("moved", "first"):
        C = sqdist32(*points(family, m, R))
    elif family == "int01":
        C = rs.randint(0, 2, (m, n)).astype(F32)
    elif family == "int03":
        C = rs.randint(0, 4, (m, n)).astype(F32)
    elif family == "rows":
        C = np.tile(rs.rand(n).astype(F32), (m, 1))
    elif family == "const":
        C = np.full((m, n), 0.75, F32)
    elif family == "zeros":
        C = np.zeros((m, n), F32)
    else:
        raise KeyError(family)
    C = np.ascontiguousarray(C, F32)
    C.setflags(write=False)
    return C


# ------------------------------------------------------------- the bounds --
def eps_final(C):
    cmax = float(np.max(C))
    return max(cmax * 2.0 ** -24 / C.shape[1], cmax * 1e-13)


def cost_bound(C):
    """n eps_final: cmax 2^-24 up to n = 2^-24 / 1e-13."""
    return C.shape[1] * eps_final(C)


def is_permutation(plan, n):
    plan = np.asarray(plan)
    return plan.shape == (n,) and bool(np.array_equal(np.sort(plan), np.arange(n)))


def plan_cost(C, plan):
    m, n = C.shape
    return float(C[np.arange(n) // (n // m), np.asarray(plan)].astype(np.float64).sum())


def row_sets(plan, m):
    """The plan as per-row column sets (slots of one row are interchangeable)."""
    return np.sort(np.asarray(plan).reshape(m, -1), axis=1)


@functools.lru_cache(maxsize=None)
def optimum(family, m, R):
    """(plan, cost) of scipy's exact assignment on the fp64 costs, once per case."""
    C = cost(family, m, R)
    plan = O.w2_plan(C.astype(np.float64))
    plan.setflags(write=False)
    return plan, plan_cost(C, plan)


def cost_gap_ratio(C, plan, opt):
    """(cost - opt) / (n eps_final); 0 where the bound is 0 and met exactly."""
    gap, b = plan_cost(C, plan) - opt, cost_bound(C)
    if b == 0.0:
        return 0.0 if gap <= 0.0 else np.inf
    return gap / b


def swap_gap(C, plan):
    """The smallest cost increase of exchanging the columns of two slots of
    different rows (inf if there are no two rows)."""
    m, n = C.shape
    rows = np.arange(n) // (n // m)
    M = C.astype(np.float64)[rows][:, np.asarray(plan)]   # M[s, t] = C[row(s), plan[t]]
    dg = np.diagonal(M).copy()
    D = M + M.T
    D -= dg[:, None]
    D -= dg[None, :]
    D[rows[:, None] == rows[None, :]] = np.inf
    return float(D.min())


def brute_force(C):
    """The optimal slot -> column plan's cost over all n! permutations (n <= 7)."""
    m, n = C.shape
    perms = np.array(list(itertools.permutations(range(n))))
    rows = np.arange(n) // (n // m)
    return float(C.astype(np.float64)[rows[None, :], perms].sum(1).min())


# -------------------------------------------------- the dual certificate --
def certificate(C, plan, price, chunk=512):
    """R = 1.  (worst, eps_final, slack): worst = max over rows of the best
    value -C64 - p minus the held column's, over row chunks; slack covers the
    fp64 additions of the price updates: 2^-40 (cmax + max p), and never more
    than eps_final / 16.  The plan passes if worst <= eps_final + slack."""
    m, n = C.shape
    assert m == n
    p = np.asarray(price, np.float64)
    plan = np.asarray(plan)
    worst = 0.0
    for a in range(0, m, chunk):
        V = -C[a:a + chunk].astype(np.float64) - p[None, :]
        own = V[np.arange(V.shape[0]), plan[a:a + chunk]]
        worst = max(worst, float((V.max(1) - own).max()))
    eps = eps_final(C)
    scale = float(np.max(C)) + float(np.abs(p).max())
    slack = min(2.0 ** -40 * scale, eps / 16)
    # the capped slack still has to cover a few fp64 roundings at the prices' size
    assert slack >= 2.0 ** -50 * scale, (slack, scale)
    return worst, eps, slack


def certificate_ratio(C, plan, price):
    worst, eps, slack = certificate(C, plan, price)
    assert slack <= eps / 16
    return worst / (eps + slack) if eps > 0 else (0.0 if worst <= 0 else np.inf)


def auction64(C64, theta=8.0):
    """Bertsekas' forward auction with epsilon scaling in plain fp64, one bid
    at a time (R = 1, small n): (plan, prices) at eps_final."""
    n = C64.shape[0]
    if n == 1:
        return np.zeros(1, np.int64), np.zeros(1)
    cmax = float(C64.max())
    epsf = max(cmax * 2.0 ** -24 / n, cmax * 1e-13)
    p = np.zeros(n)
    eps = max(cmax / theta, epsf)
    while True:
        owner = -np.ones(n, np.int64)
        plan = -np.ones(n, np.int64)
        free = list(range(n))
        while free:
            i = free.pop()
            v = -C64[i] - p
            j = int(np.argmax(v))
            v1 = v[j]
            v[j] = -np.inf
            p[j] += v1 - v.max() + eps
            if owner[j] >= 0:
                plan[owner[j]] = -1
                free.append(int(owner[j]))
            owner[j], plan[i] = i, j
        if eps <= epsf:
            return plan, p
        eps = max(eps / theta, epsf)


# ---------------------------------------------------------- the gradient --
GRAD_PLANS = ["random", "identity", "reversed"]


def grad_inputs(m, R, d):
    """(X, Y) fp32 of one dsvgd_w2_grad shape."""
    rs = np.random.RandomState(977 * m + 31 * R + d)
    return rs.randn(m, d).astype(F32), rs.randn(m * R, d).astype(F32)


def grad_plan(kind, n):
    """Plans made by the tests; none need be optimal."""
    if kind == "identity":
        return np.arange(n, dtype=np.int32)
    if kind == "reversed":
        return np.arange(n, dtype=np.int32)[::-1].copy()
    return np.random.RandomState(n).permutation(n).astype(np.int32)


def grad64(X, Y, plan, h):
    """(G64, A): G64[i, c] = h / n sum_r (x_ic - y_(plan[iR + r], c)) from the
    fp32 inputs in fp64, A the same sum of magnitudes."""
    X64, Y64 = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    m, n = X64.shape[0], Y64.shape[0]
    df = X64[:, None, :] - Y64[np.asarray(plan)].reshape(m, n // m, -1)
    return h / n * df.sum(1), abs(h) / n * np.abs(df).sum(1)


def grad_ratio(G, X, Y, plan, h):
    """max |G - G64| / ((R + 3) 2^-24 A): R roundings of the differences, R - 1
    of the adds, the divide and the multiply (0 / 0 counts as met)."""
    G64, A = grad64(X, Y, plan, h)
    R = Y.shape[0] // X.shape[0]
    err, tol = np.abs(np.asarray(G, np.float64) - G64), (R + 3) * 2.0 ** -24 * A
    ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max())
