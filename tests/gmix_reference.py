"""fp64 reference of the Gaussian-mixture target with diagonal precisions
(numpy): the closed form, the seeded problem generator, the a-priori bounds of
an fp32 evaluation, and an fp32 restatement of the kernel's arithmetic.  Shared
by tests/test_gmix_host.py and tests/test_gpu_gmix.py.

    p(x) = sum_k w~_k N(x; mu_k, diag(1/lam_k)),   w~ = w / sum(w)
    c_k   = log w~_k + 1/2 sum_c log lam_kc
    q_ik  = 1/2 sum_c lam_kc (x_ic - mu_kc)^2,  l_ik = c_k - q_ik,  r_ik = softmax_k(l_ik)
    S_ic  = sum_k r_ik lam_kc (mu_kc - x_ic)
    log p(x_i) = logsumexp_k l_ik - (d/2) log(2 pi)

The bounds, per entry:

    A_ic     = sum_k r_ik lam_kc (|mu_kc| + |x_ic|)            absolute-term scale
    L_ik     = |c_k| + q_ik,   delta_ik = (d + 8) 2^-24 L_ik   fp32 error of an exponent
    B_ic     = 2 sum_k r_ik expm1(delta_ik) |v_ikc - S_ic|,  v_ikc = lam_kc (mu_kc - x_ic)
    |S - S64| <= 1e-5 A + B
    |logp - logp64| <= 2 sum_k r_ik expm1(delta_ik) + 8 2^-24 (|logp64| + (d/2) log 2 pi)

1e-5 A is the project's score bound (SCORE_TOL of tests/bnn_reference.py).
delta is the a-priori error of l_ik in fp32 for any summation order of the d
products (each with three roundings, plus c_k's own and the final subtraction).
B is the first-order sensitivity of a softmax-weighted mean to errors of that
size in its exponents, with the worst-case constant 2 (numerator and
denominator); it vanishes for K = 1 and for well-separated modes.
"""
import numpy as np

SCORE_TOL = 1e-5
EPS = 2.0 ** -24
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)

# (n, K, d, spread, far): the shapes of the GPU score tests.  n = 1, K = 1 and
# d = 1; d = 2 and 3 (either side of the engine's DIRECT_MAX_D); K and d that
# are no multiple of any tile (5, 7, 65, 257); K beyond one LDS tile (257);
# d = 1024 (the limit); particles 40 away from every mode; d = 256.
SHAPES = [(1, 1, 1, 1.0, False), (33, 3, 2, 1.0, False), (37, 5, 3, 3.0, False),
          (130, 7, 65, 0.3, False), (64, 64, 257, 0.1, False), (9, 257, 64, 0.2, False),
          (5, 2, 1024, 0.05, False), (33, 5, 7, 1.0, True), (64, 16, 256, 0.05, False)]


def problem(n, K, d, spread, seed, far=False):
    """The seeded test problem (X (n, d), means (K, d), lam (K, d), w (K,)),
    all fp32: means = spread randn, lam = exp(U(-1, 1)), w = U(0.2, 1), the
    particles drawn from the mixture itself; far: every third particle moved
    by +40 in every coordinate."""
    rs = np.random.RandomState(seed)
    means = (spread * rs.randn(K, d)).astype(np.float32)
    lam = np.exp(rs.uniform(-1, 1, (K, d))).astype(np.float32)
    w = rs.uniform(0.2, 1, K).astype(np.float32)
    p = w.astype(np.float64) / w.astype(np.float64).sum()
    comp = rs.choice(K, size=n, p=p)
    X = means[comp].astype(np.float64) + rs.randn(n, d) / np.sqrt(lam[comp].astype(np.float64))
    if far:
        X[::3] += 40.0
    return X.astype(np.float32), means, lam, w


def log_weights(lam, w):
    """c_k in fp64."""
    lam, w = np.asarray(lam, np.float64), np.asarray(w, np.float64)
    return np.log(w / w.sum()) + 0.5 * np.log(lam).sum(1)


def evaluate64(X, means, lam, w):
    """The closed form and its bounds in fp64, as a dict: S (n, d), logp (n,),
    r and l (n, K), A and score_bound (n, d), logp_bound (n,), delta (n, K)."""
    X, mu, lam = (np.asarray(a, np.float64) for a in (X, means, lam))
    n, d = X.shape
    c = log_weights(lam, w)
    diff = mu[None, :, :] - X[:, None, :]                      # (n, K, d)
    v = lam[None] * diff
    q = 0.5 * (v * diff).sum(2)
    l = c[None, :] - q
    mx = l.max(1, keepdims=True)
    e = np.exp(l - mx)
    den = e.sum(1, keepdims=True)
    r = e / den
    logp = (mx + np.log(den))[:, 0] - d * HALF_LOG_2PI
    S = np.einsum("ik,ikc->ic", r, v)
    A = np.einsum("ik,ikc->ic", r, lam[None] * (np.abs(mu)[None] + np.abs(X)[:, None, :]))
    delta = (d + 8) * EPS * (np.abs(c)[None, :] + q)
    g = r * np.expm1(delta)
    B = 2.0 * np.einsum("ik,ikc->ic", g, np.abs(v - S[:, None, :]))
    logp_bound = 2.0 * g.sum(1) + 8 * EPS * (np.abs(logp) + d * HALF_LOG_2PI)
    return {"S": S, "logp": logp, "r": r, "l": l, "A": A, "score_bound": SCORE_TOL * A + B,
            "logp_bound": logp_bound, "delta": delta, "L": np.abs(c)[None, :] + q, "d": d}


def decided(ev):
    """(argmax (n,), mask (n,)): the fp64 most responsible component, and the
    particles on which fp32 must agree with it: those whose two largest
    exponents differ by more than (d + 8) 2^-24 times the larger of their two
    L.  K = 1: every particle."""
    l, L = ev["l"], ev["L"]
    arg = l.argmax(1)
    if l.shape[1] == 1:
        return arg, np.ones(len(arg), bool)
    order = np.argsort(-l, axis=1, kind="stable")[:, :2]
    rows = np.arange(len(arg))
    gap = l[rows, order[:, 0]] - l[rows, order[:, 1]]
    tol = (ev["d"] + 8) * EPS * np.maximum(L[rows, order[:, 0]], L[rows, order[:, 1]])
    return arg, gap > tol


def fp32_restatement(X, means, lam, w, pairwise=False):
    """(S, logp, comp) from a plain fp32 restatement of the kernel: the
    difference form, the d products summed sequentially (or pairwise), one pass
    over the components with a running maximum."""
    f = np.float32
    X, mu, lam = (np.asarray(a, f) for a in (X, means, lam))
    n, d = X.shape
    K = mu.shape[0]
    c = log_weights(lam, w).astype(f)
    m = np.full(n, -np.finfo(f).max, f)
    den = np.zeros(n, f)
    acc = np.zeros((n, d), f)
    best = np.full(n, -np.inf, f)
    comp = np.zeros(n, np.int32)
    for k in range(K):
        diff = mu[k][None, :] - X
        t = lam[k][None, :] * diff
        prod = t * diff
        q = prod.sum(1, dtype=f) if pairwise else np.cumsum(prod, axis=1, dtype=f)[:, -1]
        l = (c[k] - f(0.5) * q).astype(f)
        comp = np.where(l > best, np.int32(k), comp)
        best = np.maximum(best, l)
        dl = l - m
        with np.errstate(over="ignore", under="ignore"):
            ex = np.exp(-np.abs(dl)).astype(f)
        up = dl > 0
        sc, e = np.where(up, ex, f(1)), np.where(up, f(1), ex)
        m = np.where(up, l, m)
        den = (den * sc + e).astype(f)
        acc = (acc * sc[:, None] + e[:, None] * t).astype(f)
    S = acc / den[:, None]
    logp = (m + np.log(den)).astype(f) - f(HALF_LOG_2PI) * f(d)
    return S, logp.astype(f), comp


# ---- the online-softmax edge problems -----------------------------------
EDGE_N, EDGE_K, EDGE_D, EDGE_SPREAD = 16, 20, 300, 0.1
# d = 300 takes tiles of 8 components: the first, the last, and either side of
# the first tile boundary
EDGE_POSITIONS = (0, 7, 8, 19)


def edge_problem(position, seed=21):
    """A mixture whose particles are all drawn from ONE component (the
    dominant one for them), with that component moved to `position` in the
    order of the components.  Every position is the same mixture, so one fp64
    evaluation serves them all."""
    rs = np.random.RandomState(seed)
    K, d = EDGE_K, EDGE_D
    means = (EDGE_SPREAD * rs.randn(K, d)).astype(np.float32)
    lam = np.exp(rs.uniform(-1, 1, (K, d))).astype(np.float32)
    w = rs.uniform(0.2, 1, K).astype(np.float32)
    X = means[0].astype(np.float64) + rs.randn(EDGE_N, d) / np.sqrt(lam[0].astype(np.float64))
    perm = list(range(1, K))
    perm.insert(position, 0)
    perm = np.asarray(perm)
    return X.astype(np.float32), means[perm], lam[perm], w[perm]


def duplicate_problem(seed=22):
    """(split, merged): a mixture with one component present twice (the same
    mean, precisions and weight, at both ends of the order) and the same
    mixture with that component once at twice the weight; the same particles."""
    X, means, lam, w = problem(33, 6, 9, 1.0, seed)
    split = (X, np.concatenate([means, means[:1]]), np.concatenate([lam, lam[:1]]),
             np.concatenate([w, w[:1]]))
    w2 = w.copy()
    w2[0] = 2 * w[0]
    return split, (X, means, lam, w2)
