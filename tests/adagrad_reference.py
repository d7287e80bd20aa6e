"""fp64 references of the AdaGrad steps and of the minibatch BayesianNN score
(numpy), shared by tests/test_adagrad_host.py and tests/test_gpu_adagrad.py.

AdaGrad (Liu & Wang's rule), per entry of the moved rows, p the whole
direction:

    G' = p^2                          where G < 0 (no history)
    G' = alpha G + (1 - alpha) p^2    elsewhere
    x' = x + step p / (eps + sqrt(G'))

The minibatch score over the cyclic window rows (c + q) mod N, q < B, with
w = N / B: the likelihood terms times w, the prior terms once.  From the
full-data closed form of tests/bnn_reference.py on the window's rows (whose
N/2 is then B/2) and the prior gradient P,

    S_mb = w S64(Z_b, y_b) - (w - 1) P,
    P = -lambda theta (weights), a0 - b0 gamma (log gamma),
        (d-2)/2 - lambda/2 |theta|^2 + a0 - b0 lambda (log lambda),

and the scale A and the ambiguity slack the same way, the likelihood part
times w.
"""
import numpy as np

import bnn_reference as R
from oracle import svgd_oracle as O


# ---------------------------------------------------------------- AdaGrad --
def update64(X, P, G, step, alpha, eps):
    """(X', G') of the rule in fp64; G < 0 marks an entry without history."""
    X, P, G = (np.asarray(a, np.float64) for a in (X, P, G))
    p2 = P * P
    Gn = np.where(G < 0.0, p2, alpha * G + (1.0 - alpha) * p2)
    return X + step * P / (eps + np.sqrt(Gn)), Gn


def jacobi64(X0, score_fn, h, T, step, alpha, eps, median=False, phi_fn=None, extra_fn=None):
    """The AdaGrad Jacobi loop: (history (T + 1, n, d), [p_t]).  score_fn(X, t)
    is iteration t's score function (a minibatch target's window moves with
    t); h a fixed bandwidth, or median=True for median(D) / log n of each
    step's particles; phi_fn(X, S, h) defaults to the oracle's RBF phi;
    extra_fn(X, t) (optional) rows added to phi before conditioning."""
    phi_fn = phi_fn or O.phi
    X = np.array(X0, np.float64)
    G = np.full(X.shape, -1.0)
    hist, dirs = [X.copy()], []
    for t in range(T):
        hh = O.median_bandwidth(X)[0] if median else h
        p = phi_fn(X, score_fn(X, t), hh)
        if extra_fn is not None:
            p = p + extra_fn(X, t)
        dirs.append(p)
        X, G = update64(X, p, G, step, alpha, eps)
        hist.append(X.copy())
    return np.stack(hist), dirs


def jacobi_fixed64(X0, score_fn, h, T, step):
    """The fixed-step Jacobi loop with a per-iteration score function."""
    X = np.array(X0, np.float64)
    hist = [X.copy()]
    for t in range(T):
        X = X + step * O.phi(X, score_fn(X, t), h)
        hist.append(X.copy())
    return np.stack(hist)


def sequential64(X0, score_fn, h, T, step):
    """The Gauss-Seidel loop (the oracle's sequential_sweep) with iteration
    t's score function fixed through sweep t: the window moves between
    sweeps, not inside one."""
    X = np.array(X0, np.float64)
    hist = [X.copy()]
    for t in range(T):
        fn = lambda x, t=t: score_fn(x, t)   # noqa: E731
        X, _, _ = O.sequential_sweep(X, fn(X), h, range(X.shape[0]), step, score_fn=fn)
        hist.append(X.copy())
    return np.stack(hist)


# -------------------------------------------------------- minibatch score --
def window(N, B, c):
    """Rows of the cyclic window that starts at c."""
    return (int(c) + np.arange(B)) % N


def prior64(X, p, H, a0=1.0, b0=0.1):
    """(P, |P| term sums): the gradient of the prior terms of log p, and the
    sum of the absolute values of each entry's prior terms."""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    assert d == R.dim(p, H)
    g, l = np.exp(X[:, -2]), np.exp(X[:, -1])
    th = X[:, :d - 2]
    th2 = (th * th).sum(1)
    P, Pa = np.empty((n, d)), np.empty((n, d))
    P[:, :d - 2] = -l[:, None] * th
    Pa[:, :d - 2] = l[:, None] * np.abs(th)
    P[:, d - 2] = a0 - b0 * g
    Pa[:, d - 2] = a0 + b0 * g
    P[:, d - 1] = 0.5 * (d - 2) - 0.5 * l * th2 + a0 - b0 * l
    Pa[:, d - 1] = 0.5 * (d - 2) + 0.5 * l * th2 + a0 + b0 * l
    return P, Pa


def minibatch_score64(X, Z, y, p, H, B, c, a0=1.0, b0=0.1):
    """(S_mb, A_mb, bound, count) of the window (c, B): the fp64 estimate,
    the scale of its terms, SCORE_TOL A_mb + the ambiguity slack (times w),
    and the number of ambiguous triples among the window's rows."""
    Z, y = np.asarray(Z), np.asarray(y)
    N = Z.shape[0]
    rows = window(N, B, c)
    w = N / B
    S, A, amb = R.score64(X, Z[rows], y[rows], p, H, a0, b0)
    P, Pa = prior64(X, p, H, a0, b0)
    S_mb = w * S - (w - 1.0) * P
    A_mb = w * A - (w - 1.0) * Pa
    slack = w * R.ambiguity_slack(X, Z[rows], amb, p, H)
    return S_mb, A_mb, R.SCORE_TOL * A_mb + slack, len(amb[0])


def minibatch_score_fn(Z, y, p, H, B, a0=1.0, b0=0.1):
    """score_fn(X, t): iteration t's estimate, window origin (t B) mod N."""
    N = np.asarray(Z).shape[0]
    return lambda X, t: minibatch_score64(X, Z, y, p, H, B, (t * B) % N, a0, b0)[0]
