"""fp64 reference of the Bayesian neural-network regression target (numpy):
the score in closed form with its absolute-term scale and the set of
pre-activations too close to 0 for fp32 to sign, the predictions, and the
seeded test problem.  Shared by tests/test_bnn_host.py (which pins the closed
form against fp64 autograd of BayesianNN.logp) and tests/test_gpu_bnn.py.

    x = [ vec(W1) (p x H row-major) | b1 (H) | w2 (H) | b2 | log g | log l ]
    f(z) = w2 . relu(W1^T z + b1) + b2,  r_q = y_q - f(z_q),  th = x[:d-2]
    log p = N/2 log g - g/2 sum r_q^2 + (d-2)/2 log l - l/2 |th|^2
            + a0 log g - b0 g + a0 log l - b0 l

With a = Z W1 + b1, m = [a > 0] (strict), G_qh = r_q w2_h m_qh:
    dW1[k][h] = g sum_q z_qk G_qh - l W1[k][h]     db1[h] = g sum_q G_qh - l b1[h]
    dw2[h]    = g sum_q relu(a_qh) r_q - l w2[h]   db2    = g sum_q r_q - l b2
    dlog g    = N/2 - g/2 sum r^2 + a0 - b0 g      dlog l = (d-2)/2 - l/2 |th|^2 + a0 - b0 l
"""
import numpy as np

AMBIGUOUS_REL = 1e-5   # |a| <= this * (|b1| + sum_k |W1_kh| |z_qk|): fp32 may flip its sign
SCORE_TOL = 1e-5       # the project's score bound against absolute-term scales


def dim(p, H):
    return H * (p + 2) + 3


def unpack(X, p, H):
    """(W1 (n, p, H), b1 (n, H), w2 (n, H), b2 (n,), log g (n,), log l (n,)) in fp64."""
    X = np.asarray(X, np.float64)
    assert X.ndim == 2 and X.shape[1] == dim(p, H)
    n = X.shape[0]
    return (X[:, :p * H].reshape(n, p, H), X[:, p * H:p * H + H], X[:, p * H + H:p * H + 2 * H],
            X[:, p * H + 2 * H], X[:, -2], X[:, -1])


def problem(n, N, p, H, seed):
    """The seeded test problem (X (n, d), Z (N, p), y (N,)), all fp32."""
    rs = np.random.RandomState(seed)
    Z = rs.randn(N, p)
    y = np.sin(Z.sum(1)) + 0.1 * rs.randn(N)
    X = rs.randn(n, dim(p, H)) / np.sqrt(p + 1)
    X[:, -2] = rs.uniform(-1, 1, n)
    X[:, -1] = rs.uniform(-1, 1, n)
    return X.astype(np.float32), Z.astype(np.float32), y.astype(np.float32)


def predict64(X, Zt, p, H):
    """(F, Fscale): F[i][q] = f_i(zt_q) and |b2| + sum_h |w2_h| (|b1_h| + sum_k
    |W1_kh| |z_qk|), the scale of its terms."""
    W1, b1, w2, b2, _, _ = unpack(X, p, H)
    Zt = np.asarray(Zt, np.float64)
    a = np.einsum("qk,ikh->iqh", Zt, W1) + b1[:, None, :]
    F = np.einsum("iqh,ih->iq", np.maximum(a, 0.0), w2) + b2[:, None]
    aabs = np.einsum("qk,ikh->iqh", np.abs(Zt), np.abs(W1)) + np.abs(b1)[:, None, :]
    return F, np.einsum("iqh,ih->iq", aabs, np.abs(w2)) + np.abs(b2)[:, None]


def score64(X, Z, y, p, H, a0=1.0, b0=0.1):
    """(S, A, amb): the score of every particle (n, d), the scale A of the
    absolute values of each entry's terms, and the ambiguous set as a list of
    (i, q, h) index arrays, one entry per triple."""
    W1, b1, w2, b2, lg, ll = unpack(X, p, H)
    X64 = np.asarray(X, np.float64)
    Z, y = np.asarray(Z, np.float64), np.asarray(y, np.float64)
    n, d = X64.shape
    N = Z.shape[0]
    g, l = np.exp(lg), np.exp(ll)
    aZ = np.abs(Z)
    S, A = np.empty((n, d)), np.empty((n, d))
    amb = []
    for i in range(n):   # one particle at a time: (N, H) intermediates only
        a = Z @ W1[i] + b1[i]
        m = a > 0.0
        relu = np.where(m, a, 0.0)
        r = y - (relu @ w2[i] + b2[i])
        G = r[:, None] * w2[i][None, :] * m
        th = X64[i, :d - 2]
        th2, r2 = float(th @ th), float(r @ r)
        data = np.concatenate([(Z.T @ G).ravel(), G.sum(0), relu.T @ r, [r.sum()]])
        dabs = np.concatenate([(aZ.T @ np.abs(G)).ravel(), np.abs(G).sum(0), relu.T @ np.abs(r),
                               [np.abs(r).sum()]])
        S[i, :d - 2] = g[i] * data - l[i] * th
        A[i, :d - 2] = g[i] * dabs + l[i] * np.abs(th)
        S[i, d - 2] = 0.5 * N - 0.5 * g[i] * r2 + a0 - b0 * g[i]
        A[i, d - 2] = 0.5 * N + 0.5 * g[i] * r2 + a0 + b0 * g[i]
        S[i, d - 1] = 0.5 * (d - 2) - 0.5 * l[i] * th2 + a0 - b0 * l[i]
        A[i, d - 1] = 0.5 * (d - 2) + 0.5 * l[i] * th2 + a0 + b0 * l[i]
        scale = aZ @ np.abs(W1[i]) + np.abs(b1[i])
        q, h = np.nonzero(np.abs(a) <= AMBIGUOUS_REL * scale)
        if len(q):
            amb.append((np.full(len(q), i), q, h, r[q]))
    if amb:
        ai, aq, ah, ar = (np.concatenate(c) for c in zip(*amb))
    else:
        ai = aq = ah = np.zeros(0, np.int64)
        ar = np.zeros(0)
    return S, A, (ai.astype(np.int64), aq.astype(np.int64), ah.astype(np.int64), ar)


def ambiguity_slack(X, Z, amb, p, H):
    """(n, d): per entry, gamma_i times the sum over the particle's ambiguous
    (q, h) of that triple's term in the entry -- |z_qk r_q w2_h| for W1[k][h],
    |r_q w2_h| for b1[h]; zero elsewhere.  An fp32 pre-activation of the set
    may land on the other side of 0, and its term is then present or absent
    as a whole."""
    _, _, w2, _, lg, _ = unpack(X, p, H)
    Z = np.asarray(Z, np.float64)
    n = w2.shape[0]
    slack = np.zeros((n, dim(p, H)))
    ai, aq, ah, ar = amb
    for i, q, h, r in zip(ai, aq, ah, ar):
        t = np.exp(lg[i]) * abs(r * w2[i, h])
        slack[i, np.arange(p) * H + h] += t * np.abs(Z[q])
        slack[i, p * H + h] += t
    return slack


def score_bound(X, Z, y, p, H, a0=1.0, b0=0.1):
    """(S, A, bound, count): the fp64 score, its scale, the bound
    SCORE_TOL * A + the ambiguity slack, and the size of the ambiguous set."""
    S, A, amb = score64(X, Z, y, p, H, a0, b0)
    return S, A, SCORE_TOL * A + ambiguity_slack(X, Z, amb, p, H), len(amb[0])
