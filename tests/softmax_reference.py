"""fp64 reference of the softmax-regression target (numpy): the score in
closed form with its absolute-term scale A, the minibatch-window estimate, the
predictive probabilities, an fp32 restatement chunked like the kernel, and the
shape tables.  Shared by tests/test_softmax_host.py (which pins the closed
form against fp64 autograd of SoftmaxRegression.logp) and
tests/test_gpu_softmax.py.

    x = [log alpha | vec(W)], W (C, p) row-major, d = 1 + C p, alpha = exp(x_0)
    z_qc = w_c . xd_q,  pi_qc = softmax_c(z_q.),  G_qc = 1[y_q = c] - pi_qc
    log p  = sum_q [z_{q,y_q} - logsumexp_c z_qc] + (C p / 2) x_0 - (alpha/2) |W|^2
             + a0 x_0 - b0 alpha
    d/dW_c = sum_q G_qc xd_q - alpha W_c
    d/dx_0 = C p / 2 - (alpha/2) |W|^2 + a0 - b0 alpha

The window of B rows from row `origin` (cyclic): the data sum over those rows
times N / B, the prior terms once.  A, per entry, is the sum of the absolute
values of the entry's terms:
    W rows:  A = (N/B) sum_q |G_qc| |xd_qk| + |alpha W_ck|
    x_0:     A = C p / 2 + (alpha/2) |W|^2 + a0 + b0 alpha
"""
import numpy as np

SCORE_TOL = 1e-5       # the project's score bound against absolute-term scales
SMALL_ROWS = 16        # the largest n of the row form (dsvgd_softmax_small_rows)
CHUNK = 32             # data rows per chunk of the tile form
WAVES = 4              # the waves that share a window's chunks
TILES = 16             # 32 x 32 output tiles per slab

# (n, N, C, p): the smallest shapes that reach each edge of csrc/softmax.hip.
# The kernel's constants are the issue's (row form up to n = 16, chunks of 32
# rows); a slab here is 16 tiles of (class, 32 columns), so "exactly one slab"
# is C ceil(p / 32) = 16 -- (8, 64) -- and (4, 64), (5, 52) are half slabs; the
# ragged second slab is (3, 341) (33 tiles, at n = 40 so that the tile form
# runs it) beside the issue's own shapes, all kept.
SHAPES = [
    (1, 1, 2, 1),          # the smallest shape
    (16, 33, 3, 5),        # the last n of the row form
    (17, 33, 3, 5),        # the first n of the tile form
    (33, 31, 7, 54),       # one row short of a data chunk
    (33, 32, 7, 54),       # exactly a chunk
    (33, 33, 7, 54),       # one row past
    (129, 257, 7, 54),     # more than one workgroup, ragged; more chunks than waves
    (64, 100, 4, 64),      # 8 tiles
    (40, 33, 5, 52),       # 10 tiles, ragged columns
    (33, 40, 8, 64),       # exactly one slab of 16 tiles
    (40, 150, 3, 341),     # d = 1024 in the tile form: 3 slabs, the last of one tile; 6 pieces, 2 rounds
    (5, 70, 2, 511),       # the widest rows, d = 1023 (row form)
    (9, 64, 3, 341),       # d = 1024 (row form)
    (33, 100, 16, 63),     # the most classes: two slabs
    (300, 1000, 10, 64),   # a digits-like shape
]


def dim(C, p):
    return 1 + C * p


def problem(n, N, C, p, seed, wscale=1.0, labels=None):
    """The seeded test problem (X (n, d) fp32, Xd (N, p) fp32, y (N,) int32).
    labels: None (uniform), "missing" (class 1 never occurs) or "single"
    (every label is class C - 1)."""
    rs = np.random.RandomState(seed)
    Xd = rs.randn(N, p)
    y = rs.randint(0, C, N)
    if labels == "missing":
        y[y == 1] = 0
    elif labels == "single":
        y[:] = C - 1
    X = wscale * rs.randn(n, dim(C, p)) / np.sqrt(p)
    X[:, 0] = rs.uniform(-1, 1, n)
    return X.astype(np.float32), Xd.astype(np.float32), y.astype(np.int32)


def origins(N, B):
    """The window origins worth testing: the start, the last window that does
    not wrap, the first that does, and the last row."""
    return sorted({0, N - B, (N - B + 1) % N, N - 1})


def window_rows(N, origin, B):
    return (origin + np.arange(B)) % N


def softmax64(z):
    z = z - z.max(-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(-1, keepdims=True)


def score64(X, Xd, y, C, a0=1.0, b0=1.0, origin=0, B=None):
    """(S, A): the fp64 score of every particle (n, d) over the window of B
    rows from `origin` (B=None: all the data), and the scale A of its terms."""
    X = np.asarray(X, np.float64)
    Xd, y = np.asarray(Xd, np.float64), np.asarray(y)
    n, d = X.shape
    N, p = Xd.shape
    assert d == dim(C, p)
    B = N if B is None else B
    rows = window_rows(N, origin, B)
    xw, yw = Xd[rows], y[rows]
    wt = N / B
    onehot = np.zeros((B, C))
    onehot[np.arange(B), yw] = 1.0
    S, A = np.empty((n, d)), np.empty((n, d))
    for i in range(n):
        W = X[i, 1:].reshape(C, p)
        a = np.exp(X[i, 0])
        G = onehot - softmax64(xw @ W.T)
        S[i, 1:] = (wt * (G.T @ xw) - a * W).ravel()
        A[i, 1:] = (wt * (np.abs(G).T @ np.abs(xw)) + np.abs(a * W)).ravel()
        w2 = float((W * W).sum())
        S[i, 0] = 0.5 * C * p - 0.5 * a * w2 + a0 - b0 * a
        A[i, 0] = 0.5 * C * p + 0.5 * a * w2 + a0 + b0 * a
    return S, A


def data_term64(X, Xd, y, C):
    """(n, C, p): sum_q G_qc xd_q alone, and the sum of its terms' magnitudes."""
    X = np.asarray(X, np.float64)
    Xd = np.asarray(Xd, np.float64)
    N, p = Xd.shape
    onehot = np.zeros((N, C))
    onehot[np.arange(N), np.asarray(y)] = 1.0
    T, TA = [], []
    for x in X:
        G = onehot - softmax64(Xd @ x[1:].reshape(C, p).T)
        T.append(G.T @ Xd)
        TA.append(np.abs(G).T @ np.abs(Xd))
    return np.stack(T), np.stack(TA)


def predict64(X, Xt, C):
    """(Nt, C): P[q][c] = (1/n) sum_i softmax_c(W_i xt_q)."""
    X, Xt = np.asarray(X, np.float64), np.asarray(Xt, np.float64)
    p = Xt.shape[1]
    P = np.zeros((Xt.shape[0], C))
    for x in X:
        P += softmax64(Xt @ x[1:].reshape(C, p).T)
    return P / X.shape[0]


def score32(X, Xd, y, C, a0=1.0, b0=1.0, origin=0, B=None):
    """An fp32 restatement chunked like the tile form: chunks of 32 rows, chunk
    c summed by wave c % 4 in ascending order, the waves' sums ((w0 + w1) + w2)
    + w3; every product, exponent and sum in float32."""
    f = np.float32
    X, Xd = np.asarray(X, f), np.asarray(Xd, f)
    n, d = X.shape
    N, p = Xd.shape
    B = N if B is None else B
    rows = window_rows(N, origin, B)
    wt = f(np.float64(N) / np.float64(B))
    S = np.empty((n, d), f)
    for i in range(n):
        W = X[i, 1:].reshape(C, p)
        a = np.exp(X[i, 0])
        part = np.zeros((WAVES, C, p), f)
        for c, s in enumerate(range(0, B, CHUNK)):
            r = rows[s:s + CHUNK]
            xc = Xd[r]
            z = (xc @ W.T).astype(f)
            e = np.exp((z - z.max(1, keepdims=True)).astype(f)).astype(f)
            pi = (e / e.sum(1, keepdims=True, dtype=f)).astype(f)
            G = -pi
            G[np.arange(len(r)), np.asarray(y)[r]] += f(1)
            part[c % WAVES] += (G.T @ xc).astype(f)
        acc = ((part[0] + part[1]) + part[2]) + part[3]
        S[i, 1:] = (wt * acc - a * W).ravel()
        w2 = f((W * W).sum(dtype=f))
        S[i, 0] = f(0.5) * f(C * p) - f(0.5) * a * w2 + f(a0) - f(b0) * a
    return S
