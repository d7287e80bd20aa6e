"""fp64 reference of the inverse multiquadric (IMQ) kernel
k = (1 + |x - y|^2 / h)^beta = u^beta (numpy): the SVGD direction phi, a Jacobi
step, the sequential (Gauss-Seidel) sweep and the Stein kernel matrix with its
absolute-term scale A, built as tests/ksd_reference.py builds the RBF's.
Shared by tests/test_imq_host.py (which pins it against the reference-run
fixtures and second-order autograd) and tests/test_gpu_imq.py.

With F = u^beta, G' = u^(beta-1), H' = u^(beta-2), c1 = -2 beta / h and
c2 = 4 beta (beta - 1) / h^2:
  phi_i = (1/n) [ s_i + (F S)_i + c1 (rG_i xc_i - (G' Xc)_i) ]  (sums over j != i)
  u_ij  = F s_i.s_j + c1 G' [(s_i - s_j).(x_i - x_j) + d] - c2 H' D_ij
  u_ii  = |s_i|^2 + c1 d
"""
import numpy as np

from ksd_reference import median_h64, sqdist64


def _powers(D, h, beta):
    u = 1.0 + D / h
    return u ** beta, u ** (beta - 1.0), u ** (beta - 2.0)


def phi64(X, S, h, beta, rows=None):
    """phi of `rows` of the interacting set X with scores S, pair by pair as
    the reference sums it; rows=None: all rows, in the matrix form above
    (fp64: its r x - G' X cancellation costs ~1e-13)."""
    X, S = np.asarray(X, np.float64), np.asarray(S, np.float64)
    n = X.shape[0]
    c1 = -2.0 * beta / h
    if rows is None:
        Xc = X - X.mean(0)
        F, G, _ = _powers(sqdist64(X), h, beta)
        np.fill_diagonal(F, 0.0)
        np.fill_diagonal(G, 0.0)
        return (S + F @ S + c1 * (G.sum(1)[:, None] * Xc - G @ Xc)) / n
    rows = np.asarray(rows)
    out = np.empty((len(rows), X.shape[1]))
    for k, i in enumerate(rows):
        diff = X[i] - X                                  # x_i - x_j
        F, G, _ = _powers((diff ** 2).sum(1), h, beta)   # (j = i: F = 1, diff = 0)
        out[k] = (F[:, None] * S + c1 * G[:, None] * diff).sum(0) / n
    return out


def jacobi64(X0, score, h, beta, steps, eps, median=False):
    """(steps + 1, n, d): every particle moves from the frozen set; median:
    h = median(D) / log n of each step's particles (the engine's rule)."""
    X = np.asarray(X0, np.float64).copy()
    out = [X.copy()]
    for _ in range(steps):
        hh = median_h64(X) if median else h
        X = X + eps * phi64(X, score(X), hh, beta)
        out.append(X.copy())
    return np.stack(out)


def sequential64(X0, score, h, beta, steps, eps):
    """(steps + 1, n, d) in the reference's order (dsvgd/sampler.py:62-68):
    particle i moves from the current set, earlier particles already moved."""
    X = np.asarray(X0, np.float64).copy()
    out = [X.copy()]
    for _ in range(steps):
        for i in range(X.shape[0]):
            X[i] += eps * phi64(X, score(X), h, beta, rows=[i])[0]
        out.append(X.copy())
    return np.stack(out)


def stein_matrix(X, S, h, beta):
    """(U, Aabs): the n x n Stein kernel matrix and the matrix of the absolute
    values of its terms (the scale its rounding error is measured against)."""
    X, S = np.asarray(X, np.float64), np.asarray(S, np.float64)
    n, d = X.shape
    Xc = X - X.mean(0)
    D = sqdist64(X)
    F, G, H = _powers(D, h, beta)
    c1, c2 = -2.0 * beta / h, 4.0 * beta * (beta - 1.0) / h ** 2
    SS = S @ S.T
    SX = S @ Xc.T                                   # s_i . x_j
    a = np.einsum("ij,ij->i", S, Xc)
    M = a[:, None] + a[None, :] - SX - SX.T         # (s_i - s_j) . (x_i - x_j)
    np.fill_diagonal(M, 0.0)
    U = F * SS + c1 * G * (M + d) - c2 * H * D
    A = F * np.abs(SS) + c1 * G * (np.abs(M) + d) + c2 * H * D
    return U, A


def ksd_reference(X, S, h, beta):
    """dict: t (off-diagonal row sums), udiag, A_rows (the rows' error scale),
    off, diag, V, U and the scales A_v, A_u of V and U (ksd_reference.py's)."""
    U, A = stein_matrix(X, S, h, beta)
    n = U.shape[0]
    udiag = np.diag(U).copy()
    t = U.sum(1) - udiag
    A_rows = A.sum(1) - np.diag(A)
    off, diag = float(t.sum()), float(udiag.sum())
    nn1 = n * (n - 1)
    return dict(t=t, udiag=udiag, A_rows=A_rows, off=off, diag=diag,
                V=(off + diag) / n ** 2, U=off / nn1 if n > 1 else float("nan"),
                A_v=(float(A_rows.sum()) + diag) / n ** 2,
                A_u=float(A_rows.sum()) / nn1 if n > 1 else float("nan"))
