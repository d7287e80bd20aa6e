"""fp64 reference of the kernelized Stein discrepancy for the RBF kernel
k = exp(-|x - y|^2 / h) (numpy, the pairwise closed form
u_ij = k_ij [s_i.s_j + (2/h)(s_i - s_j).(x_i - x_j) + 2d/h - (4/h^2) D_ij]),
shared by tests/test_ksd_host.py (which pins it against second-order
autograd) and tests/test_gpu_ksd.py."""
import math

import numpy as np

KSD_TOL = 1e-5    # the project's phi bound (PHI_TOL): KSD is built from the same KY / rowsum


def sqdist64(X):
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(0)
    G = Xc @ Xc.T
    nx = np.diag(G)
    D = np.maximum(nx[:, None] + nx[None, :] - 2.0 * G, 0.0)
    np.fill_diagonal(D, 0.0)
    return D


def median_h64(X):
    """The engine's median rule in fp64: lower median of the n^2 entries of D
    (diagonal included), h = median / log n (1 if the median is 0 or n = 1)."""
    D = sqdist64(X)
    n = D.shape[0]
    k = (n * n - 1) // 2
    med = float(np.partition(D.ravel(), k)[k])
    return med / math.log(n) if (med > 0.0 and n > 1) else 1.0


def stein_matrix(X, S, h):
    """(U, Aabs): the n x n Stein kernel matrix and the matrix of the absolute
    values of its terms (the scale its rounding error is measured against)."""
    X, S = np.asarray(X, np.float64), np.asarray(S, np.float64)
    n, d = X.shape
    Xc = X - X.mean(0)
    D = sqdist64(X)
    K = np.exp(-D / h)
    SS = S @ S.T
    SX = S @ Xc.T                                   # s_i . x_j
    a = np.einsum("ij,ij->i", S, Xc)
    M = a[:, None] + a[None, :] - SX - SX.T         # (s_i - s_j) . (x_i - x_j)
    np.fill_diagonal(M, 0.0)
    U = K * (SS + (2.0 / h) * M + 2.0 * d / h - (4.0 / h ** 2) * D)
    A = K * (np.abs(SS) + (2.0 / h) * np.abs(M) + 2.0 * d / h + (4.0 / h ** 2) * D)
    return U, A


def ksd_reference(X, S, h):
    """dict: t (off-diagonal row sums), udiag, A_rows (the rows' error scale),
    off, diag, V, U and the scales A_v, A_u of V and U."""
    U, A = stein_matrix(X, S, h)
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
