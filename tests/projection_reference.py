"""fp64 reference of projected SVGD (numpy), shared by
tests/test_projection_host.py and tests/test_gpu_projection.py.

Per Jacobi iteration, with particles X (n, d), scores S and a basis Psi (d, r):

  refresh   G = S + X (add_x) or S, H = G^T G / n, Psi = the r leading
            eigenvectors of H (eigenvalues descending), each signed so that
            its largest-magnitude entry is positive
  project   Xr = X Psi, Sr = S Psi
  step      phi_r = phi of (Xr, Sr) at the bandwidth h (fixed, or the engine's
            median rule on the projected particles)
  lift      X += eps phi_r Psi^T

phi is the RBF's (K = exp(-D / h), below) or the IMQ's (imq_reference.phi64),
on the distances of ksd_reference.sqdist64.
"""
import numpy as np

import imq_reference as IMQ
from ksd_reference import median_h64, sqdist64


def gram64(X, S, add_x):
    """(H, A): H = G^T G / n and the absolute-term scale A_kl = (1/n) sum_i
    |g_ik g_il| its rounding error is measured against."""
    G = np.asarray(S, np.float64)
    if add_x:
        G = G + np.asarray(X, np.float64)
    n = G.shape[0]
    return G.T @ G / n, np.abs(G).T @ np.abs(G) / n


def basis64(H, r):
    """(Psi (d, r), lam (d,) descending) of the symmetric H."""
    lam, V = np.linalg.eigh(np.asarray(H, np.float64))
    lam, V = lam[::-1].copy(), V[:, ::-1]
    Psi = V[:, :r].copy()
    top = np.abs(Psi).argmax(0)
    sign = np.sign(Psi[top, np.arange(r)])
    sign[sign == 0] = 1.0
    return Psi * sign, lam


def rbf_phi64(X, S, h):
    """phi_i = (1/n) sum_j [K_ij s_j + (2/h) K_ij (x_i - x_j)], K = exp(-D/h)."""
    X, S = np.asarray(X, np.float64), np.asarray(S, np.float64)
    n = X.shape[0]
    Xc = X - X.mean(0)
    K = np.exp(-sqdist64(X) / h)
    return (K @ S + (2.0 / h) * (K.sum(1)[:, None] * Xc - K @ Xc)) / n


def phi64(X, S, h, beta=None):
    """The SVGD direction: RBF (beta None) or IMQ with exponent beta."""
    return rbf_phi64(X, S, h) if beta is None else IMQ.phi64(X, S, h, beta)


def direction64(X, S, Psi, h=None, beta=None):
    """(phi (n, d), h used): phi_r Psi^T; h=None: the median rule on X Psi."""
    X, S, Psi = (np.asarray(a, np.float64) for a in (X, S, Psi))
    Xr, Sr = X @ Psi, S @ Psi
    hh = median_h64(Xr) if h is None else h
    return phi64(Xr, Sr, hh, beta) @ Psi.T, hh


def step64(X, S, Psi, eps, h=None, beta=None):
    """One projected step: the moved particles (a new array)."""
    return np.asarray(X, np.float64) + eps * direction64(X, S, Psi, h, beta)[0]


def jacobi64(X0, score, basis, steps, eps, h=None, beta=None):
    """(steps + 1, n, d).  score(X, l): the scores of iteration l; basis: a
    (d, r) array, or basis(l, X, S) -> the (d, r) basis of iteration l."""
    X = np.asarray(X0, np.float64).copy()
    out = [X.copy()]
    for l in range(steps):
        S = score(X, l)
        Psi = basis(l, X, S) if callable(basis) else basis
        X = step64(X, S, Psi, eps, h, beta)
        out.append(X.copy())
    return np.stack(out)


def learned(rank, every=10, add_x=True):
    """basis(l, X, S) of jacobi64 that learns its basis as Projection(rank=
    rank, every=every) does, all in fp64."""
    hold = {}

    def basis(l, X, S):
        if (l == 0) if every is None else (l % every == 0):
            hold["Psi"] = basis64(gram64(X, S, add_x)[0], rank)[0]
        return hold["Psi"]
    return basis
