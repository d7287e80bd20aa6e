"""fp64 reference of the maximum mean discrepancy between two particle sets
(numpy), the problems and the bounds shared by tests/test_mmd_host.py and
tests/test_gpu_mmd.py, and an fp32 numpy emulation of the decomposition in
csrc/mmd.hip.

Definitions (the pooled set Z = [P; Q], N = n + m, D its squared distances by
explicit differences in fp64, k = exp(-D/h) or (1 + D/h)^beta):

    rP_i = sum_{j < n, j != i} k_ij      rQ_i = sum_{j >= n, j != i} k_ij
    PP = sum_{i<n} rP_i   PQ = sum_{i<n} rQ_i   QQ = sum_{i>=n} rQ_i
    V = (PP + n)/n^2 + (QQ + m)/m^2 - 2 PQ/(n m)
    U = PP/(n(n-1)) + QQ/(m(m-1)) - 2 PQ/(n m)           (NaN if n = 1 or m = 1)
    A = (PP + n)/n^2 + (QQ + m)/m^2 + 2 PQ/(n m)         (every term positive)
    witness_i = (rP_i + [i<n])/n - (rQ_i + [i>=n])/m

The median bandwidth is the lower median of the pooled N x N matrix, diagonal
included (k = (N^2 - 1) // 2), with no 1 / log N factor; 1 if it is 0.
"""
import math

import numpy as np

MMD_TOL = 1e-5    # the project's phi / KSD bound (ksd_reference.KSD_TOL)

RBF, IMQ = 0, 1
KERNELS = {"rbf": (RBF, 0.0), "imq": (IMQ, -0.5)}

# (n, m, d): the parity shapes
SHAPES = [(1, 1, 3), (2, 3, 1), (5, 4, 2), (70, 59, 37), (200, 100, 64), (130, 254, 128),
          (128, 256, 100), (257, 256, 256), (383, 1, 128)]
# the shapes that are there for the symmetric layout
SYM_SHAPES = {(130, 254, 128), (128, 256, 100), (257, 256, 256), (383, 1, 128)}
SLICE_SHAPES = [(200, 100, 64), (130, 254, 128)]     # run with a forced slice count too
ENGINE_SHAPES = [(70, 59, 37), (130, 254, 128)]      # run on the x3 and f32 engines too
FORCED = (1, 2)


def problem(n, m, d, offcentre=False, seed=0):
    """(P, Q) fp32: standard normal draws, Q shifted by 0.3 per coordinate so
    that the statistic is not all cancellation; offcentre: 1.5 x + 3."""
    rs = np.random.RandomState(1000 * seed + 7 * n + 13 * m + d)
    P = rs.randn(n, d).astype(np.float32)
    Q = (rs.randn(m, d) + 0.3).astype(np.float32)
    if offcentre:
        P, Q = (1.5 * P + 3.0).astype(np.float32), (1.5 * Q + 3.0).astype(np.float32)
    return P, Q


_D64 = {}     # the last few problems' matrices: computed once, shared, left unchanged


def sqdist64(Z):
    """Squared distances by explicit differences in fp64 (exact zero
    diagonal); read-only, cached per input."""
    Z = np.ascontiguousarray(Z, np.float64)
    key = (Z.shape, hash(Z.tobytes()))
    if key not in _D64:
        D = np.zeros((Z.shape[0], Z.shape[0]))
        for c in range(Z.shape[1]):          # (column by column: no N x N x d array)
            diff = Z[:, c][:, None] - Z[:, c][None, :]
            D += diff * diff
        D.setflags(write=False)
        if len(_D64) >= 8:
            _D64.pop(next(iter(_D64)))
        _D64[key] = D
    return _D64[key]


def median64(D):
    """The pinned select: the lower median of all N^2 entries, diagonal included."""
    k = (D.size - 1) // 2
    return float(np.partition(D.ravel(), k)[k])


def median_h64(P, Q):
    med = median64(sqdist64(np.concatenate([P, Q], 0)))
    return med if med > 0.0 else 1.0


def fixed_h(P, Q):
    """The fixed bandwidth of the parity cases: the mean squared distance,
    rounded to fp32 (what dsvgd_set_bandwidth receives)."""
    D = sqdist64(np.concatenate([P, Q], 0))
    return float(np.float32(D.mean())) if D.mean() > 0 else 1.0


def kernel64(D, h, family, beta):
    return np.exp(-D / h) if family == RBF else (1.0 + D / h) ** beta


def finish(rP, rQ, n, m):
    """PP, PQ, QQ, V, U, A, A_u, the witness and its absolute-term sum from
    the (N,) rows (fp64)."""
    N = n + m
    first = np.arange(N) < n
    PP, PQ, QQ = float(rP[:n].sum()), float(rQ[:n].sum()), float(rQ[n:].sum())
    cross = 2.0 * PQ / (n * m)
    V = (PP + n) / n ** 2 + (QQ + m) / m ** 2 - cross
    A = (PP + n) / n ** 2 + (QQ + m) / m ** 2 + cross
    if n > 1 and m > 1:
        U = PP / (n * (n - 1)) + QQ / (m * (m - 1)) - cross
        A_u = PP / (n * (n - 1)) + QQ / (m * (m - 1)) + cross
    else:
        U = A_u = float("nan")
    wp, wq = (rP + first) / n, (rQ + ~first) / m
    return dict(PP=PP, PQ=PQ, QQ=QQ, V=V, U=U, A=A, A_u=A_u, rP=rP, rQ=rQ, witness=wp - wq,
                A_w=wp + wq, n=n, m=m)


def mmd_reference(P, Q, h=None, family=RBF, beta=0.0):
    """The fp64 closed form on the given (fp32) inputs; h=None: the median
    rule.  dict: PP, PQ, QQ, V, U, A, A_u, rP, rQ, witness, A_w, h."""
    n, m = len(P), len(Q)
    D = sqdist64(np.concatenate([P, Q], 0))
    if h is None:
        med = median64(D)
        h = med if med > 0.0 else 1.0
    K = kernel64(D, h, family, beta)
    np.fill_diagonal(K, 0.0)
    ref = finish(K[:, :n].sum(1), K[:, n:].sum(1), n, m)
    ref["h"] = h
    return ref


def check(out, rP, rQ, witness, ref, tol=MMD_TOL):
    """The bounds of the parity tests on out = [PP, PQ, QQ, V, U] and the
    rows; prints every figure before it asserts; returns the worst error /
    scale ratio."""
    out = np.asarray(out, np.float64)
    er = max(float((np.abs(rP - ref["rP"]) / (ref["rP"] + 1.0)).max()),
             float((np.abs(rQ - ref["rQ"]) / (ref["rQ"] + 1.0)).max()))
    ew = float((np.abs(witness - ref["witness"]) / ref["A_w"]).max())
    ev = abs(out[3] - ref["V"]) / ref["A"]
    nan_u = math.isnan(ref["U"])
    eu = 0.0 if nan_u else abs(out[4] - ref["U"]) / ref["A_u"]
    print("rows %.3g  witness %.3g  V %.9g ref %.9g err/A %.3g  U %.9g ref %.9g err/A_u %.3g"
          % (er, ew, out[3], ref["V"], ev, out[4], ref["U"], eu))
    assert np.isfinite(rP).all() and np.isfinite(rQ).all() and np.isfinite(witness).all()
    assert np.isfinite(out[:4]).all()
    assert er <= tol, er
    assert ew <= tol, ew
    assert ev <= tol, ev
    if nan_u:
        assert math.isnan(out[4])
    else:
        assert eu <= tol, eu
    # the class sums themselves, against their own (positive) size
    for k, name in enumerate(("PP", "PQ", "QQ")):
        assert abs(out[k] - ref[name]) <= tol * (ref[name] + 1.0), name
    return max(er, ew, ev, eu)


# ---- the fp32 emulation of csrc/mmd.hip's decomposition -------------------
def mmd_parts(N, sym, force=0):
    """dsvgd_mmd_parts."""
    T = (N + 127) // 128
    rparts = min(force, T) if force > 0 else max(1, min((2048 + T - 1) // T, T))
    return rparts + T if sym else rparts


def _kernel32(D, h, family, beta):
    f = np.float32
    inv_h = f(1.0) / f(h)
    with np.errstate(over="ignore", invalid="ignore"):
        if family == IMQ:
            u = (D * inv_h + f(1.0)).astype(f)
            return np.exp2((f(beta) * np.log2(u)).astype(f)).astype(f)
        scale = f(-inv_h * f(1.4426950408889634))
        return np.exp2((D * scale).astype(f)).astype(f)


def emulate32(P, Q, h, family=RBF, beta=0.0, sym=False, force=0):
    """The kernel's arithmetic in fp32 numpy: D in the Gram form on centred
    fp32 data (explicit differences for d <= 2, as the engine), +inf pads, the
    kernel values in fp32, one fp32 partial per row, class and slot -- column
    slices of the full layout, or the stored upper-triangle tiles of the
    symmetric layout with the transposed tiles' terms as column sums -- and
    the finish in fp64.  Returns (out[5], rP, rQ, witness)."""
    f = np.float32
    n, m = len(P), len(Q)
    Z = np.concatenate([P, Q], 0).astype(f)
    N, d = Z.shape
    n_pad = (N + 127) // 128 * 128
    T = n_pad // 128
    Zc = (Z - np.sort(Z, 0)[(N - 1) // 2]).astype(f)      # a robust centre, as pack's
    if d <= 2:
        D = np.zeros((N, N), f)
        for c in range(d):
            diff = (Zc[:, c][:, None] - Zc[:, c][None, :]).astype(f)
            D = (D + diff * diff).astype(f)
    else:
        norms = (Zc * Zc).sum(1, dtype=f)
        G = (Zc @ Zc.T).astype(f)
        D = np.maximum(norms[:, None] + norms[None, :] - f(2.0) * G, f(0.0)).astype(f)
    Dp = np.full((n_pad, n_pad), np.inf, f)
    Dp[:N, :N] = D
    K = _kernel32(Dp, h, family, beta)
    K[np.arange(n_pad), np.arange(n_pad)] = 0.0      # the diagonal, the pads: exactly 0
    K[N:, :] = 0.0
    K[:, N:] = 0.0
    parts = mmd_parts(N, sym, force)
    S = np.zeros((parts, 2, n_pad), f)
    written = np.zeros((parts, n_pad), bool)

    def split_rows(block, col0):
        """fp32 row sums of a block of columns starting at col0, per class."""
        cut = min(max(n - col0, 0), block.shape[1])
        return block[:, :cut].sum(1, dtype=f), block[:, cut:].sum(1, dtype=f)

    if not sym:
        pcols = n_pad // 16
        for z in range(parts):
            lo, hi = 16 * (pcols * z // parts), 16 * (pcols * (z + 1) // parts)
            S[z, 0], S[z, 1] = split_rows(K[:, lo:hi], lo)
            written[z] = True
    else:
        rparts = parts - T
        for I in range(T):
            rI = slice(128 * I, 128 * I + 128)
            for z in range(rparts):
                J0, J1 = I + (T - I) * z // rparts, I + (T - I) * (z + 1) // rparts
                for J in range(J0, J1):
                    rJ = slice(128 * J, 128 * J + 128)
                    tile = K[rI, rJ]
                    a, b = split_rows(tile, 128 * J)
                    S[z, 0, rI] = (S[z, 0, rI] + a).astype(f)
                    S[z, 1, rI] = (S[z, 1, rI] + b).astype(f)
                    if J != I:      # the unwritten tile (J, I): classes by the stored row
                        cut = min(max(n - 128 * I, 0), 128)
                        S[rparts + I, 0, rJ] = tile[:cut].sum(0, dtype=f)
                        S[rparts + I, 1, rJ] = tile[cut:].sum(0, dtype=f)
                        written[rparts + I, rJ] = True
                written[z, rI] = True
    rP, rQ = np.zeros(N), np.zeros(N)
    for i in range(N):
        slots = list(range(parts)) if not sym else list(range(parts - T + i // 128))
        assert written[slots, i].all()
        rP[i] = S[slots, 0, i].astype(np.float64).sum()
        rQ[i] = S[slots, 1, i].astype(np.float64).sum()
    res = finish(rP, rQ, n, m)
    out = np.array([res["PP"], res["PQ"], res["QQ"], res["V"], res["U"]])
    return out, rP.astype(f), rQ.astype(f), res["witness"].astype(f)


# ---- the problems of "it measures what it is for" --------------------------
SHIFT_CASES = [(2, 0), (16, 0), (64, 0)]        # (d, seed); n = m = 256, shift 0.5
MIXTURE_CASES = [(2, 0), (16, 0)]               # (d, seed); 512 points, modes 12 apart


def shift_problem(d, seed):
    """(A, B, B + 0.5): two independent standard normal sets and the shifted
    second one."""
    rs = np.random.RandomState(500 + 31 * d + seed)
    A = rs.randn(256, d).astype(np.float32)
    B = rs.randn(256, d).astype(np.float32)
    return A, B, (B + np.float32(0.5)).astype(np.float32)


def mixture_targets(d):
    """(exact, wrong): two unit-variance modes 12 apart with weights 0.5 / 0.5
    and 0.9 / 0.1."""
    import dsvgd
    means = np.zeros((2, d), np.float32)
    means[0, 0], means[1, 0] = -6.0, 6.0
    return (dsvgd.targets.GaussianMixture(means, 1.0, [0.5, 0.5]),
            dsvgd.targets.GaussianMixture(means, 1.0, [0.9, 0.1]))


def mixture_problem(d, seed):
    """(E1, E2, W): two independent sets of exact draws and one with the
    shares 0.9 / 0.1, 512 points each (GaussianMixture.sample)."""
    exact, wrong = mixture_targets(d)
    return (exact.sample(512, seed=3 * seed + 1).numpy(), exact.sample(512, seed=3 * seed + 2).numpy(),
            wrong.sample(512, seed=3 * seed + 3).numpy())
