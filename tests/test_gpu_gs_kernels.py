"""The Gauss-Seidel sweep kernels of csrc/gs.hip called directly at their
edges, in one process, n <= 640 (include/dsvgd.h: "Blocked Gauss-Seidel
sweep" and "the reference's Gauss-Seidel order for 64 < d <= 1024").

A. The d <= 64 form: dsvgd_gs_block_part against the header's definition of
   Q in fp64 -- every slice over its own j range, an empty slice exactly
   zero, the sum, both sides of the fold / reduce boundary B d nsplit = 16384
   -- and dsvgd_gs_block_sweep on that call's output for score kinds 0, 1, 2
   with and without extra and phi_out.
B. dsvgd_gs_mask and dsvgd_gs_mask_cols cell by cell through the panel layout
   of gemm_tiles.hpp: exactly the contract's cells +inf, every other bit kept.
C. The wide form: dsvgd_gsw_group_corr on synthetic sums (both code paths,
   pB up to 128, the ragged second half), dsvgd_gsw_block_sweep ALONE on sums
   built in fp64 (both walks, score kinds 0 .. 3, every block size at which
   the dispatch changes), and the whole wide sweep at its smallest shapes
   with the workspace each setting names.
D. Ill-scaled particles (an outlier 2^17 bulk radii away, inside and outside
   the moved range; every coordinate offset by 1e4) through the blocked and
   the per-row sweep, row-normalised.

Every case of A - C first shows in fp64 that its inputs would notice the
error it exists for (the in-block moved-row terms dropped, the moved rows at
their old positions and scores, one moved row or one j row dropped) by at
least SENS = 100 x the tolerance of the comparison.  That holds only where
the block is a large part of n, so these cases use n close to B, a step of
1 and scores of order 1.  Every mutation is held to the phi comparison; the
position comparison (TRAJ_TOL, absolute, the coarser of the two) to the
mutation that changes phi to first order, the dropped in-block terms --
old positions and one dropped row move X by a second-order amount.

Which walk dsvgd_gsw_block_sweep ran cannot be observed from outside: the
incremental-walk cases choose B <= 64 / (columns per thread), where the
documented rule picks it, and the silent fallback when its LDS cannot be
reserved stays unverifiable.

Tolerances: PHI_TOL / TRAJ_TOL (test_gpu_parity.py), ROW_TOL
(test_gpu_range.py), 1e-5 max |S| for refreshed scores (the existing sweep
test), 1e-6 for Y and the norms of the moved rows.  PHI_TOL is max-normalised
over the fp64 reference; a j slice of dsvgd_gs_block_part over the Q it is a
summand of.  (The worst figure of the file, 8.8e-6, is Q at B = 1, d = 1: a
reference of one number, the sum of 200 terms of either sign.)
"""
import numpy as np
import pytest
import torch

from conftest import record_parity
from oracle import svgd_oracle as O
from test_gpu_parity import PHI_TOL, TRAJ_TOL
from test_gpu_range import ROW_TOL, row_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
S_TOL = 1e-5       # refreshed scores, relative to max |S|
Y_TOL = 1e-6       # the moved rows of Y and their norms
SENS = 100.0       # the sensitivity condition: mutation >= SENS x tolerance
STEP = 1.0
F32 = np.float32


def dsvgd():
    import dsvgd as m
    return m


def native():
    from dsvgd import _native as N
    return N


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def stream():
    return native().stream(torch.device(DEV))


def sync():
    torch.cuda.synchronize()


def nan_buf(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def state(h):
    """A SelectState with the fixed bandwidth h (dsvgd_set_bandwidth)."""
    N = native()
    st = dsvgd().engine.SelectState(torch.device(DEV))
    N.call("dsvgd_set_bandwidth", st.ptr, float(h), stream())
    return st


def rup(x, m):
    return -(-x // m) * m


def mx(a):
    a = np.abs(np.asarray(a, np.float64))
    return float(a.max()) if a.size else 0.0


def nerr(got, ref):
    """max |got - ref| / max |ref| (0 / 0 = 0)."""
    den, num = mx(ref), mx(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return num / den if den > 0 else num


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def padded(A, ld, rows=None, fill=NAN):
    """A (r x c) in the first columns of a (rows x ld) float32 array of `fill`."""
    A = np.asarray(A)
    out = np.full((A.shape[0] if rows is None else rows, ld), fill, F32)
    out[:A.shape[0], :A.shape[1]] = A
    return out


def bandwidth(d):
    """exp(-D / h) of the particles below spans about e^-1.5 .. e^-8."""
    return float(F32(0.45 * d + 1.5))


def particles(n, d, seed, tight=()):
    """randn particles whose per-row radius varies over 0.6 .. 1.4 (`tight`
    rows at 0.6: near the centre, so with weight to every row); scores
    -x + noise, of order 1."""
    rs = np.random.RandomState(seed)
    rad = rs.uniform(0.6, 1.4, (n, 1))
    for j in tight:
        if j < n:
            rad[j] = 0.6
    X = (rs.randn(n, d) * rad).astype(F32)
    S = (-X + 0.3 * rs.randn(n, d)).astype(F32)
    return X, S


class Sens(object):
    """The sensitivity condition: every mutation at least SENS x tol."""

    def __init__(self):
        self.ratio = float("inf")

    def need(self, change, tol, what):
        assert change >= SENS * tol, ("insensitive inputs", what, change, tol)
        self.ratio = min(self.ratio, change / tol)


# ------------------------------------------------ score kinds, in fp64 --
MU_LAM = {}


def gauss_params(d):
    if d not in MU_LAM:
        rs = np.random.RandomState(7000 + d)
        MU_LAM[d] = (0.3 * rs.randn(d).astype(F32), rs.uniform(0.5, 2.0, d).astype(F32))
    return MU_LAM[d]


def score_fn(kind, d, scale, data=None):
    """The closed-form score of dsvgd_gs_block_sweep's / gsw's score_kind."""
    if kind == 0:
        return None
    if kind == 1:
        mu, lam = gauss_params(d)
        return lambda X: scale * O.score_gaussian(X, mu, lam)
    if kind == 2:
        return lambda X: scale * O.score_gmm(X)
    xd, td = data
    return lambda X: scale * O.score_logreg(X, xd, td)


def walk_ref(X0, S0, h, r0, B, step, fn=None, extra=None, mode=None, round32=False):
    """The sweep of rows [r0, r0 + B) in explicit fp64: row i moves with
    phi_i = sum_j k(x_i, x_j)(s_j + (2/h)(x_i - x_j)) / n (+ extra_i) of the
    CURRENT particles, then its score is refreshed (fn).  Returns (X, S, phi).

    mode = a deliberate error, for the sensitivity condition: "drop" leaves
    the block's moved rows out, "jacobi" takes them at their old positions and
    scores, "last" leaves out the row moved last, "noself" the row itself.
    round32: the moved position is stored as float32, as the kernels do."""
    X, S = np.array(X0, np.float64), np.array(S0, np.float64)
    Xu, Su = (np.array(X0, np.float64), np.array(S0, np.float64)) if mode == "jacobi" else (X, S)
    n = X.shape[0]
    phi = np.zeros((B, X.shape[1]))
    for i in range(B):
        gi = r0 + i
        df = X[gi][None, :] - Xu
        k = np.exp(-(df * df).sum(1) / h)
        if mode == "drop":
            k[r0:gi] = 0.0
        elif mode == "last" and i > 0:
            k[gi - 1] = 0.0
        elif mode == "noself":
            k[gi] = 0.0
        p = (k[:, None] * (Su + (2.0 / h) * df)).sum(0) / n
        if extra is not None:
            p = p + extra[i]
        phi[i] = p
        x = X[gi] + step * p
        X[gi] = x.astype(F32) if round32 else x
        if fn is not None:
            S[gi] = fn(X[gi:gi + 1])[0]
    return X, S, phi


def walk_sensitivity(sens, X0, S0, h, r0, B, step, fn, extra, ref):
    """Asserts the sensitivity condition of a walk on these inputs."""
    Xr, _, pr = ref
    modes = ("drop", "jacobi", "last") if B >= 2 else ("noself",)
    for mode in modes:
        Xm, _, pm = walk_ref(X0, S0, h, r0, B, step, fn, extra, mode)
        sens.need(nerr(pm, pr), PHI_TOL, (mode, "phi"))
        if mode in ("drop", "noself"):
            sens.need(mx(Xm - Xr), TRAJ_TOL, (mode, "X"))


# =================================================== A. the d <= 64 form ==
GS_D = [1, 3, 4, 5, 63, 64]
GS_N = [1, 63, 64, 65, 100, 200, 257]
GS_B = [1, 2, 63, 64]
FOLD_MAX = 16384


def gs_inputs(n, d):
    # the rows the sensitivity condition turns on -- the first two of every
    # block below and the last row -- at the small radius, so that they weigh
    tight = {n - 1, 36, 37}
    for B in (1, 2):
        for r0 in part_r0s(n, B):
            tight.update((r0, r0 + 1))
    return particles(n, d, 100 * n + d + 1000, tight=sorted(t for t in tight if 0 <= t < n))


_kmat = {}


def gs_kmat(n, d):
    """(X, S, h, K) with K = exp(-D / h) of explicit fp64 differences."""
    key = (n, d)
    if key not in _kmat:
        X, S = gs_inputs(n, d)
        h = bandwidth(d)
        K = np.exp(-O.sqdist(X, X, self_cols=np.arange(n)) / h)
        _kmat[key] = (X, S, h, K)
    return _kmat[key]


def part_ref(case, r0, B, lo, hi, unmask=False, skip=None):
    """The header's Q in fp64 over j in [lo, hi): Q[i] = sum over j outside
    [r0, r0 + i) of k(x_i, x_j)(s_j + (2/h)(x_i - x_j)), i < B.  unmask: the
    earlier rows counted all the same; skip: one j left out."""
    X, S, h, K = case
    X, S = X.astype(np.float64), S.astype(np.float64)
    cols = np.arange(lo, hi)
    Kb = K[r0:r0 + B][:, cols].copy()
    if not unmask:
        Kb[(cols[None, :] >= r0) & (cols[None, :] < r0 + np.arange(B)[:, None])] = 0.0
    if skip is not None:
        Kb[:, cols == skip] = 0.0
    return Kb @ S[cols] + (2.0 / h) * (Kb.sum(1)[:, None] * X[r0:r0 + B] - Kb @ X[cols])


def part_sensitivity(sens, case, n, r0, B):
    Q = part_ref(case, r0, B, 0, n)
    if B >= 2:
        sens.need(nerr(part_ref(case, r0, B, 0, n, unmask=True), Q), PHI_TOL, "unmasked")
    sens.need(nerr(part_ref(case, r0, B, 0, n, skip=n - 1), Q), PHI_TOL, "last j dropped")
    return Q


def part_nsplits(n):
    s = {int(native().load().dsvgd_gs_splits(n)), 1, 4, 5}
    if n == 100:
        s.add(8)      # j slices of 64 rows: six of the eight are empty
    return sorted(s)


def part_r0s(n, B):
    return sorted({0, (n - B) // 2, n - B})


def run_part(Xg, Sg, n, d, r0, B, st, ns):
    N = native()
    part = nan_buf(ns * B * d + 64)
    N.call("dsvgd_gs_block_part", N.ptr(Xg), Xg.shape[1], N.ptr(Sg), Sg.shape[1], n, d, r0, B,
           st.ptr, N.ptr(part), ns, stream())
    return part


def check_part(part, case, n, d, r0, B, ns, Q):
    """The slices over their own j ranges, an empty one exactly zero, and Q,
    all max-normalised over Q; returns the worst error."""
    P = host(part)
    assert np.isnan(P[ns * B * d:]).all()
    P = P[:ns * B * d].reshape(ns, B, d)
    assert not np.isnan(P).any()
    reduced = ns > 1 and B * d * ns > FOLD_MAX
    J = rup(-(-n // ns), 64)
    worst = 0.0
    for z in range(ns):
        lo, hi = z * J, min(n, (z + 1) * J)
        if hi <= lo:
            assert (P[z] == 0).all(), ("empty slice", z)
            continue
        if reduced and z == 0:
            continue          # overwritten with Q
        # (relative to Q, which the slice is a summand of: a slice of a 1 x 1
        # block may cancel to a hundredth of its terms)
        e = mx(P[z] - part_ref(case, r0, B, lo, hi)) / mx(Q)
        worst = max(worst, e)
        assert e < PHI_TOL, ("slice", z, e)
    e = nerr(P[0] if reduced else P.astype(np.float64).sum(0), Q)
    assert e < PHI_TOL, ("Q", e)
    return max(worst, e)


@pytest.mark.parametrize("d", GS_D)
def test_gs_block_part_matches_fp64(d):
    """dsvgd_gs_block_part for every n, B, r0 (0, mid-range, n - B) and nsplit
    (dsvgd_gs_splits(n), 1, 4, 5, and 8 at n = 100): B = 64, d = 64 folds at
    nsplit = 4 (B d nsplit = 16384) and runs gs_reduce_kernel at 5."""
    sens, worst, calls, seen = Sens(), 0.0, 0, set()
    for n in GS_N:
        case = gs_kmat(n, d)
        X, S, h, K = case
        if n >= 63:     # the weights that matter span two decades above 1e-4
            kk = K[~np.eye(n, dtype=bool)]
            big = kk[kk > 1e-4]
            assert big.size >= 0.5 * kk.size and big.max() / big.min() >= 100.0
        Xn, Sn = padded(X, d + 3), padded(S, d + 5)
        Xg, Sg = gpu(Xn), gpu(Sn)
        st = state(h)
        for B in [b for b in GS_B if b <= n]:
            for r0 in part_r0s(n, B):
                Q = part_sensitivity(sens, case, n, r0, B)
                for ns in part_nsplits(n):
                    part = run_part(Xg, Sg, n, d, r0, B, st, ns)
                    sync()
                    worst = max(worst, check_part(part, case, n, d, r0, B, ns, Q))
                    calls += 1
                    if ns > 1:
                        seen.add(B * d * ns > FOLD_MAX)
        assert same_bits(host(Xg), Xn) and same_bits(host(Sg), Sn)
    if d == 64:
        assert seen == {True, False}
    record_parity(worst, sens=sens.ratio, calls=calls)


# (n, B, r0, nsplit): n close to B, so that the in-block terms carry phi
SWEEP_SHAPES = [(1, 1, 0, 1), (3, 1, 1, 1), (2, 2, 0, 1), (3, 2, 1, 5), (64, 63, 1, 1),
                (64, 64, 0, 4), (65, 64, 1, 5), (100, 64, 36, 8)]
_sweep_ref = {}


def sweep_case(d, n, B, r0, kind, use_extra):
    """Inputs, the fp64 sweep and its sensitivity, shared by the cases that
    differ in nsplit and phi_out only."""
    key = (d, n, B, r0, kind, use_extra)
    if key not in _sweep_ref:
        X, S, h, _ = gs_kmat(n, d)
        scale = 1.0 if kind == 0 else 1.5
        fn = score_fn(kind, d, scale)
        S0 = S if fn is None else fn(X).astype(F32)
        extra = None
        if use_extra:
            extra = (0.05 * np.random.RandomState(n + d).randn(B, d)).astype(F32)
        ref = walk_ref(X, S0, h, r0, B, STEP, fn, extra)
        sens = Sens()
        walk_sensitivity(sens, X, S0, h, r0, B, STEP, fn, extra, ref)
        _sweep_ref[key] = (X, S0, h, scale, extra, ref, sens.ratio)
    return _sweep_ref[key]


@pytest.mark.parametrize("use_phi", [True, False], ids=["phi", "nophi"])
@pytest.mark.parametrize("use_extra", [True, False], ids=["extra", "noextra"])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["frozen", "gauss", "gmm"])
def test_gs_block_sweep_matches_fp64(kind, use_extra, use_phi):
    """dsvgd_gs_block_sweep on the output of dsvgd_gs_block_part (folded and
    reduced, with empty slices), ldx, lds, lde and ldphi above d: phi_out, the
    moved X, the refreshed S; everything else keeps its bits."""
    N = native()
    worst, worst_x, worst_s, ratio = 0.0, 0.0, 0.0, float("inf")
    for d in GS_D:
        mu, lam = gauss_params(d)
        mug, lamg = gpu(mu), gpu(lam)
        for n, B, r0, ns in SWEEP_SHAPES:
            X, S0, h, scale, extra, (Xr, Sr, pr), sr = sweep_case(d, n, B, r0, kind, use_extra)
            ratio = min(ratio, sr)
            ldx, lds, lde, ldphi = d + 3, d + 5, d + 2, d + 7
            Xn, Sn = padded(X, ldx), padded(S0, lds)
            Xg, Sg = gpu(Xn), gpu(Sn)
            st = state(h)
            part = run_part(Xg, Sg, n, d, r0, B, st, ns)
            exg = gpu(padded(extra, lde)) if use_extra else None
            phi = nan_buf(B + 2, ldphi) if use_phi else None
            N.call("dsvgd_gs_block_sweep", N.ptr(Xg), ldx, N.ptr(Sg), lds, n, d, r0, B, st.ptr,
                   STEP, N.ptr(part), ns, N.ptr(exg), lde, N.ptr(phi), ldphi, kind,
                   N.ptr(mug) if kind == 1 else None, N.ptr(lamg) if kind == 1 else None, scale,
                   stream())
            sync()
            Xo, So = host(Xg), host(Sg)
            rows = slice(r0, r0 + B)
            if use_phi:
                P = host(phi)
                assert np.isnan(P[B:]).all() and np.isnan(P[:, d:]).all()
                e = nerr(P[:B, :d], pr)
                worst = max(worst, e)
                assert e < PHI_TOL, (d, n, B, e)
            e = mx(Xo[rows, :d] - Xr[rows])
            worst_x = max(worst_x, e)
            assert e < TRAJ_TOL, (d, n, B, e)
            keep = np.ones(n, bool)
            keep[rows] = False
            assert same_bits(Xo[keep], Xn[keep]) and same_bits(Xo[:, d:], Xn[:, d:])
            if kind == 0:
                assert same_bits(So, Sn)
            else:
                e = mx(So[rows, :d] - Sr[rows]) / mx(Sr)
                worst_s = max(worst_s, e)
                assert e <= S_TOL, (d, n, B, e)
                assert same_bits(So[keep], Sn[keep]) and same_bits(So[:, d:], Sn[:, d:])
    record_parity(worst, x=worst_x, s=worst_s, sens=ratio)


def test_walk_ref_is_the_oracle_row_by_row():
    """The explicit fp64 walk above is O.phi(..., rows=[i]) row after row."""
    X, S, h, _ = gs_kmat(65, 5)
    fn = score_fn(2, 5, 1.5)
    Xr, Sr, pr = walk_ref(X, S, h, 1, 64, STEP, fn)
    Xo, So = X.astype(np.float64), S.astype(np.float64)
    for i in range(1, 65):
        p = O.phi(Xo, So, h, rows=[i])[0]
        assert np.abs(p - pr[i - 1]).max() <= 1e-12 * np.abs(pr).max()
        Xo[i] += STEP * p
        So[i] = fn(Xo[i:i + 1])[0]
    assert np.abs(Xo - Xr).max() <= 1e-12


# =============================================== B. the mask kernels ======
PANEL = 128 * 16


def panel_off(i, col, ldd):
    """gemm_tiles.hpp panel_off: 128 x 16 panels, panel rows of ldd / 16."""
    return ((i >> 7) * (ldd >> 4) + (col >> 4)) * PANEL + (i & 127) * 16 + (col & 15)


def mask_buffer(B, ldd):
    """Distinct finite values over the B rows' panel rows and a tail."""
    return (np.arange(rup(B, 128) * ldd + 4096) + 1).astype(F32)


def masked(D0, cells, ldd):
    want = D0.copy()
    if len(cells):
        i, col = np.array(cells, np.int64).T
        idx = panel_off(i, col, ldd)
        assert len(np.unique(idx)) == len(idx) and idx.max() < D0.size - 4096
        want[idx] = np.inf
    return want


@pytest.mark.parametrize("B", [1, 2, 17, 128, 129, 300])
def test_gs_mask_exact(B):
    """dsvgd_gs_mask: exactly the cells (i, r0 + j), j < i < B, are +inf --
    r0 off the 16- and 128-column grid, B into the second and third panel
    row -- and every other cell keeps its bits.  (An off-by-one in j < i
    would show: the expected set differs from both neighbours'.)"""
    N = native()
    runs = 0
    for ldd in (128, 384):
        for r0 in (0, 5, 16, 127, 250):
            if r0 + B > ldd:
                continue
            D0 = mask_buffer(B, ldd)
            cells = [(i, r0 + j) for i in range(B) for j in range(i)]
            want = masked(D0, cells, ldd)
            if B >= 2:
                assert not same_bits(want, masked(D0, [(i, r0 + j) for i in range(B)
                                                       for j in range(i + 1)], ldd))
                assert not same_bits(want, masked(D0, [(i, r0 + j) for i in range(B)
                                                       for j in range(i - 1)], ldd))
            Dg = gpu(D0)
            N.call("dsvgd_gs_mask", N.ptr(Dg), ldd, r0, B, stream())
            sync()
            assert same_bits(host(Dg), want), (ldd, r0)
            runs += 1
    assert runs >= 1
    record_parity(0.0, runs=runs)


@pytest.mark.parametrize("B", [1, 129])
def test_gs_mask_cols_exact(B):
    """dsvgd_gs_mask_cols: exactly the cells (i, c0 + j), i < B, j < nc."""
    N = native()
    runs = 0
    for ldd in (128, 384):
        for c0, nc in ((0, 1), (15, 2), (120, 16), (3, 300)):
            if c0 + nc > ldd:
                continue
            D0 = mask_buffer(B, ldd)
            want = masked(D0, [(i, c0 + j) for i in range(B) for j in range(nc)], ldd)
            assert not same_bits(want, masked(D0, [(i, c0 + j) for i in range(B)
                                                   for j in range(nc - 1)], ldd))
            Dg = gpu(D0)
            N.call("dsvgd_gs_mask_cols", N.ptr(Dg), ldd, B, c0, nc, stream())
            sync()
            assert same_bits(host(Dg), want), (ldd, c0, nc)
            runs += 1
    record_parity(0.0, runs=runs)


# ==================================================== C. the wide form ====
CORR_N, CORR_P0 = 262, 1
CORR_PB = [1, 63, 64, 65, 127, 128]


@pytest.mark.parametrize("d", [65, 255, 256, 257, 700, 1024])
def test_gsw_group_corr_matches_fp64(d):
    """dsvgd_gsw_group_corr on synthetic Q and Qr: the increments k_ij (x_j -
    c | s_j) and k_ij over j in [p0, p0 + pB) for pB = 1 .. 128, nr = 1, 3,
    130, the later rows right behind the earlier ones and two rows on; d <=
    256 on the unrolled path (halves of 64, the second ragged), above on the
    general one.  Everything outside the contract stays NaN."""
    N = native()
    n, p0 = CORR_N, CORR_P0
    # the earlier rows the sensitivity condition drops (the first, the last)
    X, S = particles(n, d, 31 * d, tight=[p0] + [p0 + pB - 1 for pB in CORR_PB])
    h = bandwidth(d)
    rs = np.random.RandomState(d)
    cen = (X.mean(0) + 0.1 * rs.randn(d)).astype(F32)
    K = np.exp(-O.sqdist_gram(X, X) / h)
    Xc = X.astype(np.float64) - cen.astype(np.float64)
    Sd = S.astype(np.float64)
    dp = rup(d, 32)
    ldq, ldx, lds = 2 * dp + 8, d + 3, d + 5
    Xg, Sg, cg = gpu(padded(X, ldx)), gpu(padded(S, lds)), gpu(cen)
    st = state(h)
    sens, worst = Sens(), 0.0
    for pB in CORR_PB:
        for gap in (0, 2):
            for nr in (1, 3, 130):
                r0 = p0 + pB + gap
                assert r0 + nr <= n
                ps = np.arange(p0, p0 + pB)

                def inc(cols):
                    Kc = K[r0:r0 + nr][:, cols]
                    return Kc @ Xc[cols], Kc @ Sd[cols], Kc.sum(1)
                dx, ds, dr = inc(ps)
                for name, cols in (("last", ps[:-1]), ("first", ps[1:])):
                    mx_, ms_, mr_ = inc(cols)
                    sens.need(nerr(mx_, dx), PHI_TOL, (name, "x"))
                    sens.need(nerr(ms_, ds), PHI_TOL, (name, "s"))
                    sens.need(nerr(mr_, dr), PHI_TOL, (name, "r"))
                Q0 = np.full((nr + 2, ldq), NAN, F32)
                Q0[:nr, :d] = mx(dx) * rs.randn(nr, d)
                Q0[:nr, dp:dp + d] = mx(ds) * rs.randn(nr, d)
                R0 = np.full(nr + 5, NAN, F32)
                R0[:nr] = mx(dr) * rs.uniform(0.5, 1.5, nr)
                Qg, Rg = gpu(Q0), gpu(R0)
                N.call("dsvgd_gsw_group_corr", N.ptr(Xg), ldx, N.ptr(Sg), lds, N.ptr(cg), n, d,
                       r0, nr, p0, pB, st.ptr, N.ptr(Qg), ldq, N.ptr(Rg), stream())
                sync()
                Q1, R1 = host(Qg), host(Rg)
                live = np.zeros(Q0.shape, bool)
                live[:nr, :d] = live[:nr, dp:dp + d] = True
                assert np.isnan(Q1[~live]).all() and np.isnan(R1[nr:]).all()
                Q064 = Q0.astype(np.float64)
                e = max(mx(Q1[:nr, :d] - (Q064[:nr, :d] + dx)) / mx(dx),
                        mx(Q1[:nr, dp:dp + d] - (Q064[:nr, dp:dp + d] + ds)) / mx(ds),
                        mx(R1[:nr] - (R0[:nr].astype(np.float64) + dr)) / mx(dr))
                worst = max(worst, e)
                assert e < PHI_TOL, (pB, gap, nr, e)
    record_parity(worst, sens=sens.ratio)


def walk_limit(d):
    """Rows up to which the incremental walk applies: 64 / columns per thread."""
    dp = rup(d, 32)
    return 64 // (1 if dp <= 256 else (2 if dp <= 512 else 4))


def logreg_data(d, nd, seed):
    """nd data rows of d - 1 features at a padded 16-byte-aligned ldxd (the
    pad finite and non-zero), labels +-1."""
    rs = np.random.RandomState(seed)
    p = d - 1
    # (the likelihood's sum over nd rows of order 1 .. 10 at every shape)
    xd = (rs.randn(nd, p) / np.sqrt(max(1, p) * max(1.0, nd / 64.0))).astype(F32)
    td = np.where(rs.rand(nd) < 0.5, -1.0, 1.0).astype(F32)
    return xd, td, padded(xd, rup(p, 4) + 4, fill=7.0)


_walk_ref = {}


def walk_case(d, B, kind, nd=0):
    """The inputs of dsvgd_gsw_block_sweep alone, built in fp64 and cast to
    float32 -- Y = [X - c | S] at ldy = dsvgd_ldy(dp), norms = |x - c|^2, and
    the wide pass's Q = [K Xc | K S], Qr = K 1 over every row but the row
    itself and the block's earlier rows -- with the fp64 sweep and its
    sensitivity.  n = B + 5, the block at r0 = 2."""
    key = (d, B, kind, nd)
    if key in _walk_ref:
        return _walk_ref[key]
    n, r0 = B + 5, 2
    X, S = particles(n, d, 17 * d + B)
    h = bandwidth(d)
    rs = np.random.RandomState(d + B)
    scale, data, xdp = (1.0 if kind == 0 else 1.5), None, None
    if kind == 3:
        # log alpha near the root of its own score, -a + p / 2 - a |w|^2 / 2,
        # whose slope there is p / 2: away from it, or at the whole scale,
        # a step of 1 multiplies a rounding error from row to row until the
        # fp64 sweep itself is no reference any more
        p = d - 1
        w2 = (X[:, 1:].astype(np.float64) ** 2).sum(1)
        X[:, 0] = (np.log(p / (2.0 + w2)) + 0.01 * rs.randn(n)).astype(F32)
        xd, td, xdp = logreg_data(d, nd, d + nd)
        data, scale = (xd, td), (2.0 if p <= 32 else 64.0 / p)
    fn = score_fn(kind, d, scale, data)
    S0 = S if fn is None else fn(X).astype(F32)
    cen = (X.mean(0) + 0.1 * rs.randn(d)).astype(F32)
    extra = (0.05 * rs.randn(B, d)).astype(F32)
    ref = walk_ref(X, S0, h, r0, B, STEP, fn, extra)
    sens = Sens()
    walk_sensitivity(sens, X, S0, h, r0, B, STEP, fn, extra, ref)
    dp = rup(d, 32)
    ldy = int(native().load().dsvgd_ldy(dp))
    X64, S64, c64 = X.astype(np.float64), S0.astype(np.float64), cen.astype(np.float64)
    Xc = X64 - c64
    Y = np.full((n + 1, ldy), NAN, F32)
    Y[:n, :dp] = 0.0
    Y[:n, :d] = Xc
    Y[:n, dp:dp + d] = S64
    norms = np.full(n + 3, NAN, F32)
    norms[:n] = (Xc * Xc).sum(1)
    Kb = np.exp(-O.sqdist_gram(X64[r0:r0 + B], X64) / h)
    cols = np.arange(n)[None, :]
    Kb[(cols >= r0) & (cols <= r0 + np.arange(B)[:, None])] = 0.0
    ldq = 2 * dp + 8
    Q = np.full((B + 1, ldq), NAN, F32)
    Q[:B, :d] = Kb @ Xc
    Q[:B, dp:dp + d] = Kb @ S64
    Qr = np.full(B + 3, NAN, F32)
    Qr[:B] = Kb.sum(1)
    out = dict(n=n, r0=r0, X=X, S=S0, h=h, cen=cen, extra=extra, ref=ref, sens=sens.ratio, dp=dp,
               ldy=ldy, Y=Y, norms=norms, Q=Q, ldq=ldq, Qr=Qr, scale=scale, data=data, xdp=xdp)
    _walk_ref[key] = out
    return out


def run_walk(c, d, B, kind, inc):
    """dsvgd_gsw_block_sweep on the case's buffers with the walk's form set
    to `inc`; checks everything the call may and may not write.  Returns the
    errors (phi, X, S) and phi's bits."""
    N = native()
    lib = N.load()
    n, r0, dp, ldy = c["n"], c["r0"], c["dp"], c["ldy"]
    ldx, lds, lde, ldphi = d + 3, d + 5, d + 2, d + 7
    Xn, Sn = padded(c["X"], ldx), padded(c["S"], lds)
    Xg, Sg, Yg, ng = gpu(Xn), gpu(Sn), gpu(c["Y"]), gpu(c["norms"])
    Qg, Rg, cg = gpu(c["Q"]), gpu(c["Qr"]), gpu(c["cen"])
    exg = gpu(padded(c["extra"], lde))
    phi = nan_buf(B + 2, ldphi)
    mu, lam = gauss_params(d)
    mug, lamg = gpu(mu), gpu(lam)
    xdg = tdg = None
    ldxd = nd = 0
    if kind == 3:
        xdg, tdg = gpu(c["xdp"]), gpu(c["data"][1])
        ldxd, nd = c["xdp"].shape[1], c["xdp"].shape[0]
    st = state(c["h"])
    prev = lib.dsvgd_gsw_set_inc(inc)
    try:
        N.call("dsvgd_gsw_block_sweep", N.ptr(Xg), ldx, N.ptr(Sg), lds, N.ptr(Yg), ldy, N.ptr(ng),
               N.ptr(cg), n, d, r0, B, st.ptr, STEP, N.ptr(Qg), c["ldq"], N.ptr(Rg), N.ptr(exg),
               lde, N.ptr(phi), ldphi, kind, N.ptr(mug) if kind == 1 else None,
               N.ptr(lamg) if kind == 1 else None, c["scale"], N.ptr(xdg), ldxd, N.ptr(tdg), nd,
               stream())
        sync()
    finally:
        lib.dsvgd_gsw_set_inc(prev)
    Xr, Sr, pr = c["ref"]
    Xo, So, Yo, no, P = host(Xg), host(Sg), host(Yg), host(ng), host(phi)
    rows = slice(r0, r0 + B)
    keep = np.ones(n, bool)
    keep[rows] = False
    assert np.isnan(P[B:]).all() and np.isnan(P[:, d:]).all()
    e_phi = nerr(P[:B, :d], pr)
    assert e_phi < PHI_TOL, ("phi", d, B, kind, inc, e_phi)
    e_x = mx(Xo[rows, :d] - Xr[rows])
    assert e_x < TRAJ_TOL, ("X", d, B, kind, inc, e_x)
    assert same_bits(Xo[keep], Xn[keep]) and same_bits(Xo[:, d:], Xn[:, d:])
    e_s = 0.0
    if kind == 0:
        assert same_bits(So, Sn)
        assert same_bits(Yo[:, dp:], c["Y"][:, dp:])
    else:
        e_s = mx(So[rows, :d] - Sr[rows]) / mx(Sr)
        assert e_s <= S_TOL, ("S", d, B, kind, inc, e_s)
        assert same_bits(So[keep], Sn[keep]) and same_bits(So[:, d:], Sn[:, d:])
    # Y and the norms of the moved rows follow the call's own X and S; the
    # rest of Y (other rows, the zeros up to dp, the columns past dp + d) and
    # of the norms keeps its bits
    Ykeep = np.ones(Yo.shape, bool)
    Ykeep[rows, :d] = False
    if kind != 0:
        Ykeep[rows, dp:dp + d] = False
    assert same_bits(np.where(Ykeep, Yo, 0), np.where(Ykeep, c["Y"], 0))
    nkeep = np.ones(no.shape, bool)
    nkeep[rows] = False
    assert same_bits(no[nkeep], c["norms"][nkeep])
    yx = Xo[rows, :d].astype(np.float64) - c["cen"].astype(np.float64)
    assert nerr(Yo[rows, :d], yx) <= Y_TOL
    assert nerr(Yo[rows, dp:dp + d], So[rows, :d]) <= Y_TOL
    assert nerr(no[rows], (Yo[rows, :dp].astype(np.float64) ** 2).sum(1)) <= Y_TOL
    return e_phi, e_x, e_s, P[:B, :d].copy()


def walk_blocks(d, kind):
    """B = 1, the incremental limit, one above it, the most the walk takes."""
    top = int(native().load().dsvgd_gsw_block_rows(d, kind))
    lim = walk_limit(d)
    return sorted({b for b in (1, lim, lim + 1, top) if b <= top})


@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=["frozen", "gauss", "gmm", "logreg"])
@pytest.mark.parametrize("d", [65, 256, 257, 512, 513, 1024])
def test_gsw_block_sweep_alone_matches_fp64(d, kind):
    """dsvgd_gsw_block_sweep without the wide pass, in both forms where the
    incremental walk applies (B <= 64 / columns per thread, score kinds 0 ..
    2) and on the four-wave walk alone elsewhere.  Kind 3: data sets of one
    row and of one row more than a batch of 4 (16 / NV) rows."""
    worst, worst_x, worst_s, ratio, differ, incs = 0.0, 0.0, 0.0, float("inf"), 0, 0
    nv = -(-(d - 1) // 256)
    for B in walk_blocks(d, kind):
        for nd in ((1, 4 * (16 // nv) + 1) if kind == 3 else (0,)):
            c = walk_case(d, B, kind, nd)
            ratio = min(ratio, c["sens"])
            forms = (1, 0) if (kind != 3 and B <= walk_limit(d)) else (0,)
            bits = []
            for inc in forms:
                e, ex, es, P = run_walk(c, d, B, kind, inc)
                worst, worst_x, worst_s = max(worst, e), max(worst_x, ex), max(worst_s, es)
                bits.append(P)
            if len(bits) == 2:
                incs += 1
                differ += int(not same_bits(bits[0], bits[1]))
    record_parity(worst, x=worst_x, s=worst_s, sens=ratio, inc_cases=incs, forms_differ=differ)


@pytest.mark.parametrize("d", [2, 5, 33, 64])
def test_gsw_logreg_walk_small_d(d):
    """The logistic-regression walk at d <= 64 (the wide sweep takes it at any
    d), B = 1 and 64, nd = 1, 63, 65 (one more than a batch of 64) and 1025
    data rows."""
    worst, worst_x, worst_s, ratio = 0.0, 0.0, 0.0, float("inf")
    assert int(native().load().dsvgd_gsw_block_rows(d, 3)) == 64
    for B in (1, 64):
        for nd in (1, 63, 65, 1025):
            c = walk_case(d, B, 3, nd)
            ratio = min(ratio, c["sens"])
            e, ex, es, _ = run_walk(c, d, B, 3, 0)
            worst, worst_x, worst_s = max(worst, e), max(worst_x, ex), max(worst_s, es)
    record_parity(worst, x=worst_x, s=worst_s, sens=ratio)


# (id, n, d, lo, hi, Gaussian target?, settings, (gram_h2, phi_x3, G, splits))
WIDE = [
    ("ragged_block", 65, 65, 0, 65, True, {}, (False, True, 2, 1)),
    ("n130", 130, 65, 1, 129, True, {}, (False, True, 2, 2)),
    ("pipelined", 300, 256, 7, 295, False, {}, (True, True, 2, 2)),
    ("no_pipeline", 300, 256, 7, 295, False, {"GSW_PIPELINE": False}, (True, True, 2, 2)),
    ("group1", 300, 256, 7, 295, False, {"GSW_GROUP": 1}, (True, True, 1, 2)),
    ("group4", 300, 256, 7, 295, False, {"GSW_GROUP": 4}, (True, True, 4, 2)),
    ("f32", 300, 256, 7, 295, False, {"GSW_GEMM": "f32"}, (False, False, 2, 2)),
]
_wide_ref = {}


def wide_ref(n, d, lo, hi, gauss):
    key = (n, d, lo, hi, gauss)
    if key not in _wide_ref:
        X, S = particles(n, d, 5 * n + d)
        h = bandwidth(d)
        fn = score_fn(1, d, 1.0) if gauss else None
        S0 = fn(X).astype(F32) if gauss else S
        # (a block is a fifth of n = 300: a longer step for the same effect)
        step = STEP if n < 300 else 2.0
        ref = O.sequential_sweep(X, S0, h, range(lo, hi), step, fn)
        sens = Sens()
        sens.need(nerr(O.phi(X, S0, h)[lo:hi], ref[2]), PHI_TOL, "jacobi phi")
        # every 64-row block without its own moved rows' terms
        Xm, Sm, pm = X, S0, []
        for b0 in range(lo, hi, 64):
            Xm, Sm, p = walk_ref(Xm, Sm, h, b0, min(64, hi - b0), step, fn, mode="drop")
            pm.append(p)
        sens.need(nerr(np.concatenate(pm), ref[2]), PHI_TOL, "drop phi")
        sens.need(mx(Xm - ref[0]), TRAJ_TOL, "drop X")
        _wide_ref[key] = (X, S0, h, step, ref, sens.ratio)
    return _wide_ref[key]


@pytest.mark.parametrize("case", WIDE, ids=[c[0] for c in WIDE])
def test_wide_sweep_smallest_shapes(case, monkeypatch):
    """engine.sequential_sweep(blocked=True) at 64 < d: one ragged block, two
    blocks, and three groups (the last ragged) pipelined, block after block,
    one and four blocks per pass and on the f32 engines -- each against the
    fp64 sweep, beside the per-row path, on the workspace its settings name."""
    name, n, d, lo, hi, gauss, settings, want = case
    E = dsvgd().engine
    monkeypatch.setattr(E, "GS_BLOCK_MIN_ROWS", 1)
    for k, v in settings.items():
        monkeypatch.setattr(E, k, v)
    X, S0, h, step, (Xr, Sr, pr), ratio = wide_ref(n, d, lo, hi, gauss)
    mu, lam = gauss_params(d)
    tgt = dsvgd().targets.Gaussian(mu, lam) if gauss else None
    st = state(h)
    errs = {}
    for blocked in (True, False):
        Xg, Sg = gpu(X), gpu(S0)
        phi = nan_buf(hi - lo, d)
        E.sequential_sweep(Xg, Sg, range(lo, hi), st, step, target=tgt, phi_out=phi,
                           blocked=blocked)
        sync()
        if blocked:
            W = E._WIDE_LAST[0]
            assert (W.n, W.d) == (n, d)
            assert (W.gram_h2, W.phi_x3, W.G, W.splits) == want
            assert W.B == 64 and W.n_pad == rup(n, 128)
        Xo, So = host(Xg), host(Sg)
        e, ex = nerr(host(phi), pr), mx(Xo[lo:hi] - Xr[lo:hi])
        errs[blocked] = (e, ex)
        assert e < PHI_TOL, (blocked, e)
        assert ex < TRAJ_TOL, (blocked, ex)
        assert same_bits(Xo[:lo], X[:lo]) and same_bits(Xo[hi:], X[hi:])
        if gauss:
            assert mx(So[lo:hi] - Sr[lo:hi]) <= S_TOL * mx(Sr)
            assert same_bits(So[:lo], S0[:lo]) and same_bits(So[hi:], S0[hi:])
        else:
            assert same_bits(So, S0)
    record_parity(errs[True][0], x=errs[True][1], per_row=errs[False][0], sens=ratio)


# =================================== D. ill-scaled particles in the sweeps ==
def ill_scaled(d, kind):
    """0.3 randn particles with the Gaussian target's scores -x / 0.09, frozen
    for the sweep; (X, S, moved rows)."""
    n = 384
    rs = np.random.RandomState(900 + d)
    X = (0.3 * rs.randn(n, d)).astype(F32)
    off = np.zeros(d, F32)
    lo, hi = 0, n
    if kind == "outlier_moved":
        X[300, 0] += F32(2.0 ** 17 * 0.3)
    elif kind == "outlier_fixed":
        X[300, 0] += F32(2.0 ** 17 * 0.3)
        hi = 200
    else:
        off[:] = 1e4
        X = (X + off).astype(F32)
    S = (-(X.astype(np.float64) - off) / 0.09).astype(F32)
    return X, S, lo, hi


@pytest.mark.parametrize("kind", ["outlier_moved", "outlier_fixed", "offset"])
@pytest.mark.parametrize("d", [64, 256])
def test_sweeps_row_normalised_with_ill_scaled_particles(d, kind):
    """n = 384 on the d <= 64 form and on the wide one (FmtH2 Gram with
    per-row scales, phi_mm on unscaled FmtX3): every row of phi_out within
    ROW_TOL of fp64, row-normalised, for the blocked sweep and for the per-row
    path (explicit differences: the yardstick) on the same input.  The fp64
    sweep stores each moved position as float32, as both paths do (at an
    offset of 1e4 that rounding is 5e-4 of a coordinate)."""
    E = dsvgd().engine
    X, S, lo, hi = ill_scaled(d, kind)
    h = float(F32(0.06 * d))
    step = 0.05
    _, _, ref = walk_ref(X, S, h, lo, hi - lo, step, round32=True)
    st = state(h)
    errs = {}
    for blocked in (False, True):
        Xg, Sg = gpu(X), gpu(S)
        phi = nan_buf(hi - lo, d)
        E.sequential_sweep(Xg, Sg, range(lo, hi), st, step, phi_out=phi, blocked=blocked)
        sync()
        errs[blocked] = row_err(host(phi), ref)
        assert same_bits(host(Xg)[hi:], X[hi:])
    if d > 64:
        W = E._WIDE_LAST[0]
        assert (W.n, W.d, W.gram_h2, W.phi_x3) == (384, d, True, True)
    record_parity(float(errs[True].max()), per_row=float(errs[False].max()),
                  row=int(errs[True].argmax()))
    assert errs[False].max() <= ROW_TOL, ("per-row", errs[False].max(), int(errs[False].argmax()))
    assert errs[True].max() <= ROW_TOL, ("blocked", errs[True].max(), int(errs[True].argmax()))
