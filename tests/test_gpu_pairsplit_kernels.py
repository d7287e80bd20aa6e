"""The kernels of the pair-split layout (include/dsvgd.h, "the
pair-split layout of a DistSampler rank") called directly at their smallest
shapes, in one process, d = 256 (ldy = 512) and n <= 2048.

A. The product kernels -- dsvgd_phi_h2_window (the cyclic column window),
   dsvgd_phi_h2_transposed, _transposed_blocks and _transposed_blocks_split --
   against the fp64 product of a full-layout engine's own D and Y: every
   split-K slice over its own K range, then the sum; windows and rectangles
   off the 128 grid, wrapped, ragged, with empty slices, with ldk > ldy.  The
   output buffers start as NaN and every cell outside the contract must still
   be NaN afterwards.  Each case first shows in fp64 that its inputs would
   notice a K-step misplaced by 16 columns.
B. The exact kernels bit for bit: the two partial reductions against a numpy
   float32 restatement of their documented order, the pair-split median
   (dsvgd_radix_hist_wmap) driven in lockstep from the host without
   candidates and after a forced bracket miss, the bracket counts of
   dsvgd_sqdist_h2_parts, and the shares of dsvgd_sample_sqdist_range.
C. dsvgd_phi_finish_parts on synthetic buffers against its formula in fp64,
   and the whole layout for S = 2 .. 5 with every row of every rank against
   the fp64 oracle, the exchange done by a stub in this process.

Tolerances: KY_TOL / PHI_TOL (test_gpu_split.py), ROW_TOL (test_gpu_range.py),
1e-6 for the row sums (test_gpu_phi_wform.py) -- all max-normalised over the
reference.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import record_parity
from oracle import svgd_oracle as O
from test_gpu_range import ROW_TOL, row_err
from test_gpu_split import KY_TOL, PHI_TOL, decode_h2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIM = 256
RS_TOL = 1e-6
# bandwidth of the fixture: the squared distances of the inputs below span
# about 180 .. 1100, so k = exp(-D / h) spans about three decades above 1e-4
H_FIX = 120.0
NAN = float("nan")


def dsvgd():
    import dsvgd as m
    return m


def native():
    from dsvgd import _native as N
    return N


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def stream():
    return native().stream(torch.device(DEV))


def nan_buf(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def all_nan(t):
    return t.numel() == 0 or bool(torch.isnan(t).all())


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


def pad128(x):
    return -(-x // 128) * 128


def kchunk_of(K, splits):
    """The K range of a split-K slice: roundup(ceil(K / splits), 16)."""
    return -(-(-(-K // splits)) // 16) * 16


_data = {}


def _inputs(n):
    """randn particles whose per-row radius varies by about 2x; scores -x + noise."""
    if n not in _data:
        rs = np.random.RandomState(1000 + n)
        X = (rs.randn(n, DIM) * rs.uniform(0.6, 1.4, (n, 1))).astype(np.float32)
        _data[n] = (X, (-X + 0.3 * rs.randn(n, DIM)).astype(np.float32))
    return _data[n]


class _Full(object):
    """A full-layout h2 engine after one direction(): D (n_pad x n_pad, +inf
    pads), the FmtH2 image Yx, the column scales and the state, with the fp64
    K = exp(-D / h) of its own D and Y in fp64."""


_full = {}


def full(n):
    if n in _full:
        return _full[n]
    N = native()
    X, S = _inputs(n)
    eng = dsvgd().PhiEngine(n, DIM, device=DEV, sym_layout=False, gemm="h2")
    assert not eng.sym and eng.phi_form == "xs" and eng.ldy == 512
    eng.pack(gpu(X), gpu(S))
    eng.distances(median=False)
    eng.fixed_bandwidth(H_FIX)
    eng.direction(gpu(X).clone(), 0.0)
    torch.cuda.synchronize()
    assert eng.range_guard() is False
    F = _Full()
    F.eng, F.n, F.n_pad, F.ldy = eng, n, eng.n_pad, eng.ldy
    F.D = eng.dense_D(padded=True).double()
    assert bool(torch.isinf(F.D[n:, :]).all()) and bool(torch.isinf(F.D[:, n:]).all())
    assert bool(torch.isfinite(F.D[:n, :n]).all())
    _, F.h, _ = eng.state.read()
    F.K = torch.exp(-F.D / F.h)
    off = F.K[:n, :n][~torch.eye(n, dtype=torch.bool, device=DEV)]
    # the off-diagonal weights span at least two decades and stay above 1e-6
    assert float(off.min()) > 1e-6 and float(off.max() / off.min()) >= 100.0
    assert bool((eng.Y[n:F.n_pad] == 0).all())
    F.Y = eng.Y[:F.n_pad].double()
    # the image the products read is Y (dsvgd_h2_ysplit's two-part bound)
    Yn = F.Y.cpu().numpy()
    sc = eng.yscale.cpu().numpy().astype(np.float64)
    rec = decode_h2(eng.Yx, F.n_pad, F.ldy).sum(0) * sc[F.ldy:2 * F.ldy][None, :]
    mx = np.abs(Yn).max(0)
    assert np.all(np.abs(rec - Yn) <= 2.0 ** -22 * np.abs(Yn) + 2.0 ** -38 * mx[None, :])
    F.Dp, F.Yx = N.ptr(eng.D), N.ptr(eng.Yx)
    F.colinv = N.ptr(eng.yscale) + 4 * F.ldy
    F.st = eng.state.ptr
    _full[n] = F
    return F


def max_err(got, ref):
    """max |got - ref| / max |ref| (0 / 0 = 0)."""
    den = float(ref.abs().max())
    num = float((got - ref).abs().max())
    return num / den if den > 0 else num


def check_slices(KY, RS, ref_fn, K, splits, shifted_fn=None):
    """KY (splits, rows, ldy) and RS (splits, rows) against ref_fn(lo, hi) ->
    (product, row sums) in fp64 over the K positions [lo, hi): every slice
    over its own range (an empty one exactly zero), then the sum.  Before the
    GPU result is looked at, shifted_fn -- the same reference one K-step of 16
    columns away -- must differ from the true one by more than 100 x the
    tolerances.  Returns the worst (product, row sum) errors."""
    kc = kchunk_of(K, splits)
    P_all, r_all = ref_fn(0, K)
    if shifted_fn is not None:
        hi0 = min(K, kc)
        P0, r0 = ref_fn(0, hi0)
        Ps, rs_ = shifted_fn(0, hi0)
        assert max_err(Ps, P0) > 100 * KY_TOL, max_err(Ps, P0)
        assert max_err(rs_, r0) > 100 * RS_TOL, max_err(rs_, r0)
    worst, worst_r = 0.0, 0.0
    for z in range(splits):
        lo, hi = z * kc, min(K, (z + 1) * kc)
        if hi <= lo:
            assert bool((KY[z] == 0).all()) and bool((RS[z] == 0).all()), "empty slice %d" % z
            continue
        P, r = ref_fn(lo, hi)
        e, e_r = max_err(KY[z].double(), P), max_err(RS[z].double(), r)
        worst, worst_r = max(worst, e), max(worst_r, e_r)
        assert e < KY_TOL, ("slice", z, e)
        assert e_r < RS_TOL, ("slice", z, e_r)
    e, e_r = max_err(KY.double().sum(0), P_all), max_err(RS.double().sum(0), r_all)
    assert e < KY_TOL, ("sum", e)
    assert e_r < RS_TOL, ("sum", e_r)
    return max(worst, e), max(worst_r, e_r)


# ------------------------------------------------ A1. the cyclic window --
def window_ref(F, row0, m, col0, lo, hi, shift=0):
    """fp64 product of rows [row0, row0 + m) over the window positions
    [lo, hi) of the cyclic window that starts at column col0 (+ shift), the
    diagonal j == row0 + i left out; also the number of entries left out."""
    cols = (col0 + shift + torch.arange(lo, hi, device=DEV)) % F.n_pad
    Kw = F.K[row0:row0 + m][:, cols].clone()
    own = cols[None, :] == (row0 + torch.arange(m, device=DEV))[:, None]
    Kw[own] = 0.0
    return Kw @ F.Y[cols], Kw.sum(1), int(own.sum())


def run_window(F, row0, m, col0, wlen, splits, ldk):
    """dsvgd_phi_h2_window into NaN-filled buffers; returns (KY, rowsum) as
    (splits, m, ldy) / (splits, m) after checking that nothing else was written."""
    N = native()
    mp = pad128(m)
    KY = nan_buf(splits * m + 3, ldk)
    RS = nan_buf(splits * mp + 64)
    N.call("dsvgd_phi_h2_window", F.Dp + 4 * row0 * F.n_pad, F.n_pad, F.Yx, F.ldy, row0, m, F.n,
           col0, wlen, F.st, splits, N.ptr(KY), ldk, N.ptr(RS), F.colinv, None, 0, stream())
    torch.cuda.synchronize()
    assert all_nan(KY[splits * m:]) and all_nan(KY[:, F.ldy:])
    R = RS[:splits * mp].view(splits, mp)
    assert all_nan(R[:, m:]) and all_nan(RS[splits * mp:])
    return KY[:splits * m].view(splits, m, ldk)[:, :, :F.ldy], R[:, :m]


# (id, n, row0, m, col0, wlen, splits, rows whose own column is in the window)
WINDOWS = [
    ("whole_ring", 1000, 0, 1000, 0, 1024, (1, 4), 1000),
    ("plan_like_wrap", 1000, 768, 232, 768, 512, (1, 3), 232),
    ("grid16", 1000, 128, 128, 112, 144, (1, 2), 128),
    ("no_diagonal", 1000, 0, 128, 256, 256, (2,), 0),
    ("empty_slices", 1000, 0, 100, 0, 32, (4,), 32),
    ("diagonal_after_wrap", 1000, 0, 128, 512, 768, (1, 3), 128),
    ("straddling", 1000, 0, 256, 640, 640, (2,), 256),
    ("whole_ring_300", 300, 0, 300, 0, 384, (1, 4), 300),
    ("ragged_n", 300, 256, 44, 288, 192, (1,), 12),
]


@pytest.mark.parametrize("case", WINDOWS, ids=[c[0] for c in WINDOWS])
def test_window_matches_fp64(case):
    """dsvgd_phi_h2_window: every slice and the sum within KY_TOL / 1e-6 of
    fp64, the diagonal j == row0 + i left out wherever the window meets it --
    also behind the wrap ("diagonal_after_wrap", "straddling": rows left of
    col0, whose own column the window reaches only after wrapping; before the
    per-row wrap offset in phi_w1.hpp's diag0 these two missed by k_ii = 1 in
    the row sums and Y_i in the product)."""
    name, n, row0, m, col0, wlen, splits_list, ndiag = case
    F = full(n)
    ring = wlen == F.n_pad
    assert window_ref(F, row0, m, col0, 0, wlen)[2] == ndiag
    for splits in splits_list:
        def ref(lo, hi, shift=0):
            return window_ref(F, row0, m, col0, lo, hi, shift)[:2]
        # (the whole ring in one slice: a shifted window is the same columns)
        shifted = None if (ring and splits == 1) else (lambda lo, hi: ref(lo, hi, 16))
        KY, RS = run_window(F, row0, m, col0, wlen, splits, F.ldy if ring else F.ldy + 16)
        e, e_r = check_slices(KY, RS, ref, wlen, splits, shifted)
        record_parity(e, rowsum=e_r, case=name, splits=splits)
        if ring:   # the engine's own dsvgd_phi_mm_h2 over the same D and image
            eng = F.eng
            own = eng.KY.view(-1)[:eng.splits * n * F.ldy].view(eng.splits, n, F.ldy)
            assert max_err(KY.double().sum(0), own.double().sum(0)) < KY_TOL


def test_window_xcd_map_gives_identical_bits():
    """The whole ring in 4 slices of 8 row blocks is a grid the XCD slice map
    (dsvgd_phi_set_xmap bit 2) applies to: the same bits with and without."""
    F = full(1000)
    lib = native().load()
    out = {}
    for mask in (7, 0):
        prev = lib.dsvgd_phi_set_xmap(mask)
        try:
            out[mask] = run_window(F, 0, 1000, 0, 1024, 4, F.ldy)
        finally:
            lib.dsvgd_phi_set_xmap(prev)
    assert same_bits(out[7][0], out[0][0]) and same_bits(out[7][1], out[0][1])


# ------------------------------------------- A2. a transposed rectangle --
def transposed_ref(F, yrow0, col0, mo, lo, hi, shift=0):
    """P[i] = sum_j exp(-D[yrow0 + j, col0 + i] / h) Y[yrow0 + j] over the
    rectangle's rows j in [lo, hi) -- no diagonal rule: k_ii is included."""
    rows = yrow0 + shift + torch.arange(lo, hi, device=DEV)
    Kt = F.K[rows][:, col0:col0 + mo]
    return Kt.t() @ F.Y[rows], Kt.sum(0)


def run_transposed(F, yrow0, krows, col0, mo, splits, ldp):
    N = native()
    mp = pad128(mo)
    P = nan_buf(splits * mo + 3, ldp)
    RS = nan_buf(splits * mp + 64)
    N.call("dsvgd_phi_h2_transposed", F.Dp + 4 * yrow0 * F.n_pad, F.n_pad, F.Yx, F.ldy, yrow0,
           krows, col0, mo, F.n, F.st, splits, N.ptr(P), ldp, N.ptr(RS), F.colinv, None, 0,
           stream())
    torch.cuda.synchronize()
    assert all_nan(P[splits * mo:]) and all_nan(P[:, F.ldy:])
    R = RS[:splits * mp].view(splits, mp)
    assert all_nan(R[:, mo:]) and all_nan(RS[splits * mp:])
    return P[:splits * mo].view(splits, mo, ldp)[:, :, :F.ldy], R[:, :mo]


def check_transposed(F, yrow0, krows, col0, mo, splits, ldp):
    # one K-step further down D's rows, or up where that would leave n_pad
    sh = 16 if yrow0 + krows + 16 <= F.n_pad else -16

    def ref(lo, hi, shift=0):
        return transposed_ref(F, yrow0, col0, mo, lo, hi, shift)
    P, RS = run_transposed(F, yrow0, krows, col0, mo, splits, ldp)
    return check_slices(P, RS, ref, krows, splits, lambda lo, hi: ref(lo, hi, sh))


@pytest.mark.parametrize("col0,mo", [(128, 128), (256, 100), (512, 200)])
@pytest.mark.parametrize("yrow0,krows", [(0, 16), (128, 48), (256, 144), (0, 256)])
def test_transposed_matches_fp64(yrow0, krows, col0, mo):
    """dsvgd_phi_h2_transposed in 1, 2 and 3 slices; (128, 48) x (128, 128)
    and (256, 144) x (256, 100) contain the diagonal, which the transposed
    partial does not skip."""
    F = full(1000)
    for splits in (1, 2, 3):
        e, e_r = check_transposed(F, yrow0, krows, col0, mo, splits, F.ldy + 16)
        record_parity(e, rowsum=e_r, splits=splits)


def test_transposed_pad_rows_weigh_zero():
    """n = 300: rows 300 .. 383 of the rectangle are pads (D = +inf, Y = 0)."""
    F = full(300)
    for splits in (1, 2):
        e, e_r = check_transposed(F, 256, 128, 0, 100, splits, F.ldy)
        record_parity(e, rowsum=e_r, splits=splits)


# --------------------------------------- A3. the batched forward blocks --
def run_blocks(F, yrow0, m, first, nblocks, count, zsplit, ldp, pstride, split_entry):
    N = native()
    P = nan_buf(zsplit * count * pstride + 64)
    args = (F.Dp + 4 * yrow0 * F.n_pad, F.n_pad, F.Yx, F.ldy, yrow0, m, first, nblocks, count)
    tail = (F.n, F.st, N.ptr(P), ldp, pstride, F.colinv, None, 0, stream())
    if split_entry:
        N.call("dsvgd_phi_h2_transposed_blocks_split", *(args + (zsplit,) + tail))
    else:
        assert zsplit == 1
        N.call("dsvgd_phi_h2_transposed_blocks", *(args + tail))
    torch.cuda.synchronize()
    return P


def unpack_blocks(P, m, count, zsplit, ld, stride, ldy):
    """(zsplit, count, m, ldy) products and (zsplit, count, m) row sums of a
    [m x ld | m row sums] message buffer; everything else must be NaN."""
    body = P[:zsplit * count * stride].view(zsplit, count, stride)
    assert all_nan(P[zsplit * count * stride:]) and all_nan(body[:, :, m * ld + m:])
    mat = body[:, :, :m * ld].view(zsplit, count, m, ld)
    assert all_nan(mat[..., ldy:])
    return mat[..., :ldy], body[:, :, m * ld:m * ld + m]


@pytest.mark.parametrize("zsplit", [1, 2, 4])
@pytest.mark.parametrize("m", [128, 256])
def test_transposed_blocks_match_fp64(m, zsplit):
    """dsvgd_phi_h2_transposed_blocks (zsplit = 1) / _blocks_split of rank 1's
    rows: the blocks (nblocks - 1, 0, 1) -- a wrap, and the diagonal block --
    and a single one; every block and slice, then
    dsvgd_phi_partial_reduce_blocks of the slices, against fp64.  zsplit = 1
    gives the bits of dsvgd_phi_h2_transposed on the same block."""
    N = native()
    F = full(1024)
    nblocks = F.n_pad // m
    yrow0, ldp, ldo = m, F.ldy + 16, F.ldy + 8
    pstride, ostride = m * ldp + m + 64, m * ldo + m + 12
    worst, worst_r = 0.0, 0.0
    for first, count in ((nblocks - 1, 3), (2, 1)):
        P = run_blocks(F, yrow0, m, first, nblocks, count, zsplit, ldp, pstride, zsplit > 1)
        mat, rs = unpack_blocks(P, m, count, zsplit, ldp, pstride, F.ldy)
        for q in range(count):
            cb = (first + q) % nblocks

            def ref(lo, hi, shift=0):
                return transposed_ref(F, yrow0, cb * m, m, lo, hi, shift)
            e, e_r = check_slices(mat[:, q], rs[:, q], ref, m, zsplit,
                                  lambda lo, hi: ref(lo, hi, 16))
            worst, worst_r = max(worst, e), max(worst_r, e_r)
            if zsplit == 1:
                P1, R1 = run_transposed(F, yrow0, m, cb * m, m, 1, ldp)
                assert same_bits(P1[0], mat[0, q]) and same_bits(R1[0], rs[0, q])
        out = nan_buf(count * ostride + 64)
        N.call("dsvgd_phi_partial_reduce_blocks", N.ptr(P), ldp, pstride, zsplit, count, m,
               F.ldy, N.ptr(out), ldo, ostride, stream())
        torch.cuda.synchronize()
        omat, ors = unpack_blocks(out, m, count, 1, ldo, ostride, F.ldy)
        for q in range(count):
            Pq, rq = transposed_ref(F, yrow0, ((first + q) % nblocks) * m, m, 0, m)
            e, e_r = max_err(omat[0, q].double(), Pq), max_err(ors[0, q].double(), rq)
            worst, worst_r = max(worst, e), max(worst_r, e_r)
            assert e < KY_TOL and e_r < RS_TOL, (q, e, e_r)
    record_parity(worst, rowsum=worst_r)


def test_transposed_blocks_xcd_map_gives_identical_bits():
    """m = 256, two blocks in two slices: 8 workgroups, a grid the XCD map of
    the batched partials (dsvgd_phi_set_xmap bit 4) applies to."""
    F = full(1024)
    lib = native().load()
    m, ldp = 256, F.ldy
    pstride = m * ldp + m
    out = {}
    for mask in (7, 0):
        prev = lib.dsvgd_phi_set_xmap(mask)
        try:
            out[mask] = run_blocks(F, m, m, 2, F.n_pad // m, 2, 2, ldp, pstride, True)
        finally:
            lib.dsvgd_phi_set_xmap(prev)
    assert not bool(torch.isnan(out[0][:4 * pstride]).any())
    assert same_bits(out[7], out[0])


# ------------------------------------ B1. the partial reductions, exact --
def reduce_order(parts):
    """numpy float32 restatement of partial_reduce_kernel's order (csrc/phi.hip):
    G = the slice count rounded up to a power of two, at most 16; group g sums
    the slices g, g + G, ... from zero; the group sums are added in g order."""
    Z = parts.shape[0]
    G = 1
    while G < Z and G < 16:
        G *= 2
    groups = []
    for g in range(G):
        a = np.zeros(parts.shape[1:], np.float32)
        for z in range(g, Z, G):
            a = a + parts[z]
        groups.append(a)
    total = groups[0]
    for g in range(1, G):
        total = total + groups[g]
    return total


@pytest.mark.parametrize("splits", [1, 3, 16, 17, 40])
def test_partial_reduce_bits(splits):
    """dsvgd_phi_partial_reduce on synthetic partials: the bits of the
    documented order, for row counts whose row-sum tail is no multiple of 4,
    ldp > cols, ldo > cols; the outputs' padding untouched."""
    N = native()
    rs_ = np.random.RandomState(splits)
    for rows in (1, 5, 130):
        for cols in (4, 512):
            ldp, ldo, rp = cols + 8, cols + 4, pad128(rows)
            Pn = rs_.randn(splits, rows, ldp).astype(np.float32)
            Rn = rs_.randn(splits, rp).astype(np.float32)
            Pg, Rg = gpu(Pn), gpu(Rn)
            out, out_rs = nan_buf(rows + 2, ldo), nan_buf(rows + 7)
            N.call("dsvgd_phi_partial_reduce", N.ptr(Pg), ldp, N.ptr(Rg), splits, rows, cols,
                   N.ptr(out), ldo, N.ptr(out_rs), stream())
            torch.cuda.synchronize()
            assert all_nan(out[rows:]) and all_nan(out[:, cols:]) and all_nan(out_rs[rows:])
            got, got_rs = out[:rows, :cols].cpu().numpy(), out_rs[:rows].cpu().numpy()
            want, want_rs = reduce_order(Pn[:, :, :cols]), reduce_order(Rn[:, :rows])
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rows, cols)
            assert np.array_equal(got_rs.view(np.uint32), want_rs.view(np.uint32)), (rows, cols)


@pytest.mark.parametrize("splits", [1, 3, 16, 17, 40])
def test_partial_reduce_blocks_bits(splits):
    """dsvgd_phi_partial_reduce_blocks: the same order per block, for 1 and 3
    blocks with pstride and ostride above their minimum."""
    N = native()
    rs_ = np.random.RandomState(100 + splits)
    for count in (1, 3):
        for rows, cols in ((1, 512), (5, 4), (130, 4), (130, 512)):
            ldp, ldo = cols + 8, cols + 4
            pstride, ostride = rows * ldp + pad128(rows) + 12, rows * ldo + rows + 12 - rows % 4
            assert pstride % 4 == 0 and ostride % 4 == 0 and ostride >= rows * ldo + rows
            Pn = rs_.randn(splits, count, pstride).astype(np.float32)
            Pg = gpu(Pn)
            out = nan_buf(count * ostride + 16)
            N.call("dsvgd_phi_partial_reduce_blocks", N.ptr(Pg), ldp, pstride, splits, count,
                   rows, cols, N.ptr(out), ldo, ostride, stream())
            torch.cuda.synchronize()
            assert all_nan(out[count * ostride:])
            o = out[:count * ostride].view(count, ostride)
            assert all_nan(o[:, rows * ldo + rows:])
            omat = o[:, :rows * ldo].view(count, rows, ldo)
            assert all_nan(omat[:, :, cols:])
            got = omat[:, :, :cols].cpu().numpy()
            got_rs = o[:, rows * ldo:rows * ldo + rows].cpu().numpy()
            mat = Pn[:, :, :rows * ldp].reshape(splits, count, rows, ldp)[..., :cols]
            want = reduce_order(np.ascontiguousarray(mat))
            want_rs = reduce_order(np.ascontiguousarray(Pn[:, :, rows * ldp:rows * ldp + rows]))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (count, rows, cols)
            assert np.array_equal(np.ascontiguousarray(got_rs).view(np.uint32),
                                  want_rs.view(np.uint32)), (count, rows, cols)


# ------------------------------ B2 / B3. the pair-split median, lockstep --
def pair_engines(S, m):
    """The S pair-split engines of one process on the same particles, after
    pack (the distances are the caller's)."""
    n = S * m
    X, Sc = _inputs(n)
    Xg, Sg = gpu(X), gpu(Sc)
    engs = []
    for r in range(S):
        eng = dsvgd().PhiEngine(n, DIM, m=m, row0=r * m, device=DEV, pair_split=(r, S))
        assert eng.plan is not None
        eng.pack(Xg, Sg)
        engs.append(eng)
    return engs


def stored_tiles(eng):
    """(D of the owned rows as numpy (m, n), the select weight of every entry):
    weight 0 marks tiles the rank does not hold (never written)."""
    Dd = eng.dense_D(padded=True).cpu().numpy()
    W = np.kron(np.array(eng.plan.tile_weights(), np.int64), np.ones((128, 128), np.int64))
    assert W.shape == Dd.shape
    return Dd, W


def assemble(engs):
    """The symmetric n x n matrix from the ranks' own stored fp32 tiles (a
    weight-2 tile mirrored); every entry must be covered exactly once."""
    n, m = engs[0].n, engs[0].m
    full_, cover = np.full((n, n), np.nan, np.float32), np.zeros((n, n), np.int64)
    tiles = []
    for r, eng in enumerate(engs):
        Dd, W = stored_tiles(eng)
        tiles.append((Dd, W))
        for I in range(m // 128):
            for J in range(n // 128):
                w = W[I * 128, J * 128]
                if w == 0:
                    continue
                rr = slice(r * m + I * 128, r * m + (I + 1) * 128)
                cc = slice(J * 128, (J + 1) * 128)
                blk = Dd[I * 128:(I + 1) * 128, cc]
                full_[rr, cc] = blk
                cover[rr, cc] += 1
                if w == 2:
                    full_[cc, rr] = blk.T
                    cover[cc, rr] += 1
    assert (cover == 1).all() and np.isfinite(full_).all()
    return full_, tiles


def lockstep_select(engs, with_cand):
    """The three radix passes at the ABI with the host as the all-reduce:
    dsvgd_radix_hist_wmap on every rank, the histograms summed and written
    back, dsvgd_radix_pick on every rank.  Returns pass 1's per-rank
    histograms (before the sum)."""
    N = native()
    first = None
    for p in (1, 2, 3):
        for eng in engs:
            N.call("dsvgd_radix_hist_wmap", N.ptr(eng.D), eng.m_pad, eng.n_pad,
                   N.ptr(eng.cand) if with_cand else None, p, eng.state.ptr, N.ptr(eng.wmap),
                   stream())
        torch.cuda.synchronize()
        hists = [eng.state.hist.clone() for eng in engs]
        if p == 1:
            first = [h.cpu().numpy() for h in hists]
        total = torch.stack(hists).sum(0)
        for eng in engs:
            eng.state.hist.copy_(total)
            N.call("dsvgd_radix_pick", eng.state.ptr, p, stream())
    torch.cuda.synchronize()
    return first


def check_median(engs, full_):
    n = engs[0].n
    k = (n * n - 1) // 2
    want = np.partition(full_.ravel(), k)[k]
    for eng in engs:
        med, h, _ = eng.state.read()
        assert np.float32(med).view(np.uint32) == want.view(np.uint32), (med, want)
        assert h == pytest.approx(med / np.log(n), rel=1e-6)


@pytest.mark.parametrize("S,m", [(2, 512), (3, 256)])
def test_wmap_select_without_candidates(S, m):
    """dsvgd_radix_hist_wmap with cand = NULL on every rank: (a) pass 1's
    histogram is the weighted histogram of key bits 31..21 over the rank's
    stored tiles, (b) the median is the same on every rank and the bits of
    np.partition at k = (n^2 - 1) // 2 over the assembled matrix, (c) h =
    median / log n."""
    N = native()
    engs = pair_engines(S, m)
    for eng in engs:
        assert not eng.bracketed
        eng.distances(median=False)
        N.call("dsvgd_select_init", eng.state.ptr, eng.n, -1, stream())
    torch.cuda.synchronize()
    full_, tiles = assemble(engs)
    first = lockstep_select(engs, False)
    for (Dd, W), h1 in zip(tiles, first):
        keys = Dd.view(np.uint32) >> 21
        want = np.bincount(keys[W > 0], weights=W[W > 0], minlength=2048).astype(np.int64)
        assert np.array_equal(h1, want)
    assert sum(int(h1.sum()) for h1 in first) == engs[0].n ** 2
    check_median(engs, full_)


@pytest.mark.parametrize("S,m", [(2, 512), (3, 256)])
def test_parts_bracket_counts_and_forced_miss(S, m, monkeypatch):
    """dsvgd_sqdist_h2_parts with the bracket accounting at a small shape
    (BRACKET_MIN_ENTRIES lowered): per rank, below / ncand equal the weighted
    numpy counts over its stored tiles, and they add up to the whole
    matrix's; the select over the candidates gives the exact median.  Then a
    bracket that cannot hold rank k (k_lo = k_hi = 0): after the totals are
    summed over the ranks dsvgd_bracket_check sets fallback on every rank and
    the passes -- handed the candidates all the same -- read D through the
    weight map and still find the exact median."""
    N = native()
    monkeypatch.setattr(dsvgd().PhiEngine, "BRACKET_MIN_ENTRIES", 1)
    engs = pair_engines(S, m)
    n = S * m
    k = (n * n - 1) // 2
    for miss in (False, True):
        for eng in engs:
            assert eng.bracketed
            if miss:
                eng.k_lo = eng.k_hi = 0
            eng.distances(median=True)
            N.call("dsvgd_bracket_totals", eng.state.ptr, N.ptr(eng.cand), stream())
        torch.cuda.synchronize()
        full_, tiles = assemble(engs)
        br = [eng.state.bracket() for eng in engs]
        lo, hi = np.float32(br[0][0]), np.float32(br[0][1])
        assert lo <= hi
        for (Dd, W), b in zip(tiles, br):
            assert (np.float32(b[0]), np.float32(b[1])) == (lo, hi)
            held = W > 0
            assert b[2] == int((W * (Dd < lo))[held].sum())
            assert b[3] == int((W * ((Dd >= lo) & (Dd <= hi)))[held].sum())
        below, ncand = sum(b[2] for b in br), sum(b[3] for b in br)
        assert below == int((full_ < lo).sum())
        assert ncand == int(((full_ >= lo) & (full_ <= hi)).sum())
        total = torch.stack([eng.state.totals.clone() for eng in engs]).sum(0)
        for eng in engs:
            eng.state.totals.copy_(total)
            N.call("dsvgd_bracket_check", eng.state.ptr, stream())
        torch.cuda.synchronize()
        hit = below <= k < below + ncand
        assert hit == (not miss)
        for eng in engs:
            assert eng.state.bracket()[4] == (1 if miss else 0)
        lockstep_select(engs, True)
        check_median(engs, full_)


# ------------------------------------ B4. the shares of the bracket sample --
@pytest.mark.parametrize("ldy", [512, 258])
def test_sample_sqdist_range_bits(ldy):
    """dsvgd_sample_sqdist_range over three uneven ranges (bounds no multiples
    of 4) writes, concatenated, the bits of dsvgd_sample_sqdist -- on the
    16-byte-row path and with ldy % 4 != 0 (one wave per pair)."""
    N = native()
    n, d, s, seed = 1000, DIM, 1001, 0x5EED5EED
    Y = gpu(np.random.RandomState(ldy).randn(n, ldy))
    whole, shares = nan_buf(s + 5), nan_buf(s + 5)
    N.call("dsvgd_sample_sqdist", N.ptr(Y), ldy, n, d, s, seed, N.ptr(whole), stream())
    for p0, p1 in ((0, 333), (333, 702), (702, s)):
        N.call("dsvgd_sample_sqdist_range", N.ptr(Y), ldy, n, d, s, seed, p0, p1, N.ptr(shares),
               stream())
    torch.cuda.synchronize()
    assert all_nan(whole[s:]) and not bool(torch.isnan(whole[:s]).any())
    assert bool((whole[:s] > 0).any())
    assert same_bits(whole, shares)


# ------------------------------------------- C1. dsvgd_phi_finish_parts --
@pytest.mark.parametrize("gate,nparts,use_extra,write_phi,move", [
    (None, 3, True, True, True),     # the parts, extra, phi and X
    (0.0, 3, False, False, True),    # a gate that reads 0: the parts count; X only
    (1.0, 3, True, True, True),      # a gate that reads nonzero: splits_fb own slices, no parts
    (None, 0, False, True, False),   # no parts; phi only
])
def test_finish_parts_matches_formula(gate, nparts, use_extra, write_phi, move):
    """phi = inv_n ((s + KS) + (2/h)(r xc - KXc)) (+ extra) over the own
    slices plus three overlapping parts (one with its own ldk), in fp64."""
    N = native()
    m, d, dp, row0 = 300, 200, 224, 7
    ldk, ldy, ldphi, ldx, lde = 2 * dp, 2 * dp + 16, d + 8, d + 4, d + 12
    splits, splits_fb, step, inv_n, h = 3, 4, 0.25, 1.0 / 1234.0, 1.5
    mp = pad128(m)
    rs_ = np.random.RandomState(17)
    KY = gpu(rs_.randn(splits_fb, m, ldk))
    RS = gpu(rs_.uniform(0.0, 1.0, (splits_fb, mp)))
    Y = gpu(rs_.randn(row0 + m, ldy))
    extra = gpu(rs_.randn(m, lde))
    specs = [(0, 300, 2, ldk), (128, 100, 1, 2 * dp + 8), (0, 150, 4, ldk)][:nparts]
    bufs = [(gpu(rs_.randn(z, rows, lk)), gpu(rs_.uniform(0.0, 1.0, (z, pad128(rows)))))
            for _, rows, z, lk in specs]
    arr = (N.PhiPart * max(1, len(specs)))()
    for a, (ro, rows, z, lk), (ky, rsum) in zip(arr, specs, bufs):
        a.ky, a.rs, a.ldk, a.row_off, a.rows, a.splits = N.ptr(ky), N.ptr(rsum), lk, ro, rows, z
    st = dsvgd().engine.SelectState(torch.device(DEV))
    N.call("dsvgd_set_bandwidth", st.ptr, h, stream())
    g = None if gate is None else gpu(np.array([gate]))
    phi = nan_buf(m + 2, ldphi)
    X0 = gpu(rs_.randn(m, ldx))
    X = X0.clone()
    N.call("dsvgd_phi_finish_parts", N.ptr(KY), ldk, N.ptr(RS), splits, N.ptr(Y), ldy, row0, m, d,
           dp, st.ptr, inv_n, step, N.ptr(extra) if use_extra else None, lde,
           N.ptr(phi) if write_phi else None, ldphi, N.ptr(X) if move else None, ldx,
           ctypes.addressof(arr) if specs else None, len(specs), N.ptr(g), splits_fb, stream())
    torch.cuda.synchronize()
    fb = gate is not None and gate != 0.0
    ns = splits_fb if fb else splits
    kx = KY[:ns, :, :d].double().sum(0)
    ks = KY[:ns, :, dp:dp + d].double().sum(0)
    r = RS[:ns, :m].double().sum(0)
    if not fb:
        for (ro, rows, z, lk), (ky, rsum) in zip(specs, bufs):
            kx[ro:ro + rows] += ky[:, :, :d].double().sum(0)
            ks[ro:ro + rows] += ky[:, :, dp:dp + d].double().sum(0)
            r[ro:ro + rows] += rsum[:, :rows].double().sum(0)
    inv_h = float(np.float32(st.read()[2]))
    yi = Y[row0:row0 + m].double()
    ref = float(np.float32(inv_n)) * ((yi[:, dp:dp + d] + ks)
                                      + 2.0 * inv_h * (r[:, None] * yi[:, :d] - kx))
    if use_extra:
        ref = ref + extra[:, :d].double()
    if write_phi:
        assert all_nan(phi[m:]) and all_nan(phi[:, d:])
        e = max_err(phi[:m, :d].double(), ref)
        record_parity(e)
        assert e < PHI_TOL, e
    else:
        assert all_nan(phi)
    if move:
        assert torch.equal(X[:, d:], X0[:, d:])
        X1 = X[:, :d].double()
        tol = step * PHI_TOL * float(ref.abs().max()) + \
            2 * torch.as_tensor(np.spacing(np.abs(X[:, :d].cpu().numpy())), device=DEV).double()
        assert bool(((X1 - (X0[:, :d].double() + step * ref)).abs() <= tol).all())
    else:
        assert torch.equal(X, X0)


# ------------------------------ C2. the whole layout, every row, one process --
_phi_ref = {}


def oracle_phi(key, X, Sc, h):
    if key not in _phi_ref:
        _phi_ref[key] = O.phi(X, Sc, h)
    return _phi_ref[key]


def pair_split_phi(S, m, X, Sc, h):
    """phi of all n = S m rows from S pair-split engines in this process: two
    passes of every rank's step (pack, distances, bandwidth, direction), the
    first with a p2p stub that keeps a copy of every send buffer keyed by
    (src, dest), the second with one that copies them into the receive
    buffers before the finish.  Returns (phi (n, d) numpy, the engines)."""
    n = S * m
    Xg, Sg = gpu(X), gpu(Sc)
    engs = [dsvgd().PhiEngine(n, DIM, m=m, row0=r * m, device=DEV, pair_split=(r, S))
            for r in range(S)]
    sent = {}
    for deliver in (False, True):
        for r, eng in enumerate(engs):
            def p2p(sends, recvs, r=r):
                if deliver:
                    for buf, src in recvs:
                        buf.copy_(sent[src, r])
                else:
                    for buf, dest in sends:
                        assert (r, dest) not in sent
                        sent[r, dest] = buf.clone()
                return None
            eng.pack(Xg, Sg)
            eng.distances(median=False)
            eng.fixed_bandwidth(h)
            eng.direction(Xg[r * m:(r + 1) * m].clone(), 0.0, write_phi=True, p2p=p2p)
    torch.cuda.synchronize()
    assert len(sent) == sum(len(eng.plan.sends) for eng in engs)
    return torch.cat([eng.phi for eng in engs]).cpu().numpy(), engs


def check_layout(S, m):
    X, Sc = _inputs(S * m)
    phi, engs = pair_split_phi(S, m, X, Sc, H_FIX)
    assert all(eng.range_guard() is False for eng in engs)
    ref = oracle_phi((S * m, "fixture"), X, Sc, H_FIX)
    e = float(np.abs(phi - ref).max() / np.abs(ref).max())
    assert e < PHI_TOL, e
    return e, engs


@pytest.mark.parametrize("S,m", [(2, 512), (3, 256), (4, 512), (5, 256)])
def test_layout_every_row_matches_oracle(S, m):
    record_parity(check_layout(S, m)[0], S=S)


@pytest.mark.parametrize("square", [True, False])
@pytest.mark.parametrize("S", [2, 4])
def test_layout_full_square_forced(S, square):
    """The diagonal square as one full rectangle and as upper tiles + mirror
    stores, at both S."""
    from dsvgd.pairsplit import PairSplitPlan
    prev = PairSplitPlan.FULL_SQUARE
    PairSplitPlan.FULL_SQUARE = square
    try:
        e, engs = check_layout(S, 512)
        kind = PairSplitPlan.GRAM_RECT if square else PairSplitPlan.GRAM_DIAG
        assert all(eng.plan.gram_parts[0]["kind"] == kind for eng in engs)
        record_parity(e, S=S, square=square)
    finally:
        PairSplitPlan.FULL_SQUARE = prev


@pytest.mark.parametrize("z", [1, 2])
def test_layout_s5_forward_zsplit(z):
    """S = 5 with PhiEngine.FWD_ZSPLIT set.  (At m = 256 the two forward
    blocks are 4 workgroups, far from the 192 at which the engine batches
    them, so the setting selects nothing here: the batched kernels are the
    subject of test_transposed_blocks_match_fp64.)"""
    E = dsvgd().PhiEngine
    prev = E.FWD_ZSPLIT
    E.FWD_ZSPLIT = z
    try:
        e, engs = check_layout(5, 256)
        assert not any(eng.fwd_batched for eng in engs)
        record_parity(e, z=z)
    finally:
        E.FWD_ZSPLIT = prev


def test_layout_range_guard_fallback():
    """S = 2 with one particle 2^20 * 0.1 away: the FmtH2 range guard trips on
    both ranks, which then run the FmtX3 phi_mm over their whole row block;
    every row within ROW_TOL, row-normalised."""
    S, m = 2, 512
    n = S * m
    rs_ = np.random.RandomState(7)
    X = (0.1 * rs_.randn(n, DIM)).astype(np.float32)
    X[700, 1:] += np.float32(2.0 ** 20 * 0.1)
    Sc = (-X + 0.3 * rs_.randn(n, DIM)).astype(np.float32)
    h = 2.0 * DIM * 0.01 / 8.0
    phi, engs = pair_split_phi(S, m, X, Sc, h)
    assert all(eng.range_guard() is True for eng in engs)
    e = row_err(phi, O.phi(X, Sc, h))
    record_parity(float(e.max()), row=int(e.argmax()))
    assert e.max() <= ROW_TOL, (e.max(), int(e.argmax()))
