"""Host-side reference of the dsvgd_phi_mm* entry points and their finish
kernels (numpy only; no torch.cuda): the dispatch of a shape, the K-steps
every split-K slice of every form takes, the fp64 product over exactly those
K-steps, the defects a slice-by-slice check is meant to notice, the fixture
with its conditions, the finish formulas with their derived bound and a
float32 restatement of the finish kernels' order, and the case tables.

Shared by tests/test_phi_mm_host.py (which pins all of it without a GPU) and
tests/test_gpu_phi_mm_kernels.py (which runs the kernels against it).

A K-step is 16 consecutive columns of D (rows of the B operand); K = n_pad.
FORMS of a launch's split-K slices (csrc/phi.hip, csrc/phi_w1.hpp):
  "c32"    contiguous, kchunk = roundup(ceil(K / splits), 32): nn_kernel (the
           f32 engine; launch_nn takes BJ = 32 since K % 32 == 0)
  "c16"    contiguous, kchunk = roundup(ceil(K / splits), 16): nn_x3_kernel on
           both split engines and phi_w1_kernel DS 0 (full layout)
  "rows"   the same ranges walked by phi_w1_kernel DS 4 (the symmetric
           layout's one-launch form; transposed K-steps first); an empty
           slice is refused by the entry point
  "hybrid" phi_w1_kernel DS 1 + DS 2 (dsvgd_phi_set_symrow(0)): with sl =
           splits // 2, slice z < sl takes the K-steps z, z + sl, ... left of
           the row block's diagonal tile; slice sl + z takes every
           (splits - sl)-th K-step counted down from K / 16 - 1 - z while it
           is at or right of the diagonal tile
"""
import numpy as np

KY_TOL = 5e-6      # tests/test_gpu_split.py
RS_TOL = 1e-6      # tests/test_gpu_pairsplit_kernels.py
PHI_TOL = 1e-5
NOTICE = 100.0     # a defect must move a slice by this many tolerances
KS = 16            # columns of a K-step


def roundup(x, q):
    return -(-x // q) * q


def pad128(x):
    return roundup(max(x, 1), 128)


def dp_of(d):
    """dsvgd_dp: the padded feature width."""
    return roundup(max(d, 1), 32)


def ldy_of(dp):
    """dsvgd_ldy: the row stride of Y = [Xc | S]."""
    w = 2 * dp
    return 128 if w <= 128 else 256 if w <= 256 else roundup(w, 512)


def tn_of(ldy):
    """The column-tile template argument TN a leading dimension dispatches to."""
    return 4 if ldy % 512 == 0 else 2 if ldy % 256 == 0 else 1


def form_of(entry, ldy, sym, splits, symrow=1):
    """The slice form (above) of a launch: entry in "f32", "x3", "h2", "h2w"."""
    if entry == "f32":
        return "c32"
    if entry == "h2w":
        return "rows" if sym else "c16"
    if entry == "h2" and sym and tn_of(ldy) == 4 and splits >= 2:
        return "rows" if symrow else "hybrid"
    return "c16"


def kchunk_of(K, splits, step=KS):
    return roundup(-(-K // splits), step)


def has_empty_slice(K, splits, step=KS):
    return (splits - 1) * kchunk_of(K, splits, step) >= K


def slice_ksteps(form, K, splits, z, rb=0):
    """The K-steps (ascending) slice z takes for the 128-row block rb."""
    T = K // KS
    if form == "hybrid":
        sl, dg = splits // 2, rb * (128 // KS)
        if z < sl:
            return np.arange(z, dg, sl)
        return np.arange(T - 1 - (z - sl), dg - 1, -(splits - sl))[::-1]
    kc = kchunk_of(K, splits, 32 if form == "c32" else KS)
    lo, hi = z * kc, min(K, (z + 1) * kc)
    return np.arange(lo // KS, max(lo, hi) // KS)


def slice_weights(form, K, splits, z, nrb):
    """(nrb, K / 16) multiplicities: how often slice z adds each K-step."""
    w = np.zeros((nrb, K // KS), np.int64)
    for rb in range(nrb):
        w[rb, slice_ksteps(form, K, splits, z, rb)] = 1
    return w


# ------------------------------------------------------------- defects --
def defect_shift(w):
    """One K-step taken 16 columns away: in every row block the slice's first
    K-step reads its right neighbour's columns (cyclically) instead."""
    w = w.copy()
    T = w.shape[1]
    for rb in range(w.shape[0]):
        on = np.flatnonzero(w[rb])
        if len(on):
            w[rb, on[0]] -= 1
            w[rb, (on[0] + 1) % T] += 1
    return w


def defect_boundary(form, K, splits, nrb):
    """Slice 0 with its boundary moved by one K-step: a contiguous slice
    walks one K-step past its end (a single slice, which has no inner
    boundary, starts one K-step late instead); the hybrid's slice 0 takes one
    more K-step of its progression, the first one at or past the diagonal
    tile (in row block 0, where it has none: K-step 0)."""
    w = slice_weights(form, K, splits, 0, nrb)
    for rb in range(nrb):
        ks = slice_ksteps(form, K, splits, 0, rb)
        if form == "hybrid":
            w[rb, ks[-1] + splits // 2 if len(ks) else 0] += 1
        elif splits > 1:
            w[rb, ks[-1] + 1] += 1
        else:
            w[rb, 0] -= 1
    return w


# ------------------------------------------------- the fp64 reference --
def kernel_matrix(D, inv_h, row0, pw=None, zero_diag=True):
    """fp64 K of a row block's D (m_pad x n_pad, +inf pads -> 0): exp(-D inv_h),
    or u^pw with u = 1 + D inv_h (IMQ; pw = beta - order); the diagonal
    j == row0 + i zeroed."""
    D = np.asarray(D, np.float64)
    with np.errstate(over="ignore"):
        Km = np.exp(-D * inv_h) if pw is None else (1.0 + D * inv_h) ** float(pw)
    Km[~np.isfinite(D)] = 0.0
    if zero_diag:
        i = np.arange(D.shape[0])
        ok = row0 + i < D.shape[1]
        Km[i[ok], row0 + i[ok]] = 0.0
    return Km


def w_operand(Y, dp, inv_h):
    """W = S - t Xc with t = float32(2) float32(inv_h), in fp64 on Y's values."""
    t = np.float64(np.float32(2.0) * np.float32(inv_h))
    Y = np.asarray(Y, np.float64)
    return Y[:, dp:2 * dp] - t * Y[:, :dp]


def product(Km, B, w):
    """(P, r): P[i] = sum over K-steps q of w[i // 128][q] Km[i, q] B[q] and r
    the same sum of Km -- the product over exactly the K-steps of `w`."""
    wc = np.repeat(w, KS, axis=1).astype(np.float64)
    P = np.empty((Km.shape[0], B.shape[1]))
    r = np.empty(Km.shape[0])
    for rb in range(w.shape[0]):
        rows = slice(128 * rb, 128 * (rb + 1))
        Kw = Km[rows] * wc[rb][None, :]
        P[rows] = Kw @ B
        r[rows] = Kw.sum(1)
    return P, r


def max_err(got, ref):
    """max |got - ref| / max |ref| (0 / 0 = 0)."""
    den = float(np.abs(ref).max()) if ref.size else 0.0
    num = float(np.abs(got - ref).max()) if ref.size else 0.0
    return num / den if den > 0 else num


def slice_refs(Km, B, form, splits, m):
    """[(P_z, r_z)] over the live rows [0, m) for every slice, and the whole."""
    K, nrb = Km.shape[1], Km.shape[0] // 128
    out = []
    for z in range(splits):
        P, r = product(Km, B, slice_weights(form, K, splits, z, nrb))
        out.append((P[:m], r[:m]))
    P, r = product(Km, B, np.ones((nrb, K // KS), np.int64))
    return out, (P[:m], r[:m])


def sensitivity(Km, Kfull, B, form, splits, m, row0):
    """What each defect moves, in fp64, max-normalised over the live rows:
    {"shift": (eP, er), "boundary": (eP, er), "diagonal": (eP, er)}.  shift:
    the first slice that takes a K-step at all (slice 0, but for the hybrid
    on a single row block); boundary: slice 0; diagonal: row m - 1 -- a row
    of the last, ragged tile -- keeps its own column in the slice that holds
    it.  (A slice whose true product is zero is measured absolutely.)"""
    K, nrb = Km.shape[1], Km.shape[0] // 128
    out = {}

    def moved(z, wd, Kd=Km):
        P0, r0 = product(Km, B, slice_weights(form, K, splits, z, nrb))
        P1, r1 = product(Kd, B, wd)
        return max_err(P1[:m], P0[:m]), max_err(r1[:m], r0[:m])
    zs = next(z for z in range(splits) if slice_weights(form, K, splits, z, nrb).any())
    out["shift"] = moved(zs, defect_shift(slice_weights(form, K, splits, zs, nrb)))
    out["boundary"] = moved(0, defect_boundary(form, K, splits, nrb))
    i = m - 1
    q = (row0 + i) // KS
    zd = [z for z in range(splits) if q in slice_ksteps(form, K, splits, z, i // 128)]
    assert len(zd) == 1, zd
    Kd = Km.copy()
    Kd[i, row0 + i] = Kfull[i, row0 + i]
    out["diagonal"] = moved(zd[0], slice_weights(form, K, splits, zd[0], nrb), Kd)
    return out


def noticed(sens):
    """Every defect moves the product by > 100 KY_TOL and the row sums by >
    100 RS_TOL."""
    return all(eP > NOTICE * KY_TOL and er > NOTICE * RS_TOL for eP, er in sens.values())


# -------------------------------------------------------------- fixture --
_inputs = {}


def inputs(n, d):
    """randn particles whose per-row radius varies by about 2x; scores -x +
    noise (the pair-split kernel test's recipe)."""
    if (n, d) not in _inputs:
        rs = np.random.RandomState(1000 + n + 7 * d)
        X = (rs.randn(n, d) * rs.uniform(0.6, 1.4, (n, 1))).astype(np.float32)
        _inputs[n, d] = (X, (-X + 0.3 * rs.randn(n, d)).astype(np.float32))
    return _inputs[n, d]


def sqdist64(X):
    X = np.asarray(X, np.float64)
    g = (X * X).sum(1)
    return np.maximum(g[:, None] + g[None, :] - 2.0 * X @ X.T, 0.0)


def bandwidth(n, d):
    """h = (mean off-diagonal squared distance) / f, f = 3 (d >= 100) or 2."""
    D = sqdist64(inputs(n, d)[0] - inputs(n, d)[0].mean(0))
    f = 3.0 if d >= 100 else 2.0
    return float(np.float32(D[~np.eye(n, dtype=bool)].mean() / f))


def fixture_weights(n, d):
    """The off-diagonal RBF weights of the fixture at its bandwidth."""
    X = inputs(n, d)[0].astype(np.float64)
    D = sqdist64(X - X.mean(0))
    return np.exp(-D[~np.eye(n, dtype=bool)] / bandwidth(n, d))


def host_operands(n, d, m=None, row0=0):
    """(D, Y, inv_h) as an engine holds them, built on the host in fp64: D of
    the rows [row0, row0 + m) padded to (m_pad, n_pad) with +inf, Y = [Xc | S]
    (n_pad x ldy, zero pads, Xc = X - mean), inv_h = float32(1 / h)."""
    m = n if m is None else m
    X, S = inputs(n, d)
    dp = dp_of(d)
    ldy, n_pad, m_pad = ldy_of(dp), pad128(n), pad128(m)
    Xc = X.astype(np.float64) - X.astype(np.float64).mean(0)
    Y = np.zeros((n_pad, ldy))
    Y[:n, :d] = Xc
    Y[:n, dp:dp + d] = S
    D = np.full((m_pad, n_pad), np.inf)
    D[:m, :n] = sqdist64(Xc)[row0:row0 + m]
    inv_h = float(np.float32(1.0) / np.float32(bandwidth(n, d)))
    return D, Y, inv_h


# ------------------------------------------------- the finish kernels --
EPS = 2.0 ** -24


def finish_ref(kind, a):
    """(p64, A): the formula in the comment above the finish kernel `kind`
    ("xs": phi_finish_kernel, "w": phi_finish_w_kernel with the guard word 0,
    "imq": phi_finish_imq_kernel) in fp64 on the fp32 inputs of `a`, and A,
    the same formula with every term replaced by its absolute value.
    a: KY (splits, m, >= 2 dp) [w: KW (splits, m, >= dp); imq: KF, KG], RS
    (splits, >= m), Y (rows, >= 2 dp), row0, m, d, dp, inv_h, inv_n, extra
    (m, >= d) or None, beta (imq)."""
    m, d, dp, row0 = a["m"], a["d"], a["dp"], a["row0"]
    f = np.float64
    yi = a["Y"][row0:row0 + m].astype(f)
    yx, ys = yi[:, :d], yi[:, dp:dp + d]
    RS = a["RS"][:, :m].astype(f)
    r, ra = RS.sum(0)[:, None], np.abs(RS).sum(0)[:, None]
    inv_n = f(np.float32(a["inv_n"]))
    c = 2.0 * f(np.float32(a["inv_h"]))
    if kind == "xs":
        KY = a["KY"].astype(f)
        kx, ks = KY[:, :, :d], KY[:, :, dp:dp + d]
        p = inv_n * ((ys + ks.sum(0)) + c * (r * yx - kx.sum(0)))
        A = inv_n * ((np.abs(ys) + np.abs(ks).sum(0)) + c * (ra * np.abs(yx) + np.abs(kx).sum(0)))
    elif kind == "w":
        kw = a["KW"].astype(f)[:, :, :d]
        p = inv_n * ((ys + kw.sum(0)) + c * (r * yx))
        A = inv_n * ((np.abs(ys) + np.abs(kw).sum(0)) + c * (ra * np.abs(yx)))
    else:
        c = -f(np.float32(a["beta"])) * c
        fs = a["KF"].astype(f)[:, :, dp:dp + d]
        gx = a["KG"].astype(f)[:, :, :d]
        p = inv_n * ((ys + fs.sum(0)) + c * (r * yx - gx.sum(0)))
        A = inv_n * ((np.abs(ys) + np.abs(fs).sum(0)) + abs(c) * (ra * np.abs(yx) + np.abs(gx).sum(0)))
    if a.get("extra") is not None:
        ex = a["extra"][:, :d].astype(f)
        p, A = p + ex, A + np.abs(ex)
    return p, A


def finish_bound(A, splits):
    """|p - p64| <= (splits + 8) 2^-24 A: every fp32 operation adds at most
    2^-24 of the running absolute sum; at most splits - 1 additions per
    partial sum and fewer than eight further operations."""
    return (splits + 8) * EPS * A


def move_bound(A, splits, step, x0, p64):
    """|x - (x0 + step p64)| <= |step| finish_bound + 2^-23 (|x0| + |step p64|)."""
    return abs(step) * finish_bound(A, splits) + 2.0 * EPS * (np.abs(x0) + np.abs(step * p64))


def finish_f32(kind, a):
    """float32 numpy restatement of the finish kernel's own order (slices
    summed from zero in slice order, then the expression as written)."""
    m, d, dp, row0 = a["m"], a["d"], a["dp"], a["row0"]
    f = np.float32
    yi = a["Y"][row0:row0 + m].astype(f)
    yx, ys = yi[:, :d], yi[:, dp:dp + d]
    inv_n = f(a["inv_n"])
    c = f(2.0) * f(a["inv_h"])

    def ssum(parts):
        acc = np.zeros(parts.shape[1:], f)
        for z in range(parts.shape[0]):
            acc = acc + parts[z].astype(f)
        return acc
    r = ssum(a["RS"][:, :m])[:, None]
    if kind == "xs":
        kx, ks = ssum(a["KY"][:, :, :d]), ssum(a["KY"][:, :, dp:dp + d])
        p = inv_n * ((ys + ks) + c * (r * yx - kx))
    elif kind == "w":
        p = inv_n * ((ys + ssum(a["KW"][:, :, :d])) + c * (r * yx))
    else:
        c = f(-2.0) * f(a["beta"]) * f(a["inv_h"])
        fs, gx = ssum(a["KF"][:, :, dp:dp + d]), ssum(a["KG"][:, :, :d])
        p = inv_n * ((ys + fs) + c * (r * yx - gx))
    if a.get("extra") is not None:
        p = p + a["extra"][:, :d].astype(f)
    assert p.dtype == f
    return p


# (id, m, row0, splits, d, extra, phi, X, path): the shapes of section B.
# path: "vec" four columns per thread; the scalar kernel by "d" (d % 4 != 0),
# "xalign" (X one float off 16-byte alignment) or "ldphi" (an odd ldphi)
FINISH_SHAPES = [
    ("all_vec", 130, 7, 3, 200, True, True, True, "vec"),
    ("one_row_phi_only", 1, 0, 1, 200, False, True, False, "vec"),
    ("move_only", 130, 0, 3, 200, True, False, True, "vec"),
    ("no_extra", 130, 7, 1, 200, False, True, True, "vec"),
    ("scalar_d", 130, 7, 3, 203, True, True, True, "d"),
    ("scalar_x_misaligned", 130, 0, 3, 200, True, True, True, "xalign"),
    ("scalar_odd_ldphi", 1, 7, 3, 200, False, True, True, "ldphi"),
    ("scalar_one_row_move_only", 1, 7, 1, 203, True, False, True, "d"),
]


def finish_inputs(shape, kind, seed=0):
    """Synthetic fp32 inputs of one FINISH_SHAPES row for finish kernel `kind`
    ("xs", "w", "imq"): every leading dimension larger than its width."""
    name, m, row0, splits, d, extra, _, _, path = shape
    dp = dp_of(d)
    rs = np.random.RandomState(seed + 31 * m + d + splits)
    f = np.float32
    a = dict(m=m, row0=row0, d=d, dp=dp, splits=splits, inv_n=f(1.0 / 1234.0), step=f(0.25),
             h=1.5, inv_h=f(1.0) / f(1.5), beta=f(-0.5),
             ldk=2 * dp + 16, ldkw=dp + 16, ldy=2 * dp + 32, lde=d + 12,
             ldphi=d + 9 if path == "ldphi" else d + 8, ldx=d + 4)
    mp = pad128(m)
    a["Y"] = rs.randn(row0 + m, a["ldy"]).astype(f)
    a["RS"] = rs.uniform(0.0, 1.0, (splits, mp)).astype(f)
    a["KY"] = rs.randn(splits, m, a["ldk"]).astype(f)
    a["KW"] = rs.randn(splits, m, a["ldkw"]).astype(f)
    a["KF"] = a["KY"]
    a["KG"] = rs.randn(splits, m, a["ldk"] + 4).astype(f)
    # the one-operand finish with its guard word set: splits + 1 two-operand slices
    a["KYfb"] = rs.randn(splits + 1, m, a["ldk"]).astype(f)
    a["RSfb"] = np.concatenate([a["RS"], rs.uniform(0.0, 1.0, (1, mp)).astype(f)])
    a["extra"] = rs.randn(m, a["lde"]).astype(f) if extra else None
    a["X0"] = rs.randn(m, a["ldx"]).astype(f)
    return a


# -------------------------------------------------------- case tables --
# Section A.  (id, entry, n, d, m, row0, layout, splits, opts): m = None is the
# whole matrix; layout "full" / "sym"; splits a tuple; opts: m16 (x3), symrow
# (h2), ldk (floats added to the minimal ldk), imq = (beta, order).
# The ABI refuses row0 + m > n, so the row block "that ends in the pads" is
# the ragged last tile itself: rows [256, 300) of n = 300.
BLOCKS = [(70, 37), (44, 256)]


def _cases():
    c = []
    # f32: nn_kernel<TN, true, 2, 2, 32>
    for d in (20, 100, 200):
        c.append(("f32_d%d_whole" % d, "f32", 300, d, None, 0, "full", (1, 2, 3), {}))
    for m, row0 in BLOCKS:
        c.append(("f32_block_%d_%d" % (m, row0), "f32", 300, 100, m, row0, "full", (1, 2),
                  dict(ldk=16)))
    c.append(("f32_empty_slice", "f32", 300, 100, None, 0, "full", (5,), {}))
    c.append(("f32_empty_past_K", "f32", 100, 100, None, 0, "full", (7,), {}))
    c.append(("f32_n512_nopad", "f32", 512, 100, None, 0, "full", (3,), dict(ldk=16)))
    # x3: nn_x3_kernel<TN, DMA, true, M16, 2, FmtX3>
    c.append(("x3_tn1", "x3", 300, 20, None, 0, "full", (1, 2, 3), dict(m16=0)))
    for d in (100, 200):
        for m16 in (1, 0):
            for n in (129, 300):
                tag = "x3_d%d_m16%d_n%d" % (d, m16, n)
                c.append((tag + "_sym", "x3", n, d, None, 0, "sym", (1, 2, 3), dict(m16=m16)))
            c.append(("x3_d%d_m16%d_full" % (d, m16), "x3", 300, d, None, 0, "full", (2,),
                      dict(m16=m16, ldk=16)))
    for m, row0 in BLOCKS:
        c.append(("x3_block_%d_%d" % (m, row0), "x3", 300, 200, m, row0, "full", (1, 2),
                  dict(m16=1, ldk=16)))
    c.append(("x3_empty_slice", "x3", 300, 200, None, 0, "sym", (7,), dict(m16=1)))
    # h2, two operands
    c.append(("h2_tn1", "h2", 300, 20, None, 0, "full", (1, 2, 3), {}))
    c.append(("h2_tn2_full", "h2", 300, 100, None, 0, "full", (1, 2, 3), dict(ldk=16)))
    c.append(("h2_tn2_sym", "h2", 300, 100, None, 0, "sym", (1, 2, 3), {}))
    c.append(("h2_tn2_sym_n129", "h2", 129, 100, None, 0, "sym", (2,), {}))
    for d in (200, 300):
        c.append(("h2_d%d_full" % d, "h2", 300, d, None, 0, "full", (1, 2, 3), dict(ldk=16)))
        for m, row0 in BLOCKS:
            c.append(("h2_d%d_block_%d_%d" % (d, m, row0), "h2", 300, d, m, row0, "full", (1, 2),
                      {}))
        c.append(("h2_d%d_sym_8wave" % d, "h2", 300, d, None, 0, "sym", (1,), {}))
        for symrow in (1, 0):
            tag = "h2_d%d_%s" % (d, "rows" if symrow else "hybrid")
            c.append((tag + "_n300", "h2", 300, d, None, 0, "sym", (2, 3, 4, 8),
                      dict(symrow=symrow, ldk=16 * symrow)))
            c.append((tag + "_n100", "h2", 100, d, None, 0, "sym", (2, 3), dict(symrow=symrow)))
    for symrow in (1, 0):
        tag = "h2_d200_%s" % ("rows" if symrow else "hybrid")
        c.append((tag + "_n512", "h2", 512, 200, None, 0, "sym", (2, 3), dict(symrow=symrow)))
        c.append((tag + "_n129", "h2", 129, 200, None, 0, "sym", (4,), dict(symrow=symrow)))
    c.append(("h2_full_empty_slice", "h2", 300, 200, None, 0, "full", (7,), {}))
    c.append(("h2_full_empty_past_K", "h2", 100, 200, None, 0, "full", (7,), {}))
    c.append(("h2_hybrid_n129_s8", "h2", 129, 200, None, 0, "sym", (8,), dict(symrow=0)))
    c.append(("h2_d200_full_n512", "h2", 512, 200, None, 0, "full", (2, 3), {}))
    # h2, one operand
    for d in (256, 512):
        for n in (129, 300, 512):
            c.append(("h2w_d%d_sym_n%d" % (d, n), "h2w", n, d, None, 0, "sym", (1, 2, 3),
                      dict(ldk=16 if n == 300 else 0)))
        for m, row0 in BLOCKS:
            c.append(("h2w_d%d_block_%d_%d" % (d, m, row0), "h2w", 300, d, m, row0, "full",
                      (1, 2, 3), {}))
    c.append(("h2w_full_empty_slice", "h2w", 300, 256, 44, 256, "full", (7,), {}))
    # IMQ
    for beta, order in ((-0.5, 0), (-0.5, 1), (-1.0, 0), (-1.0, 1)):
        tag = "imq_b%g_o%d" % (-beta, order)
        o = dict(imq=(beta, order))
        c.append((tag + "_f32", "f32", 300, 100, None, 0, "full", (2,), o))
        c.append((tag + "_x3_full", "x3", 300, 200, None, 0, "full", (2,), dict(o, m16=1)))
        c.append((tag + "_x3_sym", "x3", 300, 200, None, 0, "sym", (2,), dict(o, m16=1)))
        c.append((tag + "_h2_full", "h2", 300, 200, None, 0, "full", (2,), o))
        c.append((tag + "_h2_sym", "h2", 300, 200, None, 0, "sym", (2,), dict(o, symrow=1)))
    c.append(("imq_h2_tn1", "h2", 300, 20, None, 0, "full", (2,), dict(imq=(-0.5, 1))))
    c.append(("imq_h2_tn2", "h2", 300, 100, None, 0, "sym", (2,), dict(imq=(-0.5, 0))))
    c.append(("imq_h2_hybrid", "h2", 300, 200, None, 0, "sym", (3,),
              dict(imq=(-1.0, 1), symrow=0)))
    return c


CASES = _cases()
SHAPES_ND = sorted({(c[2], c[3]) for c in CASES})

# The XCD map (xmap_ok: one column block, splits | 8, 8 | row blocks x splits)
XMAP_CASES = [
    ("rows_n512_s2", "h2", 512, 200, "sym", 2, 1),
    ("rows_n300_s8", "h2", 300, 200, "sym", 8, 1),
    ("rows_n129_s4", "h2", 129, 200, "sym", 4, 1),
    ("full_n512_s2", "h2", 512, 200, "full", 2, 3),
]


def xmap_ok(ldy_cols, m, splits, tile_cols=512):
    """xmap_ok of csrc/phi.hip on the grid (ldy / tile, m_pad / 128, splits)."""
    gx, gy = ldy_cols // tile_cols, pad128(m) // 128
    return gx == 1 and splits > 1 and 8 % splits == 0 and (gy * splits) % 8 == 0
