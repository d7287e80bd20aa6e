"""tests/phi_mm_reference.py pinned without a GPU: the dispatch table, the
K-steps of every split-K slice of every form against a restatement of the
kernels' own loops, the fixture's conditions per (n, d), the three defects a
slice-by-slice check must notice -- shown in fp64 for every case of the GPU
test -- and the finish kernels' derived bound against a float32 restatement
of their order."""
import numpy as np
import pytest

import phi_mm_reference as R

KS_ = (128, 256, 384, 512)
SPLITS = (1, 2, 3, 4, 5, 7, 8)


# ------------------------------------------------------------ dispatch --
@pytest.mark.parametrize("d,ldy,tn", [(20, 128, 1), (64, 128, 1), (65, 256, 2), (100, 256, 2),
                                      (128, 256, 2), (129, 512, 4), (200, 512, 4), (256, 512, 4),
                                      (300, 1024, 4), (512, 1024, 4)])
def test_dispatch_of_d(d, ldy, tn):
    assert R.ldy_of(R.dp_of(d)) == ldy and R.tn_of(ldy) == tn


def test_w_form_widths():
    assert R.dp_of(256) % 256 == 0 and R.dp_of(512) % 256 == 0 and R.dp_of(300) % 256 != 0


def test_form_of():
    assert R.form_of("f32", 256, 0, 3) == "c32"
    assert R.form_of("x3", 512, 1, 3) == "c16"
    assert R.form_of("h2", 512, 1, 1) == "c16"           # the 8-wave tile
    assert R.form_of("h2", 256, 1, 3) == "c16"           # TN 2
    assert R.form_of("h2", 512, 0, 3) == "c16"           # DS 0
    assert R.form_of("h2", 1024, 1, 2, symrow=1) == "rows"
    assert R.form_of("h2", 512, 1, 2, symrow=0) == "hybrid"
    assert R.form_of("h2w", 256, 1, 1) == "rows" and R.form_of("h2w", 256, 0, 2) == "c16"


# ------------------------------------------ the kernels' loops, restated --
def walk_nn(K, splits, z, BJ):
    """nn_kernel / nn_x3_kernel with NNTile::run / NNX3Tile::run: k0 = z kchunk,
    k1 = min(K, k0 + kchunk), `if (k0 >= k1) return`, j0 = k0, k0 + BJ, ..."""
    kchunk = (((K + splits - 1) // splits) + BJ - 1) // BJ * BJ
    k0 = z * kchunk
    k1 = min(K, k0 + kchunk)
    out = []
    j0 = k0
    while j0 < k1:
        out += [j0 // 16 + t for t in range(BJ // 16)]
        j0 += BJ
    return out


def walk_w1(DS, K, Z, bz, rb, kchunk):
    """phi_w1_kernel's K-steps in walk order (csrc/phi_w1.hpp: kb0, kend, ks0,
    nsteps, kdir, the DS 1 / DS 2 overrides, DS 4's ksp and two phases)."""
    i0 = 128 * rb
    kb0 = bz * kchunk
    kend = min(K, kb0 + kchunk)
    ks0 = kb0 // 16
    nsteps = (kend - kb0) // 16 if kend > kb0 else 0
    kdir = -Z if DS == 2 else Z if DS == 1 else 1
    if DS == 2:
        T = (K - i0) // 16
        ks0 = K // 16 - 1 - bz
        nsteps = (T - bz + Z - 1) // Z if T > bz else 0
    elif DS == 1:
        T = i0 // 16
        ks0 = bz
        nsteps = (T - bz + Z - 1) // Z if T > bz else 0
    if DS == 4:
        ksp = min(max(kb0, i0), kend) // 16
        return ([ks0 + k for k in range(max(0, ksp - ks0))]
                + [ksp + k for k in range(max(0, ks0 + nsteps - ksp))])
    return [ks0 + kdir * k for k in range(max(0, nsteps))]


def walk(form, K, splits, z, rb):
    kc = R.kchunk_of(K, splits)
    if form == "c32":
        return walk_nn(K, splits, z, 32)
    if form == "c16":
        a = walk_nn(K, splits, z, 16)
        assert a == walk_w1(0, K, splits, z, rb, kc)      # DS 0 takes the same ones
        return a
    if form == "rows":
        return walk_w1(4, K, splits, z, rb, kc)
    sl = splits // 2
    if z < sl:
        return walk_w1(1, K, sl, z, rb, kc)
    return walk_w1(2, K, splits - sl, z - sl, rb, kc)


@pytest.mark.parametrize("form", ["c32", "c16", "rows", "hybrid"])
def test_slice_ksteps_match_the_kernels_walk(form):
    """slice_ksteps is the set the kernel's loop visits, each K-step once;
    over the slices every K-step of every row block is taken exactly once."""
    n_checked = 0
    for K in KS_:
        for splits in SPLITS:
            if form == "hybrid" and splits < 2:
                continue
            if form == "rows" and R.has_empty_slice(K, splits):
                continue                                  # refused by the entry point
            for rb in range(K // 128):
                seen = np.zeros(K // 16, np.int64)
                for z in range(splits):
                    w = walk(form, K, splits, z, rb)
                    assert len(set(w)) == len(w) and all(0 <= q < K // 16 for q in w)
                    assert sorted(w) == list(R.slice_ksteps(form, K, splits, z, rb)), \
                        (K, splits, z, rb)
                    seen[w] += 1
                    n_checked += 1
                assert (seen == 1).all(), (K, splits, rb)
            nrb = K // 128
            total = sum(R.slice_weights(form, K, splits, z, nrb) for z in range(splits))
            assert (total == 1).all()
    assert n_checked > 100


def test_slice_ranges_stated_in_the_issue():
    assert R.kchunk_of(512, 3, 16) == 176 and R.kchunk_of(512, 3, 32) == 192
    assert R.kchunk_of(384, 2) == 192                     # a boundary inside tile 1
    assert list(R.slice_ksteps("c32", 512, 3, 2)) == list(range(24, 32))
    assert R.has_empty_slice(384, 7) and R.has_empty_slice(384, 5, 32)
    assert not R.has_empty_slice(384, 5) and not R.has_empty_slice(384, 8)
    # the hybrid at K = 384, splits = 3: sl = 1; row block 2's diagonal tile
    # starts at K-step 16
    assert list(R.slice_ksteps("hybrid", 384, 3, 0, 2)) == list(range(16))
    assert list(R.slice_ksteps("hybrid", 384, 3, 1, 2)) == [17, 19, 21, 23]
    assert list(R.slice_ksteps("hybrid", 384, 3, 2, 2)) == [16, 18, 20, 22]
    for z in range(4):                                    # row block 0: nothing transposed
        assert len(R.slice_ksteps("hybrid", 512, 8, z, 0)) == 0


def test_one_launch_walk_steps_past_K_on_an_empty_slice():
    """Why dsvgd_phi_mm_h2 / _h2w refuse an empty slice in the one-launch
    symmetric form: with kb0 > K the restated walk of phi_w1_kernel DS 4 has a
    plain phase of (kb0 - K) / 16 K-steps from K on -- past D's panel row and
    the image.  kb0 == K walks nothing; every other form walks nothing on any
    empty slice."""
    K, splits = 128, 7
    kc = R.kchunk_of(K, splits)
    assert kc == 32 and R.has_empty_slice(K, splits)
    assert walk_w1(4, K, splits, 4, 0, kc) == []
    assert walk_w1(4, K, splits, 5, 0, kc) == [8, 9]
    assert walk_w1(4, K, splits, 6, 0, kc) == [8, 9, 10, 11]
    for z in (4, 5, 6):
        assert walk_w1(0, K, splits, z, 0, kc) == [] and walk_nn(K, splits, z, 16) == []
        assert walk_nn(K, splits, z, 32) == []


# -------------------------------------------------------------- fixture --
@pytest.mark.parametrize("n,d", R.SHAPES_ND)
def test_fixture_conditions(n, d):
    """The off-diagonal weights stay above 1e-6 and span two decades."""
    w = R.fixture_weights(n, d)
    assert w.min() > 1e-6 and w.max() / w.min() >= 100.0, (w.min(), w.max())


def test_fixture_inputs_are_stable():
    X, S = R.inputs(300, 100)
    assert X.dtype == np.float32 and S.shape == (300, 100)
    assert R.inputs(300, 100)[0] is X
    D, Y, inv_h = R.host_operands(300, 100, 44, 256)
    assert D.shape == (128, 384) and Y.shape == (384, 256)
    assert np.isinf(D[44:]).all() and np.isinf(D[:, 300:]).all() and np.isfinite(D[:44, :300]).all()
    assert (Y[300:] == 0).all() and (Y[:, 100:128] == 0).all() and (Y[:, 228:] == 0).all()
    assert abs(D[3, 259]) < 1e-9                          # the block's own diagonal


# --------------------------------------------------------- sensitivity --
_ops = {}


def operands(n, d, m, row0):
    if (n, d, m, row0) not in _ops:
        _ops[n, d, m, row0] = R.host_operands(n, d, m, row0)
    return _ops[n, d, m, row0]


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_inputs_notice_each_defect(case):
    """Per case and slice count, in fp64 on host-built operands: a K-step
    taken 16 columns away, a slice boundary moved by one K-step and a kept
    diagonal entry in the ragged tile each move the slice's product by more
    than 100 KY_TOL and its row sums by more than 100 RS_TOL."""
    name, entry, n, d, m, row0, layout, splits_list, opts = case
    D, Y, inv_h = operands(n, d, m, row0)
    m = n if m is None else m
    dp = R.dp_of(d)
    ldy = R.ldy_of(dp)
    pw = None if "imq" not in opts else opts["imq"][0] - opts["imq"][1]
    Km = R.kernel_matrix(D, inv_h, row0, pw)
    Kf = R.kernel_matrix(D, inv_h, row0, pw, zero_diag=False)
    assert Kf[m - 1, row0 + m - 1] == pytest.approx(1.0, abs=1e-9)
    assert (Km[m:] == 0).all() and (Km[:, n:] == 0).all()
    B = R.w_operand(Y, dp, inv_h) if entry == "h2w" else Y
    for splits in splits_list:
        form = R.form_of(entry, ldy, layout == "sym", splits, opts.get("symrow", 1))
        sens = R.sensitivity(Km, Kf, B, form, splits, m, row0)
        assert R.noticed(sens), (splits, form, sens)


def test_defects_are_what_they_say():
    w = R.slice_weights("c16", 384, 2, 0, 3)
    assert w.sum() == 3 * 12 and (w[:, :12] == 1).all()
    s = R.defect_shift(w)
    assert (s[:, 0] == 0).all() and (s[:, 1] == 2).all() and s.sum() == w.sum()
    b = R.defect_boundary("c16", 384, 2, 3)
    assert (b - w)[:, 12].tolist() == [1, 1, 1] and (b - w).sum() == 3
    b1 = R.defect_boundary("c16", 384, 1, 3)
    assert (b1[:, 0] == 0).all() and (b1[:, 1:] == 1).all()
    bh = R.defect_boundary("hybrid", 384, 4, 3) - R.slice_weights("hybrid", 384, 4, 0, 3)
    assert bh[0].nonzero()[0].tolist() == [0] and bh[1].nonzero()[0].tolist() == [8]
    assert bh[2].nonzero()[0].tolist() == [16]


def test_every_form_has_a_boundary_inside_a_tile_and_pads():
    """Per entry point and slice form: one case whose slice boundary is no
    multiple of 128 and one whose K range ends in pads."""
    seen = {}
    for name, entry, n, d, m, row0, layout, splits_list, opts in R.CASES:
        ldy = R.ldy_of(R.dp_of(d))
        K = R.pad128(n)
        for splits in splits_list:
            form = R.form_of(entry, ldy, layout == "sym", splits, opts.get("symrow", 1))
            if splits == 1:
                continue
            s = seen.setdefault((entry, form), set())
            if form == "hybrid" or R.kchunk_of(K, splits, 32 if form == "c32" else 16) % 128:
                s.add("inside")
            if K > n:
                s.add("pads")
    assert set(seen) == {("f32", "c32"), ("x3", "c16"), ("h2", "c16"), ("h2", "rows"),
                         ("h2", "hybrid"), ("h2w", "c16"), ("h2w", "rows")}
    assert all(v == {"inside", "pads"} for v in seen.values()), seen


def test_xmap_cases_meet_xmap_ok():
    for name, entry, n, d, layout, splits, mask in R.XMAP_CASES:
        assert R.xmap_ok(R.ldy_of(R.dp_of(d)), n, splits), name
    assert not R.xmap_ok(1024, 512, 2) and not R.xmap_ok(512, 300, 2)
    assert not R.xmap_ok(512, 512, 3)


# ------------------------------------------------------- finish bounds --
@pytest.mark.parametrize("kind", ["xs", "w", "imq"])
@pytest.mark.parametrize("shape", R.FINISH_SHAPES, ids=[s[0] for s in R.FINISH_SHAPES])
def test_finish_bound_holds_for_the_float32_order(shape, kind):
    """The float32 restatement of the kernel's order stays within the derived
    bound of the fp64 formula, for phi and for the moved X."""
    for beta in ((-0.5, -1.0) if kind == "imq" else (-0.5,)):
        a = R.finish_inputs(shape, kind)
        a["beta"] = np.float32(beta)
        p64, A = R.finish_ref(kind, a)
        p32 = R.finish_f32(kind, a).astype(np.float64)
        bound = R.finish_bound(A, a["splits"])
        assert (np.abs(p32 - p64) <= bound).all(), float((np.abs(p32 - p64) / bound).max())
        # not vacuous: the rounding reaches a hundredth of the bound somewhere
        assert (np.abs(p32 - p64) / bound).max() > 0.01
        d = a["d"]
        x0 = a["X0"][:, :d]
        x32 = (x0 + a["step"] * R.finish_f32(kind, a)).astype(np.float64)
        want = x0.astype(np.float64) + float(a["step"]) * p64
        mb = R.move_bound(A, a["splits"], float(a["step"]), x0.astype(np.float64), p64)
        assert (np.abs(x32 - want) <= mb).all()


def test_finish_ref_is_the_documented_formula():
    """One element by hand, for each kind."""
    a = R.finish_inputs(R.FINISH_SHAPES[0], "xs")
    i, c, dp, row0 = 5, 17, a["dp"], a["row0"]
    f = np.float64
    two = 2.0 * f(a["inv_h"])
    r = a["RS"][:, i].astype(f).sum()
    yx, ys = f(a["Y"][row0 + i, c]), f(a["Y"][row0 + i, dp + c])
    kx = a["KY"][:, i, c].astype(f).sum()
    ks = a["KY"][:, i, dp + c].astype(f).sum()
    ex = f(a["extra"][i, c])
    inv_n = f(a["inv_n"])
    assert R.finish_ref("xs", a)[0][i, c] == pytest.approx(
        inv_n * (ys + ks + two * (r * yx - kx)) + ex, rel=1e-13)
    kw = a["KW"][:, i, c].astype(f).sum()
    assert R.finish_ref("w", a)[0][i, c] == pytest.approx(
        inv_n * (ys + kw + two * r * yx) + ex, rel=1e-13)
    gx = a["KG"][:, i, c].astype(f).sum()
    c1 = -2.0 * f(a["beta"]) * f(a["inv_h"])
    assert R.finish_ref("imq", a)[0][i, c] == pytest.approx(
        inv_n * (ys + ks + c1 * (r * yx - gx)) + ex, rel=1e-13)
