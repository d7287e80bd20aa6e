"""The dsvgd_phi_mm* entry points and their finish kernels called directly, in
one process, at n <= 512 with the split-K slice count forced (the engine
never takes more than one slice below n ~ 1921).  Reference, case tables,
slice ranges and bounds: tests/phi_mm_reference.py (pinned on the host by
tests/test_phi_mm_host.py).

A. Every entry point into NaN-filled, oversized buffers: every split-K slice
   against the fp64 product of the engine's own D and Y over exactly the
   K-steps that slice takes, then the sum (KY_TOL / RS_TOL, max-normalised);
   everything outside the grant still NaN; (slice, row block) pairs without a
   K-step exact zeros.  Before the GPU result is looked at each case shows in
   fp64 that its inputs would notice a K-step taken 16 columns away, a slice
   boundary moved by one K-step and a kept diagonal entry in the ragged tile.
   Then the XCD map (same bits with and without), the gates, determinism and
   the refusals (NativeError, buffers untouched).
B. dsvgd_phi_finish / _finish_w / _finish_imq on synthetic buffers against
   the formula in the comment above each kernel, in fp64, within the derived
   bound (splits + 8) 2^-24 A.
C. Product (three forced slices) + finish against the fp64 oracle, PHI_TOL.

What each case reaches (csrc/phi.hip line of the launch; W: one operand):

  entry  layout  ldy (d)           splits  kernel / template form           line
  f32    full    128 / 256 / 512   any     nn_kernel<TN, true, 2, 2, 32>    1171 (IMQ 1166)
  x3     any     128 (20)          any     nn_x3_kernel<1, false, .., X3>   286
  x3     any     256, 512, m16=1   any     nn_x3_kernel<TN, true, true, true>   291
  x3     any     256, 512, m16=0   any     nn_x3_kernel<TN, true, true, false>  295
  h2     full    128               any     nn_x3_kernel<1, false, .., H2, 2>    334
  h2     any     256 (100)         any     nn_x3_kernel<2, true, .., H2, 3>     334
  h2     sym     512, 1024         1       nn_x3_kernel<4, true, .., H2, 3>     334
  h2     full    512, 1024         any     phi_w1_kernel<0>                 330
  h2     sym     512, 1024         >= 2    phi_w1_kernel<4>   (symrow 1)    304
  h2     sym     512, 1024         >= 2    phi_w1_kernel<1> + <2> (symrow 0)    321, 325
  h2w    full    dp 256, 512       any     phi_w1_kernel<0, 2, true>        434
  h2w    sym     dp 256, 512       any     phi_w1_kernel<4, 2, true>        429
"""
import numpy as np
import pytest
import torch

import imq_reference as IR
import phi_mm_reference as R
from conftest import record_parity
from oracle import svgd_oracle as O
from test_gpu_pairsplit_kernels import DEV, all_nan, dsvgd, gpu, nan_buf, native, same_bits, stream
from test_gpu_split import KY_TOL, PHI_TOL

pytestmark = pytest.mark.gpu
assert (R.KY_TOL, R.PHI_TOL, R.RS_TOL) == (KY_TOL, PHI_TOL, 1e-6)


class _Ops(object):
    """An engine after one direction() -- D, Y, the images, the scales and
    the bandwidth on the device -- with D and Y in fp64 on the host."""


_ops = {}


def operands(entry, n, d, m, row0, layout):
    gemm = "h2" if entry == "h2w" else entry
    key = (gemm, entry == "h2w", n, d, m, row0, layout)
    if key in _ops:
        return _ops[key]
    X, S = R.inputs(n, d)
    mm = n if m is None else m
    eng = dsvgd().PhiEngine(n, d, m=mm, row0=row0, device=DEV, gemm=gemm,
                            sym_layout=layout == "sym", phi_form="w" if entry == "h2w" else None)
    assert eng.sym == (layout == "sym") and eng.phi_gemm == gemm
    assert eng.phi_form == ("w" if entry == "h2w" else "xs")
    assert (eng.dp, eng.ldy, eng.n_pad) == (R.dp_of(d), R.ldy_of(R.dp_of(d)), R.pad128(n))
    eng.pack(gpu(X), gpu(S))
    eng.distances(median=False)
    eng.fixed_bandwidth(R.bandwidth(n, d))
    eng.direction(gpu(X[row0:row0 + mm]).clone(), 0.0)
    torch.cuda.synchronize()
    if gemm == "h2":
        assert eng.range_guard() is False
    E = _Ops()
    E.eng, E.entry, E.n, E.m, E.row0 = eng, entry, n, mm, row0
    E.D = eng.dense_D(padded=True).double().cpu().numpy()
    assert np.isinf(E.D[mm:]).all() and np.isinf(E.D[:, n:]).all()
    assert np.isfinite(E.D[:mm, :n]).all()
    E.Y = eng.Y[:eng.n_pad].double().cpu().numpy()
    assert (E.Y[n:] == 0).all()
    _, E.h, E.inv_h = eng.state.read()
    E.B = R.w_operand(E.Y, eng.dp, E.inv_h) if entry == "h2w" else E.Y
    E.width = eng.dp if entry == "h2w" else eng.ldy
    E.kmat, E.refs, E.img = {}, {}, {}
    _ops[key] = E
    return E


def kmats(E, pw):
    if pw not in E.kmat:
        E.kmat[pw] = (R.kernel_matrix(E.D, E.inv_h, E.row0, pw),
                      R.kernel_matrix(E.D, E.inv_h, E.row0, pw, zero_diag=False))
        off = E.kmat[pw][0][:E.m, :E.n]
        off = off[off > 0]
        if pw is None:   # the fixture's conditions, on the engine's own D
            assert off.min() > 1e-6 and off.max() / off.min() >= 100.0
    return E.kmat[pw]


def x3_image(E, m16):
    """The FmtX3 image of the engine's Y: unswizzled for the 16x16x32 form,
    swizzled for the 32x32x16 one (the engine holds only the one it runs)."""
    if m16 not in E.img:
        N, eng = native(), E.eng
        img = torch.empty(N.load().dsvgd_ysplit_bytes(eng.n_pad, eng.ldy) // 2, dtype=torch.int16,
                          device=DEV)
        N.call("dsvgd_ysplit", N.ptr(eng.Y), eng.ldy, eng.n_pad, N.ptr(img), 0 if m16 else 1, None,
               stream())
        E.img[m16] = img
    return E.img[m16]


def kern_of(opts):
    N = native()
    if "imq" in opts:
        return N.Kernel(N.KERNEL_IMQ, opts["imq"][0]), opts["imq"][1]
    return N.Kernel(N.KERNEL_RBF, 0.0), 0


def launch(E, splits, KY, ldk, RS, sym, opts, gate=None, plain=False, **over):
    """One call of E's entry point.  over: D, ldd, image, row0, m, n replace
    the engine's (for the refusals); plain: the entry point without `_kern`."""
    N, eng = native(), E.eng
    kern, order = kern_of(opts)
    order = over.get("order", order)
    D = over.get("D", N.ptr(eng.D))
    ldd = over.get("ldd", eng.n_pad)
    mid = (over.get("row0", eng.row0), over.get("m", eng.m), over.get("n", eng.n), eng.state.ptr,
           splits, N.ptr(KY), ldk, N.ptr(RS))
    s = stream()
    if E.entry == "f32":
        Y = over.get("image", N.ptr(eng.Y))
        if plain and gate is None:
            N.call("dsvgd_phi_mm", D, ldd, Y, eng.ldy, *mid, s)
        elif plain:
            N.call("dsvgd_phi_mm_gated", D, ldd, Y, eng.ldy, *mid, gate, s)
        else:
            N.call("dsvgd_phi_mm_kern", D, ldd, Y, eng.ldy, *mid, gate, kern, order, s)
    elif E.entry == "x3":
        m16 = opts["m16"]
        img = over.get("image", N.ptr(x3_image(E, 0 if eng.ldy == 128 else m16)))
        if plain:
            N.call("dsvgd_phi_mm_x3", D, ldd, img, eng.ldy, *mid, sym, m16, gate, s)
        else:
            N.call("dsvgd_phi_mm_x3_kern", D, ldd, img, eng.ldy, *mid, sym, m16, gate, kern, order,
                   s)
    elif E.entry == "h2":
        img = over.get("image", N.ptr(eng.Yx))
        colinv = N.ptr(eng.yscale) + 4 * eng.ldy
        if plain:
            N.call("dsvgd_phi_mm_h2", D, ldd, img, eng.ldy, *mid, sym, colinv, gate, s)
        else:
            N.call("dsvgd_phi_mm_h2_kern", D, ldd, img, eng.ldy, *mid, sym, colinv, gate, kern,
                   order, s)
    else:
        img = over.get("image", N.ptr(eng.Wh))
        N.call("dsvgd_phi_mm_h2w", D, ldd, img, eng.dp, *mid, sym, N.ptr(eng.wscale) + 4 * eng.dp,
               gate, s)


def buffers(E, splits, ldk):
    """NaN-filled KY / rowsum, oversized as the pair-split test's: three extra
    rows, 64 floats of slack after the row sums."""
    return nan_buf(splits * E.m + 3, ldk), nan_buf(splits * E.eng.m_pad + 64)


def run(E, splits, sym, opts, gate=None, plain=False):
    """The entry point under the case's symrow form; returns the raw buffers."""
    ldk = E.width + opts.get("ldk", 0)
    KY, RS = buffers(E, splits, ldk)
    lib = native().load()
    prev = lib.dsvgd_phi_set_symrow(opts.get("symrow", 1))
    try:
        launch(E, splits, KY, ldk, RS, sym, opts, gate, plain)
    finally:
        lib.dsvgd_phi_set_symrow(prev)
    torch.cuda.synchronize()
    return KY, RS


def granted(E, splits, KY, RS):
    """(splits, m, width) / (splits, m) views after checking that nothing
    outside the grant was written; rows [m, m_pad) of the row sums inside the
    grant are not constrained."""
    m, mp = E.m, E.eng.m_pad
    assert all_nan(KY[splits * m:]) and all_nan(KY[:, E.width:])
    assert all_nan(RS[splits * mp:])
    return (KY[:splits * m].view(splits, m, KY.shape[1])[:, :, :E.width],
            RS[:splits * mp].view(splits, mp)[:, :m])


def check_case(E, splits, layout, opts):
    sym = int(layout == "sym")
    eng = E.eng
    form = R.form_of(E.entry, eng.ldy, sym, splits, opts.get("symrow", 1))
    pw = None if "imq" not in opts else opts["imq"][0] - opts["imq"][1]
    Km, Kf = kmats(E, pw)
    # the inputs would notice each defect this check is for (fp64)
    sens = R.sensitivity(Km, Kf, E.B, form, splits, E.m, E.row0)
    assert R.noticed(sens), sens
    if (form, splits, pw) not in E.refs:
        E.refs[form, splits, pw] = R.slice_refs(Km, E.B, form, splits, E.m)
    refs, (P_all, r_all) = E.refs[form, splits, pw]
    KY, RS = granted(E, splits, *run(E, splits, sym, opts))
    KY, RS = KY.double().cpu().numpy(), RS.double().cpu().numpy()
    worst, worst_r = 0.0, 0.0
    K = eng.n_pad
    for z in range(splits):
        for rb in range(eng.m_pad // 128):
            if len(R.slice_ksteps(form, K, splits, z, rb)) == 0:
                rows = slice(128 * rb, min(E.m, 128 * (rb + 1)))
                assert (KY[z, rows] == 0).all() and (RS[z, rows] == 0).all(), ("empty", z, rb)
        e, e_r = R.max_err(KY[z], refs[z][0]), R.max_err(RS[z], refs[z][1])
        print("%s splits %d slice %d: KY %.3g rowsum %.3g" % (form, splits, z, e, e_r))
        worst, worst_r = max(worst, e), max(worst_r, e_r)
        assert e < KY_TOL, ("slice", z, e)
        assert e_r < R.RS_TOL, ("slice", z, e_r)
    e, e_r = R.max_err(KY.sum(0), P_all), R.max_err(RS.sum(0), r_all)
    assert e < KY_TOL, ("sum", e)
    assert e_r < R.RS_TOL, ("sum", e_r)
    return max(worst, e), max(worst_r, e_r)


# ------------------------------------------------ A. slice by slice --
@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_slices_match_fp64(case):
    name, entry, n, d, m, row0, layout, splits_list, opts = case
    E = operands(entry, n, d, m, row0, layout)
    worst, worst_r = 0.0, 0.0
    for splits in splits_list:
        e, e_r = check_case(E, splits, layout, opts)
        worst, worst_r = max(worst, e), max(worst_r, e_r)
    record_parity(worst / KY_TOL, ky=worst, rowsum=worst_r, entry=entry)


@pytest.mark.parametrize("case", R.XMAP_CASES, ids=[c[0] for c in R.XMAP_CASES])
def test_xcd_map_gives_identical_bits(case):
    """A grid xmap_ok holds for, with the map's bit set and cleared: the same
    blocks' arithmetic on other workgroups, so the same bits."""
    name, entry, n, d, layout, splits, mask = case
    E = operands(entry, n, d, None, 0, layout)
    assert R.xmap_ok(E.eng.ldy, n, splits)
    bit = 1 if layout == "sym" else 2
    assert mask & bit
    lib = native().load()
    out = {}
    for on in (mask, mask & ~bit):
        prev = lib.dsvgd_phi_set_xmap(on)
        try:
            out[on] = granted(E, splits, *run(E, splits, int(layout == "sym"), {}))
        finally:
            lib.dsvgd_phi_set_xmap(prev)
    a, b = out[mask], out[mask & ~bit]
    assert not bool(torch.isnan(a[0]).any()) and not bool(torch.isnan(a[1]).any())
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


# (entry, d, layout, opts, the gate word with which the kernel must not run)
GATES = [("f32", 100, "full", {}, 0.0), ("x3", 200, "sym", dict(m16=1), 0.0),
         ("h2", 200, "sym", dict(symrow=1), 1.0), ("h2", 200, "full", {}, 1.0),
         ("h2", 100, "sym", {}, 1.0), ("h2w", 256, "sym", {}, 1.0)]


@pytest.mark.parametrize("entry,d,layout,opts,closed", GATES,
                         ids=["%s_%s_%d" % (g[0], g[2], g[1]) for g in GATES])
def test_gate_and_determinism(entry, d, layout, opts, closed):
    """Two ungated runs give the same bits; with the gate word at the other
    polarity the same bits again; with it set against the kernel nothing is
    written.  f32 / x3 / h2 also through the entry points without `_kern`."""
    E = operands(entry, 300, d, None, 0, layout)
    sym, splits = int(layout == "sym"), 2
    def live(RS):
        return RS[:splits * E.eng.m_pad].view(splits, -1)[:, :E.m]
    first = run(E, splits, sym, opts)
    granted(E, splits, *first)
    assert not bool(torch.isnan(first[0][:splits * E.m, :E.width]).any())
    assert not bool(torch.isnan(live(first[1])).any())
    again = run(E, splits, sym, opts)
    assert same_bits(first[0], again[0]) and same_bits(live(first[1]), live(again[1]))
    for plain in (False, True) if entry != "h2w" else (False,):
        for word in (closed, 1.0 - closed):
            g = gpu(np.array([word]))
            if entry == "f32" and plain and word != closed:
                KY, RS = run(E, splits, sym, opts, None, True)       # dsvgd_phi_mm itself
                assert same_bits(KY, first[0]) and same_bits(live(RS), live(first[1]))
            KY, RS = run(E, splits, sym, opts, native().ptr(g), plain)
            if word == closed:
                assert all_nan(KY) and all_nan(RS)
            else:
                assert same_bits(KY, first[0]) and same_bits(live(RS), live(first[1]))


def test_refusals_launch_nothing():
    """Every refused call raises NativeError and leaves the buffers NaN."""
    N = native()
    lib = N.load()
    assert lib.dsvgd_phi_set_symrow(1) == 1
    H = operands("h2", 300, 200, None, 0, "sym")
    Hf = operands("h2", 300, 200, None, 0, "full")
    Hb = operands("h2", 300, 200, 70, 37, "full")
    H1 = operands("h2", 300, 20, None, 0, "full")
    H100 = operands("h2", 100, 200, None, 0, "sym")
    X1 = operands("x3", 300, 20, None, 0, "full")
    Xb = operands("x3", 300, 200, 70, 37, "full")
    F = operands("f32", 300, 100, None, 0, "full")
    W = operands("h2w", 300, 256, None, 0, "sym")
    Wb = operands("h2w", 300, 256, 70, 37, "full")
    x3o = dict(m16=0)
    refused = [
        (H, 2, 1, {}, dict(ldd=512), "ldd must equal"),
        (F, 2, 0, {}, dict(ldd=512), "ldd must equal"),
        (Hb, 2, 1, {}, {}, "sym:"),
        (Xb, 2, 1, dict(m16=1), {}, "sym:"),
        (Wb, 2, 1, {}, {}, "sym:"),
        (X1, 2, 1, x3o, {}, "symmetric layout needs ldy % 256"),
        (H1, 2, 1, {}, {}, "ldy % 256 == 0"),
        (X1, 2, 0, dict(m16=1), {}, "16x16 form"),
        (Hf, 2, 0, {}, dict(order=1), "order"),
        (F, 2, 0, {}, dict(order=1), "order"),
        (X1, 2, 0, x3o, dict(order=1), "order"),
        (Hf, 0, 0, {}, {}, "splits"),
        (Hf, 1025, 0, {}, {}, "splits"),
        (F, 0, 0, {}, {}, "splits"),
        (W, 1025, 1, {}, {}, "splits"),
        (X1, 1025, 0, x3o, {}, "splits"),
        (Hf, 2, 0, {}, dict(image=N.ptr(Hf.eng.Yx) + 4), "alignment"),
        (F, 2, 0, {}, dict(image=N.ptr(F.eng.Y) + 4), "alignment"),
        (X1, 2, 0, x3o, dict(image=N.ptr(x3_image(X1, 0)) + 4), "alignment"),
        (W, 2, 1, {}, dict(image=N.ptr(W.eng.Wh) + 4), "alignment"),
        # a row block that would end in the pads: rows [256, 384) of n = 300
        (Hf, 2, 0, {}, dict(row0=256, m=128), "row block outside"),
        # the one-launch symmetric walk takes no empty slice (include/dsvgd.h)
        (H, 7, 1, {}, {}, "empty split-K slice"),
        (H100, 7, 1, {}, {}, "empty split-K slice"),
        (H100, 5, 1, {}, {}, "empty split-K slice"),
        (W, 7, 1, {}, {}, "empty split-K slice"),
    ]
    for E, splits, sym, opts, over, text in refused:
        ldk = E.width + 16
        KY, RS = nan_buf(8 * E.m + 3, ldk), nan_buf(8 * E.eng.m_pad + 64)
        with pytest.raises(N.NativeError, match=text):
            launch(E, splits, KY, ldk, RS, sym, opts, **over)
        torch.cuda.synchronize()
        assert all_nan(KY) and all_nan(RS), (E.entry, splits, text)


# --------------------------------------------- B. the finish kernels --
def _state(h):
    N = native()
    st = dsvgd().engine.SelectState(torch.device(DEV))
    N.call("dsvgd_set_bandwidth", st.ptr, float(h), stream())
    torch.cuda.synchronize()
    return st


def _finish_outputs(a, shape):
    """phi (NaN, two extra rows) and X (NaN in the gap; one float off
    16-byte alignment on the "xalign" path)."""
    _, m, _, _, d, _, want_phi, want_x, path = shape
    phi = nan_buf(m + 2, a["ldphi"])
    if path == "xalign":
        base = nan_buf(m * a["ldx"] + 8)
        X = base[1:1 + m * a["ldx"]].view(m, a["ldx"])
        assert X.data_ptr() % 16 == 4
    else:
        X = nan_buf(m, a["ldx"])
        assert X.data_ptr() % 16 == 0
    X[:, :d] = gpu(a["X0"][:, :d])
    return phi, X


def _check_finish(a, shape, p64, A, splits, phi, X):
    _, m, _, _, d, _, want_phi, want_x, _ = shape
    worst = 0.0
    if want_phi:
        assert all_nan(phi[m:]) and all_nan(phi[:, d:])
        err = np.abs(phi[:m, :d].double().cpu().numpy() - p64)
        bound = R.finish_bound(A, splits)
        worst = float((err / bound).max())
        assert (err <= bound).all(), worst
    else:
        assert all_nan(phi)
    assert all_nan(X[:, d:])
    x0 = a["X0"][:, :d].astype(np.float64)
    got = X[:, :d].double().cpu().numpy()
    if want_x:
        step = float(a["step"])
        err = np.abs(got - (x0 + step * p64))
        mb = R.move_bound(A, splits, step, x0, p64)
        worst = max(worst, float((err / mb).max()))
        assert (err <= mb).all()
    else:
        assert (got == x0).all()
    return worst


def _gap_nan(t, width):
    t = gpu(t)
    t[..., width:] = float("nan")
    return t


@pytest.mark.parametrize("shape", R.FINISH_SHAPES, ids=[s[0] for s in R.FINISH_SHAPES])
def test_finish_matches_formula(shape):
    """dsvgd_phi_finish: phi = inv_n ((s + KS) + (2/h)(r xc - KXc)) (+ extra)."""
    N = native()
    _, m, row0, splits, d, _, want_phi, want_x, _ = shape
    a = R.finish_inputs(shape, "xs")
    st = _state(a["h"])
    a["inv_h"] = np.float32(st.read()[2])
    p64, A = R.finish_ref("xs", a)
    phi, X = _finish_outputs(a, shape)
    ex = None if a["extra"] is None else _gap_nan(a["extra"], d)
    KY, RS, Y = gpu(a["KY"]), gpu(a["RS"]), gpu(a["Y"])
    N.call("dsvgd_phi_finish", N.ptr(KY), a["ldk"], N.ptr(RS), splits,
           N.ptr(Y), a["ldy"], row0, m, d, a["dp"], st.ptr, float(a["inv_n"]),
           float(a["step"]), N.ptr(ex), a["lde"], N.ptr(phi) if want_phi else None, a["ldphi"],
           N.ptr(X) if want_x else None, a["ldx"], stream())
    torch.cuda.synchronize()
    record_parity(_check_finish(a, shape, p64, A, splits, phi, X))


@pytest.mark.parametrize("mode", ["guard0", "guard1", "one_buffer"])
@pytest.mark.parametrize("shape", R.FINISH_SHAPES, ids=[s[0] for s in R.FINISH_SHAPES])
def test_finish_w_matches_formula(shape, mode):
    """dsvgd_phi_finish_w: the guard word 0 -- phi = inv_n ((s + KW) + (2/h) r
    xc) on `splits` slices at row stride ldk >= dp; nonzero -- dsvgd_phi_finish's
    formula on splits + 1 two-operand slices; and KW and KY in one buffer."""
    N = native()
    _, m, row0, splits, d, _, want_phi, want_x, _ = shape
    a = R.finish_inputs(shape, "w")
    st = _state(a["h"])
    a["inv_h"] = np.float32(st.read()[2])
    fb = splits + 1
    if mode == "guard1":
        p64, A = R.finish_ref("xs", dict(a, KY=a["KYfb"], RS=a["RSfb"]))
        ns = fb
    else:
        p64, A = R.finish_ref("w", a)
        ns = splits
    KY = gpu(a["KYfb"])
    if mode == "one_buffer":      # as the engine: K . W at row stride ldkw in KY's buffer
        assert KY.numel() >= splits * m * a["ldkw"]
        KY.view(-1)[:splits * m * a["ldkw"]] = gpu(a["KW"]).view(-1)
        KW = KY
    else:
        KW = gpu(a["KW"])
    guard = gpu(np.array([1.0 if mode == "guard1" else 0.0]))
    phi, X = _finish_outputs(a, shape)
    ex = None if a["extra"] is None else _gap_nan(a["extra"], d)
    RS, Y = gpu(a["RSfb"]), gpu(a["Y"])
    N.call("dsvgd_phi_finish_w", N.ptr(KW), a["ldkw"], N.ptr(RS), splits, N.ptr(KY),
           a["ldk"], fb, N.ptr(Y), a["ldy"], row0, m, d, a["dp"], st.ptr, N.ptr(guard),
           float(a["inv_n"]), float(a["step"]), N.ptr(ex), a["lde"],
           N.ptr(phi) if want_phi else None, a["ldphi"], N.ptr(X) if want_x else None, a["ldx"],
           stream())
    torch.cuda.synchronize()
    record_parity(_check_finish(a, shape, p64, A, ns, phi, X))


@pytest.mark.parametrize("beta", [-0.5, -1.0])
@pytest.mark.parametrize("shape", R.FINISH_SHAPES, ids=[s[0] for s in R.FINISH_SHAPES])
def test_finish_imq_matches_formula(shape, beta):
    """dsvgd_phi_finish_imq: phi = inv_n ((s + FS) + c1 (rG xc - G'Xc)), c1 =
    -2 beta / h; KF and KG with different leading dimensions."""
    N = native()
    _, m, row0, splits, d, _, want_phi, want_x, _ = shape
    a = R.finish_inputs(shape, "imq")
    a["beta"] = np.float32(beta)
    st = _state(a["h"])
    a["inv_h"] = np.float32(st.read()[2])
    p64, A = R.finish_ref("imq", a)
    phi, X = _finish_outputs(a, shape)
    ex = None if a["extra"] is None else _gap_nan(a["extra"], d)
    KF, KG, RS, Y = gpu(a["KF"]), gpu(a["KG"]), gpu(a["RS"]), gpu(a["Y"])
    N.call("dsvgd_phi_finish_imq", N.ptr(KF), a["ldk"], N.ptr(KG),
           a["ldk"] + 4, N.ptr(RS), splits, N.ptr(Y), a["ldy"], row0, m, d,
           a["dp"], st.ptr, N.Kernel(N.KERNEL_IMQ, beta), float(a["inv_n"]), float(a["step"]),
           N.ptr(ex), a["lde"], N.ptr(phi) if want_phi else None, a["ldphi"],
           N.ptr(X) if want_x else None, a["ldx"], stream())
    torch.cuda.synchronize()
    record_parity(_check_finish(a, shape, p64, A, splits, phi, X))


# ------------------------------------- C. product + finish, every row --
COMPOSED = [("f32", 100, "full", {}), ("x3", 200, "sym", dict(m16=1)),
            ("h2", 200, "sym", dict(symrow=1)), ("h2", 200, "sym", dict(symrow=0)),
            ("h2w", 256, "sym", {}), ("h2", 200, "sym", dict(symrow=1, imq=-0.5))]


@pytest.mark.parametrize("entry,d,layout,opts", COMPOSED,
                         ids=["f32", "x3_sym", "h2_rows", "h2_hybrid", "h2w_sym", "h2_imq"])
def test_product_and_finish_match_oracle(entry, d, layout, opts):
    """n = 300 in three forced slices, then the entry point's own finish: phi
    of every row within PHI_TOL of the fp64 oracle (the IMQ: tests/imq_reference.py)."""
    N = native()
    n, splits = 300, 3
    E = operands(entry, n, d, None, 0, layout)
    eng, sym = E.eng, int(layout == "sym")
    X, S = R.inputs(n, d)
    phi = nan_buf(n, d)
    common = (N.ptr(eng.Y), eng.ldy, 0, n, d, eng.dp, eng.state.ptr)
    tail = (1.0 / n, 0.0, None, d, N.ptr(phi), d, None, d, stream())
    if "imq" in opts:
        beta = opts["imq"]
        KF, RF = run(E, splits, sym, dict(opts, imq=(beta, 0)))
        KG, RG = run(E, splits, sym, dict(opts, imq=(beta, 1)))
        N.call("dsvgd_phi_finish_imq", N.ptr(KF), eng.ldy, N.ptr(KG), eng.ldy, N.ptr(RG), splits,
               *common, N.Kernel(N.KERNEL_IMQ, beta), *tail)
        ref = IR.phi64(X, S, E.h, beta)
    else:
        KY, RS = run(E, splits, sym, opts)
        if entry == "h2w":
            guard = N.ptr(eng.wscale) + 4 * (2 * eng.dp + 2)
            N.call("dsvgd_phi_finish_w", N.ptr(KY), eng.dp, N.ptr(RS), splits, N.ptr(KY), eng.ldy,
                   1, *common, guard, *tail)
        else:
            N.call("dsvgd_phi_finish", N.ptr(KY), eng.ldy, N.ptr(RS), splits, *common, *tail)
        ref = O.phi(X, S, E.h)
    torch.cuda.synchronize()
    e = float(np.abs(phi.cpu().numpy() - ref).max() / np.abs(ref).max())
    record_parity(e)
    assert e < PHI_TOL, e
