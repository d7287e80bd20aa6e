"""phi_mm in the one-operand form: K . W with W = S - (2/h) Xc
instead of K . [Xc | S], on PhiEngine(..., phi_form="w").

Checked here: (1) the W image and its scales (dsvgd_h2_wscales /
dsvgd_h2_wsplit) against numpy, (2) the raw product and the row sums against
the fp64 K @ W of the engine's own D, (3) phi against the fp64 oracle, (4)
the range guard -- off on ordinary and bench-like inputs, on for the outlier
cases, where the step is bit for bit the FmtX3 phi_mm -- and (5) when the
form engages.  Tolerances are the ones of test_gpu_split.py / test_gpu_range.py.
"""
import numpy as np
import pytest
import torch

from conftest import record_parity
from oracle import svgd_oracle as O
from test_gpu_range import CASES, ROW_TOL, _outlier_case, _phi, row_err
from test_gpu_split import KY_TOL, PHI_TOL, _pow2_scale, decode_h2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (n, d, m, row0): one partial block; padded columns; symmetric + bracketed
# with n_pad = 4224 (a half-empty last 256-row block); four column blocks; a
# row block at a multiple of 128 but not of 256; m and row0 off every tile
SHAPES = [(300, 256, None, 0), (512, 225, None, 0), (4200, 256, None, 0),
          (2048, 1024, None, 0), (4096, 256, 1024, 1152), (4096, 256, 1000, 1000)]
H_FIXED = {256: 60.0, 225: 55.0, 1024: 250.0}


def dsvgd():
    import dsvgd as m
    return m


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


_data, _refs = {}, {}


def _inputs(n, d):
    if (n, d) not in _data:
        rs = np.random.RandomState(n + d)
        X = rs.randn(n, d).astype(np.float32)
        _data[n, d] = (X, (-X + 0.3 * rs.randn(n, d)).astype(np.float32))
    return _data[n, d]


def _oracle_phi(n, d, m, row0, h):
    """The fp64 phi of the shape's inputs at bandwidth h (computed once)."""
    key = (n, d, m, row0, float(h))
    if key not in _refs:
        X, S = _inputs(n, d)
        rows = None if m is None else np.arange(row0, row0 + m)
        _refs[key] = O.phi(X, S, h) if rows is None else O.phi(X, S, h, rows=rows)
    return _refs[key]


def _w_engine(n, d, m, row0, h):
    """A "w" engine after pack, distances and the bandwidth (no direction yet)."""
    X, S = _inputs(n, d)
    # (a row block's median: the lower median of its own m x n entries)
    eng = dsvgd().PhiEngine(n, d, m=m, row0=row0, device=DEV, phi_form="w",
                            local_median=m is not None and h is None)
    assert eng.phi_form == "w"
    eng.pack(gpu(X), gpu(S))
    eng.distances(median=h is None)
    if h is None:
        eng.median_bandwidth()
    else:
        eng.fixed_bandwidth(h)
    return eng


# ------------------------------------------------------------- 1. image --
@pytest.mark.parametrize("n", [300, 2048])
@pytest.mark.parametrize("d", [225, 1024])
def test_wsplit_image_and_scales(n, d):
    """dsvgd_h2_wscales + dsvgd_h2_wsplit: power-of-two scales with s_c b_c in
    [2^14, 2^15) for b_c = max|S_c| + t max|Xc_c|; (v0 + v1) / s_c reproduces
    fmaf(-t, xc, s) within dsvgd_h2_ysplit's two-part bound (2^-22 relative
    inside the 2^-16 window of the scale's reference magnitude -- b_c here --
    and 2^-22 relative + 2^-38 of it everywhere); padding rows and columns zero."""
    from dsvgd import _native as N
    X, S = _inputs(n, d)
    eng = dsvgd().PhiEngine(n, d, device=DEV, phi_form="w")
    assert eng.phi_form == "w"
    dp, n_pad, ldy = eng.dp, eng.n_pad, eng.ldy
    eng.pack(gpu(X), gpu(S))
    eng.fixed_bandwidth(H_FIXED[d])
    s = N.stream(torch.device(DEV))
    N.call("dsvgd_h2_wscales", N.ptr(eng.colmax), N.ptr(eng.gmax), eng.colmax_nb, ldy, dp,
           eng.state.ptr, N.ptr(eng.wscale), s)
    N.call("dsvgd_h2_wsplit", N.ptr(eng.Y), ldy, n_pad, dp, eng.state.ptr, N.ptr(eng.wscale),
           N.ptr(eng.Wh), s)
    torch.cuda.synchronize()
    t = np.float64(np.float32(2.0) * np.float32(eng.state.read()[2]))
    Y = eng.Y.cpu().numpy()[:n_pad].astype(np.float64)
    # one rounding of the exact s - t xc (the product of two floats is exact in fp64)
    W = (Y[:, dp:2 * dp] - t * Y[:, :dp]).astype(np.float32).astype(np.float64)
    b = (np.abs(Y[:, dp:2 * dp]).max(0) + t * np.abs(Y[:, :dp]).max(0)).astype(np.float32)
    b = b.astype(np.float64)
    scale = eng.wscale.cpu().numpy().astype(np.float64)
    s_c = scale[:dp]
    live = b > 0
    assert np.all(np.log2(s_c) == np.round(np.log2(s_c)))
    assert np.all((s_c * b)[live] >= 2.0 ** 14) and np.all((s_c * b)[live] < 2.0 ** 15)
    assert np.all(s_c[~live] == 1.0) and np.all(scale[dp:2 * dp] * s_c == 1.0)
    np.testing.assert_array_equal(s_c, _pow2_scale(b))
    assert scale[2 * dp + 2] == 0.0          # ordinary inputs: the guard is off
    parts = decode_h2(eng.Wh, n_pad, dp)
    rec = parts.sum(0) / s_c[None, :]
    assert np.all(rec[n:] == 0.0) and np.all(rec[:, d:] == 0.0)
    big = (np.abs(W) >= b[None, :] * 2.0 ** -16) & (W != 0)
    err = np.abs(rec - W)[big] / np.abs(W)[big]
    record_parity(float(err.max()))
    assert err.max() <= 2.0 ** -22
    assert np.all(np.abs(rec - W) <= 2.0 ** -22 * np.abs(W) + 2.0 ** -38 * b[None, :])


# ------------------------------------------------------- 2. raw product --
@pytest.mark.parametrize("n,d,m,row0", SHAPES)
def test_kw_and_rowsums_match_fp64(n, d, m, row0):
    """KW and the row sums of a "w" engine against the fp64 K @ W of the
    engine's own D (diagonal left out), max-normalised as _ky_errors."""
    h = None if m is None else H_FIXED[d]
    eng = _w_engine(n, d, m, row0, h)
    Xo = gpu(_inputs(n, d)[0][row0:row0 + eng.m]).clone()
    eng.direction(Xo, 0.0)
    torch.cuda.synchronize()
    assert eng.range_guard() is False
    assert eng.sym == (m is None)
    if n >= 2048:
        assert eng.splits >= 2
    dp = eng.dp
    KW = eng.KY.view(-1)[:eng.splits * eng.m * dp].view(eng.splits, eng.m, dp)
    KW = KW.double().sum(0).cpu().numpy()
    r = eng.rowsum[:eng.splits * eng.m_pad].view(eng.splits, eng.m_pad)[:, :eng.m]
    r = r.double().sum(0).cpu().numpy()
    _, hx, inv_h = eng.state.read()
    K = torch.exp(-eng.dense_D().double() / hx)
    rows = torch.arange(eng.m, device=DEV)
    K[rows, rows + row0] = 0.0
    Y = eng.Y[:n].double()
    t = float(np.float32(2.0) * np.float32(inv_h))
    W = Y[:, dp:2 * dp] - t * Y[:, :dp]
    KW64, r64 = (K @ W).cpu().numpy(), K.sum(1).cpu().numpy()
    e = float(np.abs(KW - KW64).max() / np.abs(KW64).max())
    e_r = float(np.abs(r - r64).max() / np.abs(r64).max())
    record_parity(e, rowsum=e_r, splits=int(eng.splits))
    assert e < KY_TOL, e
    assert e_r < 1e-6, e_r


# ------------------------------------------------------ 3. phi vs oracle --
@pytest.mark.parametrize("median", [True, False])
@pytest.mark.parametrize("n,d,m,row0", SHAPES)
def test_phi_matches_oracle(n, d, m, row0, median):
    """phi of the "w" engine within PHI_TOL of the fp64 oracle (max-normalised),
    with the median and with a fixed bandwidth; then the same direction with
    step > 0, `extra` and write_phi=False: eng.phi untouched and the moved
    rows exactly step * (phi + extra) (X_own starts at zero: no rounding)."""
    eng = _w_engine(n, d, m, row0, None if median else H_FIXED[d])
    mm = eng.m
    Xo = gpu(_inputs(n, d)[0][row0:row0 + mm]).clone()
    X0 = Xo.clone()
    eng.direction(Xo, 0.0)
    torch.cuda.synchronize()
    assert eng.range_guard() is False
    assert torch.equal(Xo, X0)
    ref = _oracle_phi(n, d, m, row0, eng.state.read()[1])
    phi = eng.phi.clone()
    e = float(np.abs(phi.cpu().numpy() - ref).max() / np.abs(ref).max())
    record_parity(e)
    assert e < PHI_TOL, e
    extra = gpu(np.random.RandomState(1).randn(mm, d))
    Xz = torch.zeros(mm, d, device=DEV)
    eng.phi.fill_(7.0)
    eng.direction(Xz, 0.5, write_phi=False, extra=extra)
    torch.cuda.synchronize()
    assert bool((eng.phi == 7.0).all())
    assert torch.equal(Xz, 0.5 * (phi + extra))


# ------------------------------------------------------------- 4. guard --
@pytest.mark.parametrize("n,d", [(4096, 256)])
def test_guard_off_for_ordinary_particles_w(n, d):
    rs = np.random.RandomState(n)
    X = rs.randn(n, d).astype(np.float32)
    S = (-X + 0.3 * rs.randn(n, d)).astype(np.float32)
    _, _, eng = _phi(X, S, phi_form="w")
    assert eng.phi_form == "w" and eng.range_guard() is False


def test_guard_off_for_bench_like_inputs():
    """The benchmark's inputs at n = 4096: particles 0.1 N(0,1), logreg scores
    (data N(0, 1/p), labels from a random w + logistic noise).  A guard that
    fired here would silently run the two-operand fallback at the headline."""
    n, d, Nd = 4096, 256, 4096
    p = d - 1
    rs = np.random.RandomState(0)
    xd = rs.randn(Nd, p).astype(np.float32) / np.sqrt(p)
    z = xd @ np.random.RandomState(1).randn(p) + np.random.RandomState(2).logistic(size=Nd)
    t = np.where(z > 0, 1.0, -1.0).astype(np.float32)
    gen = torch.Generator(device="cpu").manual_seed(0)
    X = (0.1 * torch.randn(n, d, generator=gen)).to(DEV)
    S = torch.empty_like(X)
    dsvgd().targets.LogisticRegression(xd, t).score(X, S)
    eng = dsvgd().PhiEngine(n, d, device=DEV, phi_form="w")
    eng.step(X, S, X_own=X.clone(), step=0.0, h=None)
    torch.cuda.synchronize()
    assert eng.phi_form == "w" and eng.range_guard() is False
    ref = O.phi(X.cpu().numpy(), S.cpu().numpy(), eng.state.read()[1])
    e = float(np.abs(eng.phi.cpu().numpy() - ref).max() / np.abs(ref).max())
    record_parity(e)
    assert e < PHI_TOL, e


@pytest.mark.parametrize("kind,k", CASES)
def test_outlier_rows_and_guard_fallback(kind, k):
    """test_gpu_range.py's outlier cases through phi_form="w": every row within
    ROW_TOL of fp64, row-normalised; for k >= 20 the guard is on and KY and
    the row sums are bit for bit the FmtX3 engine's on the same D."""
    X, S = _outlier_case(4096, 256, kind, k)
    phi, h, eng = _phi(X, S, phi_form="w")
    assert eng.phi_form == "w"
    e = row_err(phi, O.phi(X, S, h))
    guard = eng.range_guard()
    record_parity(float(e.max()), kind=kind, k=k, guard=guard)
    assert e.max() <= ROW_TOL, (e.max(), int(e.argmax()))
    if k >= 20:
        assert guard is True
        _, _, eng3 = _phi(X, S, phi_gemm="x3", gram_gemm="h2")
        assert eng3.phi_gemm == "x3" and eng3.splits == eng.splits_fb
        torch.testing.assert_close(eng.dense_D(), eng3.dense_D(), rtol=0, atol=0)
        nk, nr = eng3.KY.numel(), eng3.rowsum.numel()
        assert torch.equal(eng.KY.view(-1)[:nk], eng3.KY.view(-1))
        assert torch.equal(eng.rowsum[:nr], eng3.rowsum)


@pytest.mark.parametrize("image", [True, False])
def test_guard_fallback_of_a_row_block(image):
    """The guard's two fallback branches at a small shape: a row block (the
    full D layout) of a "w" engine with one score row 2^20 larger, on the
    FmtX3 image and, with the image taken away, on the gated f32 phi_mm
    (both with the fallback's own slice count): every row within ROW_TOL."""
    n, d, m, row0 = 512, 256, 256, 128
    X, S = _outlier_case(n, d, "score", 20)
    eng = dsvgd().PhiEngine(n, d, m=m, row0=row0, device=DEV, phi_form="w")
    assert eng.phi_form == "w" and not eng.sym and eng.Yx3 is not None
    if not image:
        eng.Yx3 = None
    h = 2.0 * d * 0.09
    eng.step(gpu(X), gpu(S), X_own=gpu(X[row0:row0 + m]).clone(), step=0.0, h=h)
    torch.cuda.synchronize()
    assert eng.range_guard() is True
    e = row_err(eng.phi.cpu().numpy(), O.phi(X, S, h, rows=np.arange(row0, row0 + m)))
    record_parity(float(e.max()), image=image)
    assert e.max() <= ROW_TOL, (e.max(), int(e.argmax()))


# -------------------------------------------------------- 5. engagement --
def test_form_engages_only_where_it_applies():
    E = dsvgd().PhiEngine
    assert E(640, 64, device=DEV, phi_form="w").phi_form == "xs"        # dp % 256 != 0
    assert E(640, 256, device=DEV).phi_form == "xs"                    # the default
    assert E(640, 256, device=DEV, phi_form="w", phi_gemm="x3").phi_form == "xs"
    eng = E(640, 256, device=DEV, phi_form="w")
    assert eng.phi_form == "w" and not hasattr(eng, "Yx")
    with pytest.raises(ValueError):
        E(640, 256, device=DEV, phi_form="ws")
    X, S = _inputs(640, 256)
    eng.step(gpu(X), gpu(S), step=0.0, h=None)
    with pytest.raises(ValueError):
        eng.ksd()


def test_distsampler_graph_replay_same_bits_as_eager():
    """A DistSampler at S = 1 holds a "w" engine; three Jacobi steps replayed
    from the captured graph give the bits of three steps launched eagerly
    (a StageTimer set: the step then launches its kernels itself)."""
    from dsvgd.engine import StageTimer
    n, d, Nd = 4200, 256, 512
    rs = np.random.RandomState(5)
    xd = (rs.randn(Nd, d - 1) / np.sqrt(d - 1)).astype(np.float32)
    t = np.where(rs.randn(Nd) > 0, 1.0, -1.0).astype(np.float32)
    X0 = (0.1 * rs.randn(n, d)).astype(np.float32)
    out = []
    for eager in (False, True):
        smp = dsvgd().DistSampler(0, 1, dsvgd().targets.LogisticRegression(xd, t),
                                  dsvgd().RBF("median"), gpu(X0).clone(), Nd, Nd,
                                  exchange_particles=True, exchange_scores=True,
                                  include_wasserstein=False, order="jacobi")
        if eager:
            smp.timer = StageTimer(only={"phi_mm"})
        for _ in range(3):
            smp.make_step(1e-2)
        torch.cuda.synchronize()
        eng = smp._engines[next(iter(smp._engines))]
        assert eng.phi_form == "w" and eng.sym and eng.range_guard() is False
        if not eager:
            assert smp._graph is not None and smp._graph.graph is not None
        out.append(smp.particles.detach().clone())
    assert bool(torch.isfinite(out[0]).all()) and not torch.equal(out[0], gpu(X0))
    assert torch.equal(out[0], out[1])
