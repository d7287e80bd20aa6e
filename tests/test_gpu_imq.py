"""GPU tests of the inverse multiquadric (IMQ) kernel k = (1 + |x-y|^2/h)^beta
through every layer: phi on the three MFMA engines, the direct (d <= 2) and
the Gauss-Seidel row kernels, Sampler (Jacobi and sequential, graphs, a kernel
lambda), the KSD (both layouts, direct, the gate), metrics.ksd, and the
refusals.  References: the reference-run fixtures tests/golden/imq_*.npz and
the fp64 restatement tests/imq_reference.py on the same fp32 inputs.

Tolerances (the project's own): phi max-normalised <= 1e-5; KSD rows, V and U
within KSD_TOL = 1e-5 of their absolute-term scales A; trajectories 1e-4
absolute (tests/test_gpu_parity.py's bounds for its RBF golden cases)."""
import functools
import math

import numpy as np
import pytest
import torch

import imq_reference as R
from conftest import record_parity
from ksd_reference import KSD_TOL, median_h64, sqdist64
from oracle import svgd_oracle as O

pytestmark = pytest.mark.gpu
PHI_TOL = 1e-5
TRAJ_TOL = 1e-4
DEV = "cuda:0"


def dsvgd():
    import dsvgd as m
    return m


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def rel_err(got, ref):
    e = float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())
    record_parity(e)
    return e


def abs_err(got, ref):
    e = float(np.abs(np.asarray(got, np.float64) - ref).max())
    record_parity(e)
    return e


def target_for(g):
    T = dsvgd().targets
    tgt = str(g["target"])
    if tgt == "gmm":
        return T.GaussianMixture1D(), O.score_gmm
    if tgt == "gaussian":
        return T.Gaussian(g["mu"], g["lam"]), (lambda X: O.score_gaussian(X, g["mu"], g["lam"]))
    x, t = g["x_train"], g["t_train"]
    return T.LogisticRegression(x, t), (lambda X: O.score_logreg(X, x, t))


@functools.lru_cache(maxsize=None)
def _problem(n, d, seed=0):
    """Particles, a Gaussian target with random diagonal precision, and its
    scores in fp32 (computed once per shape, shared and left unchanged)."""
    rs = np.random.RandomState(1000 * seed + 7 * n + d)
    X = rs.randn(n, d).astype(np.float32)
    mu = rs.randn(d).astype(np.float32)
    lam = rs.uniform(0.5, 2.0, d).astype(np.float32)
    S = O.score_gaussian(X, mu, lam).astype(np.float32)
    for a in (X, S, mu, lam):
        a.setflags(write=False)
    return X, S, mu, lam


@functools.lru_cache(maxsize=None)
def _phi_ref(n, d, h, beta, seed=0):
    X, S, _, _ = _problem(n, d, seed)
    ref = R.phi64(X, S, h, beta)
    ref.setflags(write=False)
    return ref


def engine_phi(X, S, h, beta, m=None, row0=0, **kw):
    """phi of the owned rows through the engine (fixed h, or median if None)."""
    n, d = X.shape
    eng = dsvgd().PhiEngine(n, d, m=m, row0=row0, device=DEV, kernel=dsvgd().IMQ(1.0, beta), **kw)
    eng.step(gpu(X), gpu(S), h=h)
    torch.cuda.synchronize()
    return eng.phi.cpu().numpy(), eng


# ------------------------------------------------------- phi: fixtures --
@pytest.mark.parametrize("name", ["imq_gauss_n48_d5_h1p7", "imq_gmm_n40", "imq_logreg_n60"])
def test_phi_matches_reference_run(golden, name):
    """The reference's own _phi_hat with an IMQ lambda: the MFMA path (d = 5,
    d = 3) and the direct path (the 1-D mixture)."""
    g = golden(name)
    tgt, _ = target_for(g)
    X = g["X"]
    Xg = gpu(X)
    S = torch.empty_like(Xg)
    tgt.score(Xg, S)
    phi, eng = engine_phi(X, S.cpu().numpy(), float(g["h"]), float(g["beta"]))
    assert (X.shape[1] <= eng.DIRECT_MAX_D) == (name == "imq_gmm_n40")
    assert rel_err(phi, g["phi"]) < PHI_TOL


# ------------------------------------------------ phi: fp64, per kernel --
# (n, d, m, row0): one shape per phi_mm kernel of the FmtH2 engine
SHAPES = [(129, 37, None, 0),      # the 8-wave NNX3Tile (ldy = 128), ragged
          (300, 64, None, 0),
          (384, 128, None, 0),     # the symmetric layout (ldy = 256)
          (513, 256, None, 0),     # symmetric, ldy = 512, +inf pads (one split-K slice:
                                   # the 8-wave tile)
          (1921, 256, None, 0),    # the smallest n_pad with two slices: phi_w1 DS 4, pads
          (513, 256, 256, 128)]    # a row block: phi_w1 DS 0


@pytest.mark.parametrize("median", [False, True])
@pytest.mark.parametrize("n,d,m,row0", SHAPES)
def test_phi_matches_fp64(n, d, m, row0, median):
    X, S, _, _ = _problem(n, d)
    beta = -0.5
    h = 1.3 * d
    # (a row block alone selects the median of its own m x n entries)
    kw = dict(local_median=True) if (median and m) else {}
    phi, eng = engine_phi(X, S, None if median else h, beta, m=m, row0=row0, **kw)
    assert eng.imq and eng.phi_gemm == "h2" and eng.phi_form == "xs"
    assert eng.sym == (m is None and d >= 128)      # the layout the case is for
    assert (eng.splits > 1) == (n == 1921)
    assert eng.range_guard() is False
    assert np.isfinite(phi).all()                   # (+inf pads: u^e -> 0, no NaN)
    if median:      # (the reference at the engine's own bandwidth, itself checked)
        h = eng.state.read()[1]
        if m:
            Db = sqdist64(X)[row0:row0 + m].ravel()
            h64 = float(np.partition(Db, (m * n - 1) // 2)[(m * n - 1) // 2]) / math.log(n)
        else:
            h64 = median_h64(X)
        assert abs(h - h64) <= 1e-5 * h
    ref = _phi_ref(n, d, h, beta)
    rows = slice(row0, row0 + (m or n))
    e = float(np.abs(phi - ref[rows]).max() / np.abs(ref).max())
    record_parity(e)
    assert e < PHI_TOL, e


@pytest.mark.parametrize("beta", [-1.0, -0.5, -0.25])
def test_phi_every_beta(beta):
    n, d = 300, 64
    X, S, _, _ = _problem(n, d)
    h = 1.3 * d
    phi, _ = engine_phi(X, S, h, beta)
    assert rel_err(phi, _phi_ref(n, d, h, beta)) < PHI_TOL


@pytest.mark.parametrize("gemm", ["x3", "f32"])
@pytest.mark.parametrize("n,d", [(384, 128), (129, 37)])
def test_phi_other_engines(gemm, n, d):
    X, S, _, _ = _problem(n, d)
    h = 1.3 * d
    phi, eng = engine_phi(X, S, h, -0.5, gemm=gemm)
    assert eng.phi_gemm == gemm and eng.imq
    assert rel_err(phi, _phi_ref(n, d, h, -0.5)) < PHI_TOL


def test_phi_behind_the_range_guard():
    """One particle 2^17 away (scores of the unmoved set): the FmtH2 range
    guard fires, both products run on the FmtX3 fallback and phi still meets
    the bound."""
    n, d, beta = 300, 64, -0.5
    rs = np.random.RandomState(3)
    X = (0.3 * rs.randn(n, d)).astype(np.float32)
    S = (-X / 0.09 + rs.randn(n, d)).astype(np.float32)
    X[17, 0] += np.float32(2.0 ** 17)
    h = 0.2 * d
    phi, eng = engine_phi(X, S, h, beta)
    assert eng.range_guard() is True
    assert np.isfinite(phi).all()
    assert rel_err(phi, R.phi64(X, S, h, beta)) < PHI_TOL


@pytest.mark.parametrize("image", [True, False])
def test_phi_guard_fallback_both_branches(image):
    """The same outlier on the full D layout (n = 512, ldy = 128) through the
    fallback's two branches: both products on the FmtX3 image and, with the
    image taken away, on the gated f32 phi_mm."""
    n, d, beta = 512, 64, -0.5
    rs = np.random.RandomState(3)
    X = (0.3 * rs.randn(n, d)).astype(np.float32)
    S = (-X / 0.09 + rs.randn(n, d)).astype(np.float32)
    X[17, 0] += np.float32(2.0 ** 17)
    h = 0.2 * d
    eng = dsvgd().PhiEngine(n, d, device=DEV, kernel=dsvgd().IMQ(1.0, beta))
    assert eng.phi_gemm == "h2" and not eng.sym and eng.Yx3 is not None
    if not image:
        eng.Yx3 = None
    eng.step(gpu(X), gpu(S), h=h)
    torch.cuda.synchronize()
    assert eng.range_guard() is True
    phi = eng.phi.cpu().numpy()
    assert np.isfinite(phi).all()
    assert rel_err(phi, R.phi64(X, S, h, beta)) < PHI_TOL


def test_phi_direct_d2_and_extra_step():
    """d = 2 on the direct kernel, with `extra` rows and the X update."""
    n, d, beta, h, eps = 200, 2, -0.75, 0.8, 0.05
    X, S, _, _ = _problem(n, d)
    extra = (0.01 * np.random.RandomState(1).randn(n, d)).astype(np.float32)
    eng = dsvgd().PhiEngine(n, d, device=DEV, kernel=dsvgd().IMQ("median", beta))
    Xo = gpu(X).clone()
    eng.pack(gpu(X), gpu(S))
    eng.distances()
    eng.fixed_bandwidth(h)
    eng.direction(Xo, eps, extra=gpu(extra))
    ref = R.phi64(X, S, h, beta) + extra
    assert rel_err(eng.phi.cpu().numpy(), ref) < PHI_TOL
    assert abs_err(Xo.cpu().numpy(), X + eps * ref) < 1e-6 * max(1.0, np.abs(X).max())


def test_phi_mfma_extra_step():
    """The MFMA finish adds `extra` and moves X as dsvgd_phi_finish does."""
    n, d, beta, h, eps = 129, 37, -0.5, 40.0, 0.05
    X, S, _, _ = _problem(n, d)
    extra = (0.01 * np.random.RandomState(2).randn(n, d)).astype(np.float32)
    eng = dsvgd().PhiEngine(n, d, device=DEV, kernel=dsvgd().IMQ(1.0, beta))
    Xo = gpu(X).clone()
    eng.step(gpu(X), gpu(S), X_own=Xo, step=eps, h=h, extra=gpu(extra))
    ref = _phi_ref(n, d, h, beta) + extra
    assert rel_err(eng.phi.cpu().numpy(), ref) < PHI_TOL
    assert abs_err(Xo.cpu().numpy(), X + eps * ref) < 1e-6 * max(1.0, np.abs(X).max())


# -------------------------------------------------------------- Sampler --
def _values(df, shape):
    return np.stack(df["value"].to_list()).reshape(shape)


@pytest.mark.parametrize("median", [False, True])
def test_sampler_jacobi_matches_fp64_graphs_on_and_off(median):
    n, d, T, eps, beta = 256, 8, 3, 0.05, -0.5
    _, _, mu, lam = _problem(n, d)
    m = dsvgd()
    kern = m.IMQ("median" if median else 2.5, beta)
    out = {}
    for graphs in (True, False):
        torch.manual_seed(4)
        s = m.Sampler(d, m.targets.Gaussian(mu, lam), kern)
        df = s.sample(n, T, eps, order="jacobi", device=DEV, verbose=False, graphs=graphs)
        out[graphs] = _values(df, (T + 1, n, d))
    assert out[True].tobytes() == out[False].tobytes()
    ref = R.jacobi64(out[True][0], lambda X: O.score_gaussian(X, mu, lam), 2.5, beta, T, eps,
                     median=median)
    assert abs_err(out[True], ref) < TRAJ_TOL
    assert np.abs(ref[-1] - ref[0]).max() > 100 * TRAJ_TOL


def test_sampler_sequential_matches_reference_run(golden):
    g = golden("imq_sample_gauss_n16_d3")
    tgt, _ = target_for(g)
    m = dsvgd()
    torch.manual_seed(int(g["seed"]))
    s = m.Sampler(int(g["d"]), tgt, m.IMQ(float(g["h"]), float(g["beta"])))
    df = s.sample(int(g["n"]), int(g["T"]), float(g["eps"]), device=DEV, verbose=False)
    vals = _values(df, g["values"].shape)
    np.testing.assert_array_equal(vals[0], g["values"][0])
    assert abs_err(vals, g["values"]) < TRAJ_TOL
    np.testing.assert_array_equal(df["timestep"].to_numpy(), g["timestep"])
    np.testing.assert_array_equal(df["particle"].to_numpy(), g["particle"])


@pytest.mark.parametrize("order", ["sequential", "jacobi"])
def test_sampler_imq_lambda_equals_the_instance(golden, order):
    """A reference-style IMQ lambda is probed to the same IMQ: the same bits."""
    g = golden("imq_sample_gauss_n16_d3")
    tgt, _ = target_for(g)
    m = dsvgd()
    h, beta = 1.7, -0.75
    out = []
    for kern in (m.IMQ(h, beta), lambda x, y: (1. + torch.dist(x, y, p=2) ** 2 / h) ** beta):
        torch.manual_seed(7)
        df = m.Sampler(3, tgt, kern).sample(16, 3, 0.1, order=order, device=DEV, verbose=False)
        out.append(_values(df, (4, 16, 3)))
    assert out[0].tobytes() == out[1].tobytes()
    assert np.abs(out[0][-1] - out[0][0]).max() > 0


def test_sequential_sweep_row_split_kernels():
    """n >= 2048: the sweep's rows go through dsvgd_phi_row_split_kern (the j
    range over workgroups); a few rows against the fp64 sweep."""
    from dsvgd import _native as N
    from dsvgd.engine import SelectState, sequential_sweep
    n, d, beta, h, eps = 2100, 6, -0.5, 3.0, 0.1
    assert N.load().dsvgd_phi_row_blocks(n, d) > 1
    X, S, _, _ = _problem(n, d)
    st = SelectState(DEV)
    N.call("dsvgd_set_bandwidth", st.ptr, h, N.stream(DEV))
    rows = range(5, 13)
    Xg, Sg = gpu(X), gpu(S)
    phi = torch.zeros(len(rows), d, device=DEV)
    sequential_sweep(Xg, Sg, rows, st, eps, phi_out=phi, kernel=dsvgd().IMQ(h, beta))
    ref = X.astype(np.float64)
    ref_phi = np.zeros((len(rows), d))
    for k, i in enumerate(rows):
        ref_phi[k] = R.phi64(ref, S, h, beta, rows=[i])[0]
        ref[i] += eps * ref_phi[k]
    assert rel_err(phi.cpu().numpy(), ref_phi) < PHI_TOL
    assert abs_err(Xg.cpu().numpy(), ref) < TRAJ_TOL


# ------------------------------------------------------------------ KSD --
def _ksd_run(X, S, beta, h=None, image=True, **kw):
    """image=False: the engine's FmtX3 fallback image taken away."""
    n, d = X.shape
    eng = dsvgd().PhiEngine(n, d, device=DEV, kernel=dsvgd().IMQ(1.0, beta), **kw)
    if not image:
        eng.Yx3 = None
    eng.pack(gpu(X), gpu(S))
    eng.distances(median=h is None)
    if h is None:
        eng.median_bandwidth()
    else:
        eng.fixed_bandwidth(h)
    eng.direction(step=0.0, write_phi=False)
    out, rows = eng.ksd(rows=True)
    return eng, out.cpu().numpy(), rows.cpu().numpy()


def _ksd_check(out, rows, ref):
    t, A = ref["t"], ref["A_rows"]
    ratio = np.abs(rows - t) / np.maximum(A, 1e-300)
    ev, eu = abs(out[2] - ref["V"]) / ref["A_v"], abs(out[3] - ref["U"]) / ref["A_u"]
    print("rows: worst |err| / A_i = %.3g; V %.9g ref %.9g err/A %.3g; U err/A %.3g"
          % (ratio.max(), out[2], ref["V"], ev, eu))
    assert np.isfinite(rows).all() and np.isfinite(out).all()
    assert (np.abs(rows - t) <= KSD_TOL * A).all(), ratio.max()
    assert ev <= KSD_TOL and eu <= KSD_TOL
    assert abs(out[1] - ref["diag"]) <= KSD_TOL * abs(ref["diag"])
    record_parity(max(float(ratio.max()), ev, eu))


@pytest.mark.parametrize("n,d", [(129, 37), (300, 64), (384, 128), (513, 256)])
def test_ksd_matches_fp64_both_layouts(n, d):
    X, S, _, _ = _problem(n, d)
    beta = -0.5
    eng, out, rows = _ksd_run(X, S, beta)
    assert eng.sym == (d >= 128)
    h64 = median_h64(X)
    assert abs(eng.state.read()[1] - h64) <= 1e-5 * h64
    _ksd_check(out, rows, R.ksd_reference(X, S, h64, beta))
    assert float(eng._ksd["gate"][0]) == 0.0
    # deterministic: a second evaluation gives the same bits
    out2, rows2 = eng.ksd(rows=True)
    assert out.tobytes() == out2.cpu().numpy().tobytes()
    assert rows.tobytes() == rows2.cpu().numpy().tobytes()


@pytest.mark.parametrize("gemm", ["x3", "f32"])
def test_ksd_other_engines(gemm):
    n, d, beta = 129, 37, -0.75
    X, S, _, _ = _problem(n, d)
    eng, out, rows = _ksd_run(X, S, beta, gemm=gemm)
    assert eng.phi_gemm == gemm
    _ksd_check(out, rows, R.ksd_reference(X, S, median_h64(X), beta))


def test_ksd_direct_d2_and_1d():
    X, S, _, _ = _problem(60, 2)
    eng, out, rows = _ksd_run(X, S, -0.5)
    _ksd_check(out, rows, R.ksd_reference(X, S, median_h64(X), -0.5))
    rs = np.random.RandomState(3)
    X1 = (2.5 * rs.randn(50, 1)).astype(np.float32)
    S1 = O.score_gmm(X1).astype(np.float32)
    eng, out, rows = _ksd_run(X1, S1, -1.0)
    _ksd_check(out, rows, R.ksd_reference(X1, S1, median_h64(X1), -1.0))


def test_ksd_outlier_row_trips_the_gate():
    """One particle so far out that its whole G' mass rG is below n 2^-20 (the
    IMQ's tails are heavy: 256 per coordinate at the bulk's bandwidth): the
    gate reads rG, both products rerun on the fallback engine and the
    outlier's row meets the same bound."""
    n, d, beta = 129, 37, -0.5
    X, S, _, _ = _problem(n, d, seed=4)
    h = float(np.float32(sqdist64(X).mean()))
    X = X.copy()
    X[5] += 256.0
    ref = R.ksd_reference(X, S, h, beta)
    eng, out, rows = _ksd_run(X, S, beta, h=h)
    assert float(eng._ksd["gate"][0]) == 1.0
    _ksd_check(out, rows, ref)


def test_ksd_gate_without_an_x3_image():
    """The gate's other branch on the same outlier: with the FmtX3 image
    taken away both products rerun on the gated f32 phi_mm."""
    n, d, beta = 129, 37, -0.5
    X, S, _, _ = _problem(n, d, seed=4)
    h = float(np.float32(sqdist64(X).mean()))
    X = X.copy()
    X[5] += 256.0
    eng, out, rows = _ksd_run(X, S, beta, h=h, image=False)
    assert not eng.sym and float(eng._ksd["gate"][0]) == 1.0
    _ksd_check(out, rows, R.ksd_reference(X, S, h, beta))


def test_metrics_ksd_equals_engine_path():
    from dsvgd import metrics
    m = dsvgd()
    n, d, beta = 300, 64, -0.5
    X, S, mu, lam = _problem(n, d)
    target = m.targets.Gaussian(mu, lam)
    Xg = gpu(X)
    Sg = torch.empty_like(Xg)
    target.score(Xg, Sg)
    Sn = Sg.cpu().numpy()
    eng, out, _ = _ksd_run(X, Sn, beta)
    assert metrics.ksd(Xg, target, m.IMQ("median", beta), squared=True) == out[2]
    assert metrics.ksd(Xg, Sg, m.IMQ("median", beta)) == math.sqrt(max(out[2], 0.0))
    assert metrics.ksd(X, target, m.IMQ("median", beta), statistic="u", squared=True,
                       device=DEV) == out[3]
    eng2, out2, _ = _ksd_run(X, Sn, -0.75, h=2.5 * d)
    assert metrics.ksd(Xg, target, lambda x, y: (1 + torch.dist(x, y) ** 2 / (2.5 * d)) ** -0.75,
                       squared=True) == out2[2]
    # another kernel is another number
    assert metrics.ksd(Xg, target, m.RBF("median"), squared=True) != out[2]


def _frame(df, l):
    return np.stack(df[df.timestep == l].sort_values("particle")["value"].to_list())


@pytest.mark.parametrize("order,n,d", [("jacobi", 256, 8), ("sequential", 64, 8),
                                       ("jacobi", 64, 1)])
def test_sampler_ksd_every(order, n, d):
    """The records match fp64 at each recorded timestep's particles and
    bandwidth, and the particles are those of the run without them, bit for
    bit."""
    m = dsvgd()
    beta = -0.5
    if d == 1:
        target, score = m.targets.GaussianMixture1D(), O.score_gmm
    else:
        _, _, mu, lam = _problem(n, d)
        target, score = m.targets.Gaussian(mu, lam), (lambda X: O.score_gaussian(X, mu, lam))
    kw = dict(num_iter=4, step_size=0.05, order=order, device=DEV, verbose=False)
    s = m.Sampler(d, target, m.IMQ("median", beta))
    torch.manual_seed(11)
    df = s.sample(n, ksd_every=2, **kw)
    diag = s.diagnostics
    assert list(diag.timestep) == [0, 2, 4]
    worst = 0.0
    for _, row in diag.iterrows():
        X = _frame(df, int(row.timestep)).astype(np.float32)
        Xg = gpu(X)
        Sg = torch.empty_like(Xg)
        target.score(Xg, Sg)
        ref = R.ksd_reference(X, Sg.cpu().numpy(), float(row.h), beta)
        ev = abs(row.ksd2_v - ref["V"]) / ref["A_v"]
        eu = abs(row.ksd2_u - ref["U"]) / ref["A_u"]
        print("timestep %d: V %.9g ref %.9g err/A %.3g, U err/A %.3g"
              % (row.timestep, row.ksd2_v, ref["V"], ev, eu))
        assert ev <= KSD_TOL and eu <= KSD_TOL
        assert row.ksd == math.sqrt(max(row.ksd2_v, 0.0))
        worst = max(worst, ev, eu)
    record_parity(worst)
    s0 = m.Sampler(d, target, m.IMQ("median", beta))
    torch.manual_seed(11)
    df0 = s0.sample(n, **kw)
    assert s0.diagnostics is None
    assert (df.timestep.values == df0.timestep.values).all()
    va, vb = np.stack(df["value"].to_list()), np.stack(df0["value"].to_list())
    assert va.tobytes() == vb.tobytes()


# ------------------------------------------------------------- refusals --
def test_refusals_and_resolved_form():
    m = dsvgd()
    tgt = m.targets.Gaussian([0, 0], [1, 1])
    with pytest.raises(ValueError, match="RBF-only"):
        m.DistSampler(0, 1, tgt, m.IMQ(1.0), torch.zeros(8, 2), 1, 1, False, False, False,
                      device=DEV)
    # phi_form="w" is an RBF form: an IMQ engine keeps the two-operand one
    eng = m.PhiEngine(512, 256, device=DEV, phi_form="w", kernel=m.IMQ())
    assert eng.phi_form == "xs" and eng.imq
    assert m.PhiEngine(512, 256, device=DEV, phi_form="w").phi_form == "w"
    with pytest.raises(ValueError, match="pair_split"):
        m.PhiEngine(4096, 256, m=2048, row0=0, device=DEV, pair_split=(0, 2), kernel=m.IMQ())
