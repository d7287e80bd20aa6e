"""GPU tests of the KSD diagnostic (csrc/ksd.hip, PhiEngine.ksd, metrics.ksd,
Sampler.sample(ksd_every=...)) against the fp64 closed form on the same fp32
inputs (tests/ksd_reference.py).

Tolerance: KSD^2 can cancel without its rounding error shrinking, so errors
are measured against the sums of the absolute values of the Stein kernel's
terms: |rows_i - t_i| <= 1e-5 A_i, |V - V_ref| <= 1e-5 A_v, |U - U_ref| <=
1e-5 A_u (ksd_reference.py; 1e-5 is the project's phi bound).  An fp32 numpy
emulation of the decomposition gives 2-3e-7 per row on these shapes."""
import math

import numpy as np
import pytest
import torch

from conftest import record_parity
from ksd_reference import KSD_TOL, ksd_reference, median_h64, sqdist64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _problem(n, d, offcentre=False, seed=0):
    """Particles and a Gaussian target with random diagonal precision."""
    import dsvgd
    rs = np.random.RandomState(1000 * seed + 7 * n + d)
    X = rs.randn(n, d).astype(np.float32)
    if offcentre:
        X = (1.5 * X + 3.0).astype(np.float32)
    mu = rs.randn(d).astype(np.float32)
    lam = rs.uniform(0.5, 2.0, d).astype(np.float32)
    return X, dsvgd.targets.Gaussian(mu, lam)


def _scores(X, target):
    Xg = torch.tensor(X, device=DEV)
    Sg = torch.empty_like(Xg)
    target.score(Xg, Sg)
    return Xg, Sg


def _run(Xg, Sg, h=None, m=None, row0=0, image=True, **kw):
    """One engine evaluation; h=None: the median bandwidth; image=False: the
    engine's FmtX3 fallback image taken away."""
    import dsvgd
    n, d = Xg.shape
    eng = dsvgd.PhiEngine(n, d, m=m, row0=row0, device=DEV, **kw)
    if not image:
        eng.Yx3 = None
    eng.pack(Xg, Sg)
    eng.distances(median=h is None)
    if h is None:
        eng.median_bandwidth()
    else:
        eng.fixed_bandwidth(h)
    eng.direction(step=0.0, write_phi=False)
    out, rows = eng.ksd(rows=True)
    return eng, out.cpu().numpy(), rows.cpu().numpy()


def _check(out, rows, ref, sl=None):
    """The issue's bounds; returns the worst error / scale ratio."""
    t, A = ref["t"], ref["A_rows"]
    if sl is not None:
        t, A = t[sl], A[sl]
    print("rows: worst |err| / A_i = %.3g" % (np.abs(rows - t) / A).max() if A.size and A.min() > 0
          else "rows: (no off-diagonal terms)")
    assert np.isfinite(rows).all()
    assert (np.abs(rows - t) <= KSD_TOL * A).all(), (np.abs(rows - t) / np.maximum(A, 1e-300)).max()
    worst = float((np.abs(rows - t) / np.maximum(A, 1e-300)).max()) if A.max() > 0 else 0.0
    if sl is None:
        ev, eu = abs(out[2] - ref["V"]) / ref["A_v"], abs(out[3] - ref["U"]) / ref["A_u"]
        print("V %.9g ref %.9g err/A %.3g; U %.9g ref %.9g err/A %.3g"
              % (out[2], ref["V"], ev, out[3], ref["U"], eu))
        assert np.isfinite(out).all()
        assert ev <= KSD_TOL and eu <= KSD_TOL
        assert abs(out[1] - ref["diag"]) <= KSD_TOL * ref["diag"]
        worst = max(worst, ev, eu)
    record_parity(worst)
    return worst


SHAPES = [(2, 3), (129, 37), (300, 64), (384, 128), (513, 256)]


@pytest.mark.parametrize("offcentre", [False, True])
@pytest.mark.parametrize("n,d", SHAPES)
def test_ksd_matches_fp64_median_bandwidth(n, d, offcentre):
    X, target = _problem(n, d, offcentre)
    Xg, Sg = _scores(X, target)
    eng, out, rows = _run(Xg, Sg)
    assert eng.sym == ((n, d) in ((384, 128), (513, 256)))   # the layout the case is for
    assert np.isfinite(out).all() and np.isfinite(rows).all()   # (+inf pads: exp(-inf) inf)
    h64 = median_h64(X)
    _, h, _ = eng.state.read()
    assert abs(h - h64) <= 1e-5 * h64
    _check(out, rows, ksd_reference(X, Sg.cpu().numpy(), h64))


def test_ksd_single_particle():
    X, target = _problem(1, 3)
    Xg, Sg = _scores(X, target)
    eng, out, rows = _run(Xg, Sg)
    s = Sg.cpu().numpy().astype(np.float64)[0]
    v = float(s @ s) + 2 * 3 / 1.0      # h = 1 (median 0)
    assert out[0] == 0.0 and rows[0] == 0.0
    assert abs(out[2] - v) <= 1e-12 * v and abs(out[1] - v) <= 1e-12 * v
    assert math.isnan(out[3])


@pytest.mark.parametrize("n,d", [(300, 64), (384, 128)])
def test_ksd_fixed_bandwidth_offdiagonal_dominates(n, d):
    X, target = _problem(n, d, seed=1)
    Xg, Sg = _scores(X, target)
    h = float(np.float32(sqdist64(X).mean()))
    ref = ksd_reference(X, Sg.cpu().numpy(), h)
    assert ref["off"] > ref["diag"]     # otherwise the case shows nothing about the sweep
    eng, out, rows = _run(Xg, Sg, h=h)
    _check(out, rows, ref)


def test_ksd_outlier_row_below_the_fp16_image_of_k():
    """One particle far from the rest: its kernel values (~1e-9) sit where
    the FmtH2 image of K keeps a few bits only, so the engine reruns phi_mm
    behind dsvgd_ksd_gate and the outlier's row meets the same bound."""
    n, d = 129, 37
    X, target = _problem(n, d, seed=4)
    X[5] += 8.0
    Xg, Sg = _scores(X, target)
    h = float(np.float32(sqdist64(X).mean()))
    ref = ksd_reference(X, Sg.cpu().numpy(), h)
    eng, out, rows = _run(Xg, Sg, h=h)
    assert float(eng._ksd["gate"][0]) == 1.0
    _check(out, rows, ref)
    # an ordinary particle set leaves the gate closed
    X2, _ = _problem(n, d, seed=4)
    eng2, _, _ = _run(*_scores(X2, target))
    assert float(eng2._ksd["gate"][0]) == 0.0


def test_ksd_gate_without_an_x3_image():
    """The gate's other branch on the same outlier: with the FmtX3 image
    taken away phi_mm reruns on the gated f32 engine."""
    n, d = 129, 37
    X, target = _problem(n, d, seed=4)
    X[5] += 8.0
    Xg, Sg = _scores(X, target)
    h = float(np.float32(sqdist64(X).mean()))
    eng, out, rows = _run(Xg, Sg, h=h, image=False)
    assert not eng.sym and float(eng._ksd["gate"][0]) == 1.0
    _check(out, rows, ksd_reference(X, Sg.cpu().numpy(), h))


def test_ksd_direct_gmm_1d():
    import dsvgd
    rs = np.random.RandomState(3)
    X = (2.5 * rs.randn(50, 1)).astype(np.float32)
    Xg, Sg = _scores(X, dsvgd.targets.GaussianMixture1D())
    eng, out, rows = _run(Xg, Sg)
    _check(out, rows, ksd_reference(X, Sg.cpu().numpy(), median_h64(X)))


def test_ksd_direct_d2():
    X, target = _problem(3, 2)
    Xg, Sg = _scores(X, target)
    eng, out, rows = _run(Xg, Sg)
    _check(out, rows, ksd_reference(X, Sg.cpu().numpy(), median_h64(X)))


@pytest.mark.parametrize("m,row0", [(256, 128), (70, 37), (200, 313)])
def test_ksd_row_block(m, row0):
    """The full-layout walk's row-block geometry: a tile-aligned block; one
    ragged tile whose diagonal falls inside a 4-column vector load and across
    a panel edge (the upper 64 rows mostly invalid); a block that ends at row
    n, so its diagonal panels are also those with the +inf pads, its second
    tile ragged."""
    n, d = 513, 64
    X, target = _problem(n, d)
    Xg, Sg = _scores(X, target)
    h = float(np.float32(median_h64(X)))
    ref = ksd_reference(X, Sg.cpu().numpy(), h)
    eng, out, rows = _run(Xg, Sg, h=h, m=m, row0=row0)
    sl = slice(row0, row0 + m)
    _check(out, rows, ref, sl)
    assert abs(out[0] - ref["t"][sl].sum()) <= KSD_TOL * ref["A_rows"][sl].sum()
    assert abs(out[1] - ref["udiag"][sl].sum()) <= KSD_TOL * ref["udiag"][sl].sum()


@pytest.mark.parametrize("gemm", ["x3", "f32"])
@pytest.mark.parametrize("n,d", [(384, 128), (129, 37)])
def test_ksd_other_engines(gemm, n, d):
    X, target = _problem(n, d, seed=2)
    Xg, Sg = _scores(X, target)
    eng, out, rows = _run(Xg, Sg, gemm=gemm)
    assert eng.phi_gemm == gemm
    _check(out, rows, ksd_reference(X, Sg.cpu().numpy(), median_h64(X)))


def test_ksd_split_k_slices():
    """The smallest n at d = 256 whose phi_mm runs more than one split-K
    slice (the finish sums KY and rowsum over them), with pads."""
    from dsvgd import _native
    lib = _native.load()
    d = 256
    ldy = lib.dsvgd_ldy(lib.dsvgd_dp(d))
    n_pad = next(p for p in range(128, 1 << 16, 128) if lib.dsvgd_phi_splits_sym(p, ldy) > 1)
    n = n_pad - 127
    X, target = _problem(n, d)
    Xg, Sg = _scores(X, target)
    eng, out, rows = _run(Xg, Sg)
    assert eng.splits > 1 and eng.sym
    _check(out, rows, ksd_reference(X, Sg.cpu().numpy(), median_h64(X)))


@pytest.mark.parametrize("n,d,sym", [(300, 64, 0), (384, 128, 1)])
def test_ksd_more_than_one_sweep_slice(n, d, sym):
    """dsvgd_ksd_parts > 1 (full layout), more than one row slice (symmetric):
    the finish sums the slots; covered against fp64 by the cases above."""
    from dsvgd import _native
    lib = _native.load()
    X, target = _problem(n, d)
    Xg, Sg = _scores(X, target)
    eng, out, rows = _run(Xg, Sg)
    assert int(eng.sym) == sym
    parts = lib.dsvgd_ksd_parts(n, n, sym)
    assert eng._ksd["parts"] == parts
    assert (parts - lib.dsvgd_pad128(n) // 128 if sym else parts) > 1
    _check(out, rows, ksd_reference(X, Sg.cpu().numpy(), median_h64(X)))


def test_ksd_is_deterministic():
    X, target = _problem(513, 256)
    Xg, Sg = _scores(X, target)
    eng, out, rows = _run(Xg, Sg)
    out2, rows2 = eng.ksd(rows=True)
    assert out.tobytes() == out2.cpu().numpy().tobytes()
    assert rows.tobytes() == rows2.cpu().numpy().tobytes()


def test_ksd_refuses_scaled_scores_and_pair_split():
    import dsvgd
    X, target = _problem(129, 37)
    Xg, Sg = _scores(X, target)
    eng = dsvgd.PhiEngine(129, 37, device=DEV)
    eng.step(Xg, Sg, h=1.0, score_scale=0.5)
    with pytest.raises(ValueError):
        eng.ksd()
    eng.pack_scores(Sg)
    eng.direction()
    eng.ksd()
    eng.plan = object()     # (a pair-split engine: refused before anything is read)
    with pytest.raises(ValueError):
        eng.ksd()


def test_metrics_ksd_equals_engine_path():
    import dsvgd
    from dsvgd import metrics
    X, target = _problem(300, 64)
    Xg, Sg = _scores(X, target)
    eng, out, rows = _run(Xg, Sg)
    v = metrics.ksd(Xg, target)
    assert v == math.sqrt(max(out[2], 0.0))
    assert metrics.ksd(X, target, dsvgd.RBF("median"), device=DEV) == v     # host array in
    assert metrics.ksd(Xg, Sg) == v                                        # precomputed scores
    assert metrics.ksd(Xg, target, squared=True) == out[2]
    assert metrics.ksd(Xg, target, statistic="u", squared=True) == out[3]
    assert metrics.ksd(Xg, target, statistic="u") == math.sqrt(max(out[3], 0.0))
    eng2, out2, _ = _run(Xg, Sg, h=2.5)
    assert metrics.ksd(Xg, target, dsvgd.RBF(2.5), squared=True) == out2[2]
    with pytest.raises(ValueError):
        metrics.ksd(Xg, target, statistic="w")


def _frame_particles(df, l, n):
    return np.stack(df[df.timestep == l].sort_values("particle")["value"].to_list())


def _check_diagnostics(sampler, df, target, n, steps):
    diag = sampler.diagnostics
    assert list(diag.columns) == ["timestep", "ksd", "ksd2_v", "ksd2_u", "h"]
    assert list(diag.timestep) == steps
    worst = 0.0
    for _, row in diag.iterrows():
        X = _frame_particles(df, int(row.timestep), n).astype(np.float32)
        Xg, Sg = _scores(X, target)
        ref = ksd_reference(X, Sg.cpu().numpy(), float(row.h))
        ev = abs(row.ksd2_v - ref["V"]) / ref["A_v"]
        eu = abs(row.ksd2_u - ref["U"]) / ref["A_u"]
        print("timestep %d: V %.9g ref %.9g err/A %.3g, U err/A %.3g"
              % (row.timestep, row.ksd2_v, ref["V"], ev, eu))
        assert ev <= KSD_TOL and eu <= KSD_TOL
        assert row.ksd == math.sqrt(max(row.ksd2_v, 0.0))
        worst = max(worst, ev, eu)
    record_parity(worst)


def _same_frames(a, b):
    assert (a.timestep.values == b.timestep.values).all()
    assert (a.particle.values == b.particle.values).all()
    va, vb = np.stack(a["value"].to_list()), np.stack(b["value"].to_list())
    assert va.tobytes() == vb.tobytes()


@pytest.mark.parametrize("order,n,d", [("jacobi", 256, 8), ("sequential", 64, 8),
                                       ("jacobi", 64, 1), ("sequential", 64, 1)])
def test_sampler_ksd_every(order, n, d):
    import dsvgd
    if d == 1:
        target = dsvgd.targets.GaussianMixture1D()
    else:
        _, target = _problem(n, d)
    kw = dict(num_iter=6, step_size=0.05, order=order, device=DEV, verbose=False)
    s = dsvgd.Sampler(d, target, dsvgd.RBF("median"))
    torch.manual_seed(11)
    df = s.sample(n, ksd_every=2, **kw)
    _check_diagnostics(s, df, target, n, [0, 2, 4, 6])
    s0 = dsvgd.Sampler(d, target, dsvgd.RBF("median"))
    torch.manual_seed(11)
    df0 = s0.sample(n, **kw)
    assert s0.diagnostics is None
    _same_frames(df, df0)


def test_sampler_ksd_every_skips_a_final_timestep_off_the_grid():
    import dsvgd
    _, target = _problem(64, 8)
    s = dsvgd.Sampler(8, target, dsvgd.RBF(1.5))
    df = s.sample(64, 5, 0.05, order="jacobi", device=DEV, verbose=False, ksd_every=2)
    _check_diagnostics(s, df, target, 64, [0, 2, 4])
    assert (s.diagnostics.h == np.float32(1.5)).all()


def test_ksd_orders_target_draws_below_shifted_ones():
    import dsvgd
    from dsvgd import metrics
    n, d = 384, 128
    rs = np.random.RandomState(9)
    mu = rs.randn(d).astype(np.float32)
    lam = rs.uniform(0.5, 2.0, d).astype(np.float32)
    X = (mu + rs.randn(n, d) / np.sqrt(lam)).astype(np.float32)
    target = dsvgd.targets.Gaussian(mu, lam)
    good = metrics.ksd(torch.tensor(X, device=DEV), target)
    bad = metrics.ksd(torch.tensor(X + 1.0, device=DEV), target)
    assert good < bad
