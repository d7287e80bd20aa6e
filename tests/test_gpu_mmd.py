"""GPU tests of the MMD two-sample diagnostic (csrc/mmd.hip, PhiEngine.mmd,
metrics.mmd, GaussianMixture.sample, experiments/gmm.py --mmd) against the
fp64 closed form on the same fp32 inputs (tests/mmd_reference.py).

Tolerance: MMD^2 cancels without its rounding error shrinking, so errors are
measured against sums of positive terms: |rP_i - ref| <= 1e-5 (rP_i + 1)
(likewise rQ), |witness_i - ref| <= 1e-5 (its absolute-term sum), |V - V_ref|
<= 1e-5 A, |U - U_ref| <= 1e-5 A_u (mmd_reference.py; 1e-5 is the project's
phi / KSD bound).  The fp32 numpy emulation of the decomposition gives up to
7.3e-7 per row and 3.1e-8 of A on these shapes (tests/test_mmd_host.py)."""
import math

import numpy as np
import pytest
import torch

import mmd_reference as R
from conftest import record_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _kernel(name, h="median"):
    import dsvgd
    return dsvgd.RBF(h) if name == "rbf" else dsvgd.IMQ(h, R.KERNELS[name][1])


def _run(P, Q, kernel="rbf", h=None, parts=None, **kw):
    """One engine evaluation of the pooled set; h=None: the median rule (the
    select's median, without the sampler's 1 / log N)."""
    import dsvgd
    n, d = P.shape
    Z = torch.tensor(np.concatenate([P, Q], 0), device=DEV)
    eng = dsvgd.PhiEngine(len(Z), d, device=DEV, kernel=_kernel(kernel), **kw)
    eng.pack(Z)
    eng.distances(median=h is None)
    if h is None:
        eng.median_bandwidth()
        med = eng.state.read()[0]
        h = med if med > 0.0 else 1.0
    eng.fixed_bandwidth(h)
    out, rp, rq, w = eng.mmd(n, rows=True, parts=parts)
    return eng, out.cpu().numpy(), rp.cpu().numpy(), rq.cpu().numpy(), w.cpu().numpy()


def _parity(n, m, d, kernel, offcentre, parts=None, **kw):
    """Both bandwidth rules against fp64; returns the last engine."""
    fam, beta = R.KERNELS[kernel]
    P, Q = R.problem(n, m, d, offcentre)
    worst = 0.0
    for h in (None, R.fixed_h(P, Q)):
        ref = R.mmd_reference(P, Q, h, fam, beta)
        eng, out, rp, rq, w = _run(P, Q, kernel, h, parts, **kw)
        hg = eng.state.read()[1]
        print("h %.9g ref %.9g" % (hg, ref["h"]))
        assert abs(hg - ref["h"]) <= 1e-5 * ref["h"]
        worst = max(worst, R.check(out, rp, rq, w, ref))
    record_parity(worst)
    return eng


@pytest.mark.parametrize("offcentre", [False, True])
@pytest.mark.parametrize("kernel", sorted(R.KERNELS))
@pytest.mark.parametrize("n,m,d", R.SHAPES)
def test_mmd_matches_fp64(n, m, d, kernel, offcentre):
    eng = _parity(n, m, d, kernel, offcentre)
    assert eng.sym == ((n, m, d) in R.SYM_SHAPES)      # the layout the case is for
    assert eng._mmd["parts"] == R.mmd_parts(n + m, int(eng.sym))


@pytest.mark.parametrize("kernel", sorted(R.KERNELS))
@pytest.mark.parametrize("parts", R.FORCED)
@pytest.mark.parametrize("n,m,d", R.SLICE_SHAPES)
def test_mmd_forced_slice_counts(n, m, d, parts, kernel):
    """One slice (what a large matrix has per tile row: many tiles per
    workgroup) and two uneven ones, where the default rule gives three."""
    eng = _parity(n, m, d, kernel, True, parts=parts)
    T = eng.n_pad // 128
    assert eng._mmd["parts"] == parts + (T if eng.sym else 0) != R.mmd_parts(n + m, int(eng.sym))


@pytest.mark.parametrize("kernel", sorted(R.KERNELS))
@pytest.mark.parametrize("gemm", ["x3", "f32"])
@pytest.mark.parametrize("n,m,d", R.ENGINE_SHAPES)
def test_mmd_other_engines(n, m, d, gemm, kernel):
    eng = _parity(n, m, d, kernel, False, gemm=gemm)
    assert eng.phi_gemm == gemm and eng.gram_gemm == gemm
    assert eng.sym == (gemm == "x3" and (n, m, d) in R.SYM_SHAPES)


def test_mmd_is_deterministic_and_keeps_its_workspaces():
    P, Q = R.problem(257, 256, 256)
    eng, out, rp, rq, w = _run(P, Q)
    W = eng._mmd
    out2, rp2, rq2, w2 = eng.mmd(257, rows=True)
    assert eng._mmd is W
    assert out.tobytes() == out2.cpu().numpy().tobytes()
    for a, b in ((rp, rp2), (rq, rq2), (w, w2)):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    buf = torch.empty(5, dtype=torch.float64, device=DEV)
    assert eng.mmd(257, out=buf) is buf and buf.cpu().numpy().tobytes() == out.tobytes()
    # a second engine on the same inputs: the same bits
    _, out3, rp3, _, _ = _run(P, Q)
    assert out.tobytes() == out3.tobytes() and rp.tobytes() == rp3.tobytes()


@pytest.mark.parametrize("kernel", sorted(R.KERNELS))
@pytest.mark.parametrize("n,m,d", [(200, 100, 64), (130, 254, 128)])
def test_mmd_is_symmetric_in_its_sets_and_vanishes_on_equal_sets(n, m, d, kernel):
    fam, beta = R.KERNELS[kernel]
    P, Q = R.problem(n, m, d)
    ref = R.mmd_reference(P, Q, None, fam, beta)
    _, a, rpa, rqa, wa = _run(P, Q, kernel)
    _, b, rpb, rqb, wb = _run(Q, P, kernel)
    assert abs(a[3] - b[3]) <= R.MMD_TOL * ref["A"] and abs(a[4] - b[4]) <= R.MMD_TOL * ref["A_u"]
    assert abs(a[0] - b[2]) <= R.MMD_TOL * (ref["PP"] + 1) and abs(a[1] - b[1]) <= R.MMD_TOL * (ref["PQ"] + 1)
    assert (np.abs(wa + np.concatenate([wb[m:], wb[:m]])) <= R.MMD_TOL * ref["A_w"]).all()
    same = R.mmd_reference(P, P, None, fam, beta)
    _, c, _, _, wc = _run(P, P.copy(), kernel)
    print("V(P, P) = %.3g, A = %.3g" % (c[3], same["A"]))
    assert abs(c[3]) <= R.MMD_TOL * same["A"]
    assert (np.abs(wc) <= R.MMD_TOL * same["A_w"]).all()


def test_metrics_mmd_equals_engine_path():
    import dsvgd
    from dsvgd import metrics
    P, Q = R.problem(200, 100, 64)
    Pg, Qg = torch.tensor(P, device=DEV), torch.tensor(Q, device=DEV)
    _, out, rp, rq, w = _run(P, Q)
    assert metrics.mmd(Pg, Qg, squared=True) == out[4]
    assert metrics.mmd(Pg, Qg) == math.sqrt(max(out[4], 0.0))
    assert metrics.mmd(P, Q, dsvgd.RBF("median"), device=DEV, squared=True) == out[4]    # host arrays in
    assert metrics.mmd(Pg, Q, statistic="v", squared=True) == out[3]
    assert metrics.mmd(Pg, Qg, statistic="v") == math.sqrt(max(out[3], 0.0))
    det = metrics.mmd(Pg, Qg, details=True)
    assert sorted(det) == ["h", "m", "mmd", "mmd2_u", "mmd2_v", "n", "witness"]
    assert (det["n"], det["m"], det["mmd2_v"], det["mmd2_u"]) == (200, 100, out[3], out[4])
    assert det["mmd"] == math.sqrt(max(out[4], 0.0))
    assert abs(det["h"] - R.median_h64(P, Q)) <= 1e-5 * det["h"]
    wit = det["witness"]
    assert wit.shape == (300,) and wit.dtype == torch.float32 and wit.is_cuda
    assert wit.cpu().numpy().tobytes() == w.tobytes()
    # a kernel with a number is used as given
    for name in sorted(R.KERNELS):
        _, out2, _, _, _ = _run(P, Q, name, h=2.5 * 64)
        det2 = metrics.mmd(Pg, Qg, _kernel(name, 2.5 * 64), statistic="v", squared=True, details=True)
        assert det2["mmd"] == out2[3] and det2["h"] == 2.5 * 64
    one = metrics.mmd(Pg, Qg[:1], details=True)
    assert math.isnan(one["mmd"]) and math.isnan(one["mmd2_u"]) and one["mmd2_v"] > 0
    with pytest.raises(ValueError):
        metrics.mmd(Pg, Qg, statistic="w")
    with pytest.raises(ValueError):
        metrics.mmd(Pg, Qg[:, :5])


def test_mmd_refuses_row_blocks_pair_split_and_bad_boundaries():
    import dsvgd
    P, Q = R.problem(200, 185, 16)
    Z = torch.tensor(np.concatenate([P, Q], 0), device=DEV)
    eng = dsvgd.PhiEngine(385, 16, m=128, row0=128, device=DEV)
    eng.pack(Z)
    eng.distances()
    eng.fixed_bandwidth(16.0)
    with pytest.raises(ValueError):
        eng.mmd(200)
    eng = dsvgd.PhiEngine(385, 16, device=DEV)
    eng.pack(Z)
    eng.distances()
    eng.fixed_bandwidth(16.0)
    for bad in (0, 385, -1):
        with pytest.raises(ValueError):
            eng.mmd(bad)
    assert eng._mmd is None                 # refused before anything is allocated
    eng.mmd(200)
    eng.plan = object()     # (a pair-split engine: refused before anything is read)
    with pytest.raises(ValueError):
        eng.mmd(200)


# ---- it measures what it is for ---------------------------------------------
def _ksd_note(name, X, target):
    from dsvgd import metrics
    print("  ksd of %s: %.6g" % (name, metrics.ksd(torch.tensor(X, device=DEV), target)))


@pytest.mark.parametrize("d,seed", R.SHIFT_CASES)
def test_mmd_separates_shifted_draws(d, seed):
    import dsvgd
    from dsvgd import metrics
    A, B, Bs = R.shift_problem(d, seed)
    same = metrics.mmd(A, B, squared=True, device=DEV)
    shift = metrics.mmd(A, Bs, squared=True, device=DEV)
    print("d = %d: U_same %.6g U_shift %.6g ratio %.1f" % (d, same, shift, shift / abs(same)))
    target = dsvgd.targets.Gaussian(np.zeros(d, np.float32), np.ones(d, np.float32))
    _ksd_note("B", B, target)
    _ksd_note("B + 0.5", Bs, target)
    assert shift >= 10.0 * abs(same)


@pytest.mark.parametrize("d,seed", R.MIXTURE_CASES)
def test_mmd_sees_wrong_mixture_shares(d, seed):
    from dsvgd import metrics
    E1, E2, W = R.mixture_problem(d, seed)
    exact = metrics.mmd(E1, E2, squared=True, device=DEV)
    wrong = metrics.mmd(W, E2, squared=True, device=DEV)
    print("d = %d: U_exact %.6g U_wrong %.6g ratio %.1f" % (d, exact, wrong, wrong / abs(exact)))
    target = R.mixture_targets(d)[0]
    _ksd_note("exact draws", E1, target)      # (score-based: blind to the shares)
    _ksd_note("0.9 / 0.1 draws", W, target)
    assert wrong >= 20.0 * abs(exact)


def test_mixture_sample_lands_on_the_device_with_the_host_draws():
    exact = R.mixture_targets(3)[0]
    a = exact.sample(33, seed=5, device=DEV)
    assert a.is_cuda and a.shape == (33, 3) and a.dtype == torch.float32
    assert torch.equal(a.cpu(), exact.sample(33, seed=5))


# ---- the experiment -----------------------------------------------------------
def test_experiment_with_mmd_runs_through_the_cli():
    from click.testing import CliRunner

    from test_gmix_host import experiment
    E = experiment()
    res = CliRunner().invoke(E.cli, ['--d', '3', '--modes', '4', '--spread', '3', '--nparticles',
                                     '24', '--niter', '4', '--every', '2', '--order', 'jacobi',
                                     '--seed', '1', '--mmd', '64'])
    assert res.exit_code == 0, res.output
    lines = res.output.strip().splitlines()
    assert [ln.split()[1] for ln in lines[1:4]] == ["0", "2", "4"]
    for ln in lines[1:4]:
        assert ln.split()[-2] == "mmd" and np.isfinite(float(ln.split()[-1]))
    assert lines[-2].startswith("final mmd") and lines[-2].split()[-1] == lines[3].split()[-1]
    assert lines[-1].startswith("final ksd") and np.isfinite(float(lines[-1].split()[-1]))
    curve, ksd = E.run(16, 2, 1.0, 1, out=lambda s: None, mmd=64)   # the reference's model, d = 1
    assert [r["iteration"] for r in curve] == [0, 1, 2]
    assert all(np.isfinite(r["mmd"]) and r["mmd"] >= 0 for r in curve)
    curve, ksd = E.run(16, 2, 1.0, 1, out=lambda s: None)        # off: no entry
    assert all("mmd" not in r for r in curve) and np.isfinite(ksd)
