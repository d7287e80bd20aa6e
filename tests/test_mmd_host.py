"""CPU-only tests of the MMD two-sample diagnostic: the fp64 reference the GPU
tests use (tests/mmd_reference.py) and its identities, the fp32 emulation of
csrc/mmd.hip's decomposition against the GPU tests' bounds on the GPU tests'
problems, GaussianMixture.sample, the new C ABI entry points' meta call and
argument refusals, and the public interface's refusals without a GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mmd_reference as R


def _kern(name):
    return R.KERNELS[name]


# ---- the reference ---------------------------------------------------------
def test_reference_matches_the_pairwise_definition():
    """MMD^2 from the three Gram-matrix means, written out pair by pair."""
    P, Q = R.problem(7, 5, 3)
    h = 2.3
    for fam, beta in R.KERNELS.values():
        def k(x, y):
            r2 = float(((x.astype(np.float64) - y.astype(np.float64)) ** 2).sum())
            return math.exp(-r2 / h) if fam == R.RBF else (1.0 + r2 / h) ** beta
        kpp = np.array([[k(a, b) for b in P] for a in P])
        kqq = np.array([[k(a, b) for b in Q] for a in Q])
        kpq = np.array([[k(a, b) for b in Q] for a in P])
        n, m = 7, 5
        V = kpp.mean() + kqq.mean() - 2.0 * kpq.mean()
        U = ((kpp.sum() - np.trace(kpp)) / (n * (n - 1)) + (kqq.sum() - np.trace(kqq)) / (m * (m - 1))
             - 2.0 * kpq.mean())
        ref = R.mmd_reference(P, Q, h, fam, beta)
        assert abs(ref["V"] - V) <= 1e-13 and abs(ref["U"] - U) <= 1e-13
        assert abs(ref["A"] - (kpp.mean() + kqq.mean() + 2.0 * kpq.mean())) <= 1e-13
        w = np.concatenate([kpp.mean(1) - kpq.mean(1), kpq.mean(0) - kqq.mean(1)])
        assert np.abs(ref["witness"] - w).max() <= 1e-13
        # MMD^2_V is the mean of the witness over P minus its mean over Q
        assert abs(ref["witness"][:n].mean() - ref["witness"][n:].mean() - V) <= 1e-13


@pytest.mark.parametrize("kernel", sorted(R.KERNELS))
def test_reference_identities(kernel):
    fam, beta = _kern(kernel)
    P, Q = R.problem(40, 33, 5)
    same = R.mmd_reference(P, P.copy(), None, fam, beta)
    assert abs(same["V"]) <= 1e-14 * same["A"]                  # V(P, P) = 0
    a, b = R.mmd_reference(P, Q, None, fam, beta), R.mmd_reference(Q, P, None, fam, beta)
    assert a["h"] == b["h"]
    assert abs(a["V"] - b["V"]) <= 1e-14 * a["A"] and abs(a["U"] - b["U"]) <= 1e-14 * a["A_u"]
    assert np.abs(a["witness"] + np.concatenate([b["witness"][33:], b["witness"][:33]])).max() <= 1e-14
    for seed in range(5):                                       # V >= 0
        P, Q = R.problem(12, 9, 2, seed=seed)
        assert R.mmd_reference(P, Q, None, fam, beta)["V"] >= 0.0
    one = R.mmd_reference(P, Q[:1], None, fam, beta)
    assert math.isnan(one["U"]) and math.isfinite(one["V"])


def test_reference_median_rule():
    P, Q = R.problem(6, 5, 2)
    D = R.sqdist64(np.concatenate([P, Q], 0))
    assert R.median64(D) == np.sort(D.ravel())[(121 - 1) // 2]
    assert R.mmd_reference(P, Q)["h"] == R.median64(D)          # no 1 / log N factor
    assert R.mmd_reference(P[:1], P[:1])["h"] == 1.0            # median 0 -> h = 1


# ---- the fp32 emulation on the GPU tests' problems --------------------------
def _emulation_cases():
    for (n, m, d) in R.SHAPES:
        sym = (n, m, d) in R.SYM_SHAPES
        for force in ((0,) + R.FORCED if (n, m, d) in R.SLICE_SHAPES else (0,)):
            yield n, m, d, sym, force
        if sym and (n, m, d) in R.ENGINE_SHAPES:
            yield n, m, d, False, 0     # the f32 engine keeps the full layout


@pytest.mark.parametrize("offcentre", [False, True])
@pytest.mark.parametrize("kernel", sorted(R.KERNELS))
@pytest.mark.parametrize("n,m,d,sym,force", list(_emulation_cases()))
def test_fp32_emulation_meets_the_gpu_bounds(n, m, d, sym, force, kernel, offcentre):
    fam, beta = _kern(kernel)
    P, Q = R.problem(n, m, d, offcentre)
    for h in (None, R.fixed_h(P, Q)):
        ref = R.mmd_reference(P, Q, h, fam, beta)
        out, rP, rQ, w = R.emulate32(P, Q, np.float32(ref["h"]), fam, beta, sym, force)
        R.check(out, rP, rQ, w, ref)


def test_emulation_layouts_agree_and_the_parts_rule_mirrors_the_library():
    lib = __import__("dsvgd")._native.load()
    for N in (1, 2, 128, 129, 300, 384, 513, 65536):
        for sym in (0, 1):
            for force in (0, 1, 2, 7):
                assert R.mmd_parts(N, sym, force) == lib.dsvgd_mmd_parts(N, sym, force)
    P, Q = R.problem(130, 254, 128)
    h = np.float32(R.median_h64(P, Q))
    full = R.emulate32(P, Q, h, sym=False)
    for force in (0, 1, 2):
        sym = R.emulate32(P, Q, h, sym=True, force=force)
        assert abs(sym[0][3] - full[0][3]) <= 1e-6 * R.mmd_reference(P, Q)["A"]
        assert np.abs(sym[1] - full[1]).max() <= 1e-5 * (full[1].max() + 1.0)


# ---- the problems of "it measures what it is for": the reference alone ------
@pytest.mark.parametrize("d,seed", R.SHIFT_CASES)
def test_reference_separates_shifted_draws(d, seed):
    A, B, Bs = R.shift_problem(d, seed)
    same, shift = R.mmd_reference(A, B)["U"], R.mmd_reference(A, Bs)["U"]
    print("d = %d: U_same %.4g U_shift %.4g ratio %.1f" % (d, same, shift, shift / abs(same)))
    assert shift >= 20.0 * abs(same)


@pytest.mark.parametrize("d,seed", R.MIXTURE_CASES)
def test_reference_separates_wrong_mixture_shares(d, seed):
    E1, E2, W = R.mixture_problem(d, seed)
    exact, wrong = R.mmd_reference(E1, E2)["U"], R.mmd_reference(W, E2)["U"]
    print("d = %d: U_exact %.4g U_wrong %.4g ratio %.1f" % (d, exact, wrong, wrong / abs(exact)))
    assert wrong >= 50.0 * abs(exact)


# ---- GaussianMixture.sample --------------------------------------------------
def _mixture():
    import dsvgd
    means = np.array([[-4.0, 1.0, 0.0], [5.0, -2.0, 3.0], [0.0, 8.0, -6.0]], np.float32)
    lam = np.array([[1.0, 4.0, 0.25], [2.0, 0.5, 1.0], [9.0, 1.0, 0.5]], np.float32)
    return dsvgd.targets.GaussianMixture(means, lam, [5.0, 3.0, 2.0]), means, lam


def test_mixture_sample_is_seeded_and_shaped():
    tgt, _, _ = _mixture()
    a, b = tgt.sample(100, seed=7), tgt.sample(100, seed=7)
    assert a.shape == (100, 3) and a.dtype == torch.float32 and a.device.type == "cpu"
    assert torch.equal(a, b)
    assert not torch.equal(a, tgt.sample(100, seed=8))
    assert not torch.equal(tgt.sample(100), tgt.sample(100))    # unseeded: fresh draws
    assert tgt.sample(1, seed=0).shape == (1, 3)
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            tgt.sample(bad)


def test_mixture_sample_statistics():
    """Shares within 5 sigma of the weights; every component's mean and
    variance, per coordinate, within 5 sigma of mu_k and 1 / lam_k."""
    tgt, means, lam = _mixture()
    m = 20000
    x = tgt.sample(m, seed=11).double().numpy()
    w = tgt.weights.numpy()
    assert np.allclose(w, [0.5, 0.3, 0.2])
    # the modes are far apart against their widths: the nearest mean is the component
    comp = ((x[:, None, :] - means[None].astype(np.float64)) ** 2).sum(-1).argmin(1)
    for k in range(3):
        mk = int((comp == k).sum())
        assert abs(mk / m - w[k]) <= 5.0 * math.sqrt(w[k] * (1.0 - w[k]) / m)
        xk = x[comp == k]
        var = 1.0 / lam[k].astype(np.float64)
        assert (np.abs(xk.mean(0) - means[k]) <= 5.0 * np.sqrt(var / mk)).all()
        # Var of the sample variance of a Gaussian: 2 sigma^4 / (mk - 1)
        assert (np.abs(xk.var(0, ddof=1) - var) <= 5.0 * var * math.sqrt(2.0 / (mk - 1))).all()


# ---- the public interface without a GPU --------------------------------------
def test_metrics_mmd_argument_errors_before_the_gpu():
    import dsvgd
    from dsvgd import metrics
    x, y = np.zeros((8, 3), np.float32), np.zeros((5, 3), np.float32)
    for bad in ((x, np.zeros((5, 4), np.float32)), (x, np.zeros(5, np.float32)),
                (np.zeros((2, 2, 3), np.float32), y), (np.zeros((0, 3), np.float32), y),
                (x, np.zeros((0, 3), np.float32)), (np.zeros((4, 0), np.float32),
                                                    np.zeros((4, 0), np.float32))):
        with pytest.raises(ValueError):
            metrics.mmd(*bad)
    with pytest.raises(ValueError):
        metrics.mmd(x, y, statistic="w")
    with pytest.raises(ValueError):
        metrics.mmd(x, y, lambda a, b: (a * b).sum())           # not an RBF / IMQ
    if not torch.cuda.is_available():
        from dsvgd._native import NativeUnavailable
        with pytest.raises(NativeUnavailable):
            metrics.mmd(x, y)
        with pytest.raises(NativeUnavailable):
            metrics.mmd(torch.zeros(8, 3), torch.zeros(5, 3), dsvgd.IMQ(1.0, -0.5), details=True)


def test_library_exports_mmd_entry_points():
    from dsvgd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("dsvgd_mmd_parts", "dsvgd_mmd_workspace_doubles", "dsvgd_mmd_rows",
                 "dsvgd_mmd_finish"):
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES


def test_mmd_parts_and_workspace_sizes():
    lib = __import__("dsvgd")._native.load()
    # full layout: enough column slices for ~2048 workgroups, >= 128 columns each
    assert lib.dsvgd_mmd_parts(300, 0, 0) == 3
    assert lib.dsvgd_mmd_parts(65536, 0, 0) == 4
    assert lib.dsvgd_mmd_parts(100, 0, 0) == 1
    # symmetric layout: the row slices plus one column-sum slot per tile row
    assert lib.dsvgd_mmd_parts(384, 1, 0) == 3 + 3
    assert lib.dsvgd_mmd_parts(65536, 1, 0) == 4 + 512
    # the override: that many slices, at most one per 128 columns
    assert lib.dsvgd_mmd_parts(300, 0, 2) == 2 and lib.dsvgd_mmd_parts(300, 0, 9) == 3
    assert lib.dsvgd_mmd_parts(384, 1, 1) == 1 + 3 and lib.dsvgd_mmd_parts(65536, 0, 1) == 1
    assert lib.dsvgd_mmd_parts(0, 0, 0) == 0 and lib.dsvgd_mmd_parts(-4, 1, 2) == 0
    assert lib.dsvgd_mmd_workspace_doubles(65) == 6 and lib.dsvgd_mmd_workspace_doubles(0) == 0


def test_mmd_calls_validate_arguments_without_gpu():
    """Every call below fails a check: none reaches a launch."""
    from dsvgd import _native
    lib = _native.load()
    err = lib.dsvgd_last_error
    rbf, imq = _native.Kernel(_native.KERNEL_RBF, 0.0), _native.Kernel(_native.KERNEL_IMQ, -0.5)
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def rows(D=p, ldd=384, N=300, nf=200, st=p, kern=rbf, sym=0, parts=3, force=0, P=p):
        return lib.dsvgd_mmd_rows(D, ldd, N, nf, st, kern, sym, parts, force, P, None)

    def finish(P=p, N=300, nf=200, sym=0, parts=3, force=0, rp=p, rq=p, w=p, ws=p, out=p):
        return lib.dsvgd_mmd_finish(P, N, nf, sym, parts, force, rp, rq, w, ws, out, None)

    for kw in ({"D": None}, {"st": None}, {"P": None}):
        assert rows(**kw) == -1 and b"null" in err()
    for kw in ({"P": None}, {"ws": None}, {"out": None}):
        assert finish(**kw) == -1 and b"null" in err()
    for fn in (rows, finish):
        for kw in ({"N": 0}, {"N": 1, "nf": 1}, {"N": -3}, {"N": 2 ** 20 + 1}):
            assert fn(**kw) == -1 and b"sizes" in err()
        for nf in (0, -1, 300, 301):
            assert fn(nf=nf) == -1 and b"n_first" in err()
        for kw in ({"parts": 2}, {"parts": 0}, {"force": 2}, {"sym": 1}, {"parts": 6, "force": 1}):
            assert fn(**kw) == -1 and b"parts" in err()
    assert rows(ldd=300) == -1 and b"ldd" in err()
    assert rows(ldd=512) == -1 and b"ldd" in err()
    assert rows(D=p + 4) == -1 and b"aligned" in err()
    assert rows(P=p + 2) == -1 and b"aligned" in err()
    assert finish(ws=p + 4) == -1 and b"aligned" in err()
    assert finish(out=p + 4) == -1 and b"aligned" in err()
    assert finish(w=p + 1) == -1 and b"aligned" in err()
    for bad in (_native.Kernel(2, 0.0), _native.Kernel(_native.KERNEL_IMQ, 0.0),
                _native.Kernel(_native.KERNEL_IMQ, -1.5), _native.Kernel(-1, -0.5)):
        assert rows(kern=bad) == -1 and b"kern" in err()
    # the nullable outputs of the finish are not what is refused
    assert finish(rp=None, rq=None, w=None, parts=2) == -1 and b"parts" in err()
    # a well-formed IMQ call is refused for its sizes alone, not its kernel
    assert rows(kern=imq, N=0) == -1 and b"sizes" in err()


# ---- the experiment ------------------------------------------------------------
def test_experiment_default_is_unchanged_and_mmd_is_parsed(monkeypatch):
    from test_gmix_host import experiment
    E = experiment()
    import inspect
    sig = inspect.signature(E.run)
    assert list(sig.parameters)[:12] == ["nparticles", "niter", "stepsize", "every", "d", "modes",
                                         "spread", "order", "kernel", "seed", "device", "out"]
    assert sig.parameters["mmd"].default == 0
    defaults = {p.name: p.default for p in E.cli.params}
    assert defaults["mmd"] == 0
    from click.testing import CliRunner
    assert "--mmd" in CliRunner().invoke(E.cli, ["--help"]).output
    got = {}
    monkeypatch.setattr(E, "run", lambda *a, **kw: got.update(args=a, kw=kw))
    assert CliRunner().invoke(E.cli, ["--mmd", "64", "--d", "2"]).exit_code == 0
    assert got["kw"] == {"mmd": 64} and got["args"][4] == 2
    assert CliRunner().invoke(E.cli, []).exit_code == 0
    assert got["kw"] == {"mmd": 0}
    assert CliRunner().invoke(E.cli, ["--mmd", "many"]).exit_code != 0

    # the line layout, with the device-side pieces replaced by stubs: mmd = 0
    # prints what it printed before; mmd > 0 adds the entry and "final mmd"
    # before "final ksd"
    class _Sampler(object):
        def __init__(self, d, target, kern):
            self.d = d

        def sample(self, n, niter, step, **kw):
            import pandas as pd
            return pd.DataFrame({"value": [np.zeros(self.d, np.float32)] * ((niter + 1) * n)})

    monkeypatch.undo()
    E = experiment()
    monkeypatch.setattr(E.dsvgd, "Sampler", _Sampler)
    monkeypatch.setattr(E.dsvgd.metrics, "mode_shares", lambda P, t: torch.tensor([0.25, 0.75]))
    monkeypatch.setattr(E.dsvgd.metrics, "gmix_logp", lambda P, t: torch.zeros(len(P)))
    monkeypatch.setattr(E.dsvgd.metrics, "ksd", lambda *a, **kw: 0.5)
    monkeypatch.setattr(E.dsvgd.metrics, "mmd", lambda P, Q, **kw: 0.125 + 0 * len(Q))
    lines = []
    curve, ksd = E.run(4, 2, 1.0, 1, device="cpu", out=lines.append)
    assert ksd == 0.5 and [sorted(r) for r in curve] == [["iteration", "logp", "shares"]] * 3
    assert lines == ["weights [0.500 0.500]"] + [
        "iteration %5d  shares [0.250 0.750]  mean logp 0.0000" % it for it in (0, 1, 2)] + [
        "final ksd 0.5"]
    lines = []
    curve, ksd = E.run(4, 2, 1.0, 1, device="cpu", out=lines.append, mmd=16)
    assert ksd == 0.5 and all(r["mmd"] == 0.125 for r in curve)
    assert lines[1] == "iteration     0  shares [0.250 0.750]  mean logp 0.0000  mmd 0.125"
    assert lines[-2:] == ["final mmd 0.125", "final ksd 0.5"]
    with pytest.raises(ValueError):
        E.run(4, 2, 1.0, 1, device="cpu", out=lines.append, mmd=-1)
