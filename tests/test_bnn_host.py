"""Host-side checks of the Bayesian neural-network target (no GPU): the fp64
closed form of tests/bnn_reference.py against fp64 autograd of
BayesianNN.logp, the target's validation and digest, and the argument checks
of its two entry points."""
import ctypes

import numpy as np
import pytest
import torch

import bnn_reference as R


def _target(Z, y, H, **kw):
    from dsvgd.targets import BayesianNN
    return BayesianNN(torch.from_numpy(Z), torch.from_numpy(y), hidden=H, **kw)


def test_score64_matches_fp64_autograd_of_logp():
    n, N, p, H = 3, 37, 5, 7
    X, Z, y = R.problem(n, N, p, H, seed=3)
    tgt = _target(Z, y, H)
    assert tgt.d == R.dim(p, H) == X.shape[1] and tgt.N == N and tgt.p == p
    S, A, _ = R.score64(X, Z, y, p, H)
    for i in range(n):
        x = torch.from_numpy(X[i].astype(np.float64)).requires_grad_(True)
        (g,) = torch.autograd.grad(tgt.logp(x), x)
        assert np.all(np.abs(g.numpy() - S[i]) <= 1e-12 * A[i])
    # other hyper-prior parameters reach both the closed form and logp
    tgt2 = _target(Z, y, H, a0=2.0, b0=0.5)
    S2, A2, _ = R.score64(X, Z, y, p, H, 2.0, 0.5)
    x = torch.from_numpy(X[0].astype(np.float64)).requires_grad_(True)
    (g,) = torch.autograd.grad(tgt2.logp(x), x)
    assert np.all(np.abs(g.numpy() - S2[0]) <= 1e-12 * A2[0])
    assert np.abs(S2[0, -2:] - S[0, -2:]).min() > 0.1


def test_logp_is_a_reference_style_callable_and_batches_under_vmap():
    n, N, p, H = 4, 11, 3, 2
    X, Z, y = R.problem(n, N, p, H, seed=1)
    tgt = _target(Z, y, H)
    Xt = torch.from_numpy(X)
    assert tgt(Xt[0]).shape == () and tgt(Xt[0]) == tgt.logp(Xt[0])
    g = torch.func.vmap(torch.func.grad(tgt.logp))(Xt.double()).numpy()
    S, A, _ = R.score64(X, Z, y, p, H)
    assert np.all(np.abs(g - S) <= 1e-12 * A)


def test_fingerprint_follows_the_data_and_the_model():
    _, Z, y = R.problem(1, 20, 4, 3, seed=2)
    fp = _target(Z, y, 3).fingerprint()
    assert _target(Z.copy(), y.copy(), 3).fingerprint() == fp
    assert _target(Z, y, 4).fingerprint() != fp
    y2 = y.copy()
    y2[7] = np.nextafter(y2[7], np.float32(9))
    assert _target(Z, y2, 3).fingerprint() != fp
    assert _target(Z, y, 3, a0=2.0).fingerprint() != fp
    assert _target(Z, y, 3, b0=0.2).fingerprint() != fp
    if torch.cuda.is_available():   # the digest is of the values, wherever they live
        from dsvgd.targets import BayesianNN
        dev = BayesianNN(torch.from_numpy(Z).cuda(), torch.from_numpy(y).cuda(), hidden=3)
        assert dev.fingerprint() == fp


def test_unsupported_shapes_are_refused():
    from dsvgd.targets import BayesianNN
    _, Z, y = R.problem(1, 6, 4, 3, seed=2)
    for hidden in (0, 65, -1):
        with pytest.raises(ValueError):
            _target(Z, y, hidden)
    with pytest.raises(ValueError):
        BayesianNN(torch.zeros(6, 65), torch.zeros(6), hidden=3)
    with pytest.raises(ValueError):
        BayesianNN(torch.zeros(6, 0), torch.zeros(6), hidden=3)
    with pytest.raises(ValueError):
        BayesianNN(torch.zeros(6, 4), torch.zeros(5), hidden=3)
    BayesianNN(torch.zeros(6, 64), torch.zeros(6), hidden=64)
    tgt = _target(Z, y, 3)
    with pytest.raises(ValueError):
        tgt.logp(torch.zeros(tgt.d + 1))
    with pytest.raises(AssertionError):
        tgt.score(torch.zeros(2, tgt.d + 1), torch.zeros(2, tgt.d + 1))


def test_sampler_without_gpu_raises_native_unavailable(monkeypatch):
    """No device visible (as on a CPU machine; forced here so the test runs
    everywhere): the sampler refuses, there is no other compute path."""
    import dsvgd
    from dsvgd._native import NativeUnavailable
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    _, Z, y = R.problem(1, 6, 4, 3, seed=2)
    tgt = _target(Z, y, 3)
    with pytest.raises(NativeUnavailable):
        dsvgd.Sampler(tgt.d, tgt, dsvgd.RBF(1.0)).sample(4, 1, 0.1, verbose=False)


def experiment():
    import importlib.util
    import os

    from conftest import PKG
    spec = importlib.util.spec_from_file_location(
        "dsvgd_bnn_experiment", os.path.join(PKG, "experiments", "bnn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_experiment_dataset_is_seeded_and_split():
    E = experiment()
    xtr, ytr, xte, yte = E.synthetic_regression(1000, 8, seed=0)
    assert xtr.shape == (900, 8) and ytr.shape == (900,) and xte.shape == (100, 8)
    assert xtr.dtype == np.float32 and yte.dtype == np.float32
    again = E.synthetic_regression(1000, 8, seed=0)
    assert all(np.array_equal(a, b) for a, b in zip((xtr, ytr, xte, yte), again))
    assert not np.array_equal(E.synthetic_regression(1000, 8, seed=1)[1], ytr)
    # y = sin(sum z) + 0.1 noise
    assert np.abs(ytr - np.sin(xtr.sum(1))).std() < 0.15
    from click.testing import CliRunner
    res = CliRunner().invoke(E.cli, ['--help'])
    assert res.exit_code == 0
    for opt in ('--nparticles', '--niter', '--stepsize', '--every', '--hidden'):
        assert opt in res.output


def test_library_exports_the_bnn_entry_points_and_abi_stays_4():
    from dsvgd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("dsvgd_score_bnn", "dsvgd_bnn_predict"):
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES
    assert _native.load().dsvgd_abi_version() == 4


def test_entry_points_validate_arguments_without_gpu():
    """Every call below fails a check: none reaches a launch."""
    from dsvgd import _native as N
    lib = N.load()
    buf = (ctypes.c_double * 64)()
    q = ctypes.addressof(buf)
    p, H = 5, 7
    d = R.dim(p, H)

    def err():
        return lib.dsvgd_last_error()
    for null in range(4):
        a = [q, q, q, q]
        a[null] = None
        rc = lib.dsvgd_score_bnn(a[0], d, 2, d, a[1], p, a[2], 9, p, H, 1.0, 0.1, 1.0, a[3], d,
                                 None)
        assert rc == -1 and b"null" in err()
    for null in range(3):
        a = [q, q, q]
        a[null] = None
        rc = lib.dsvgd_bnn_predict(a[0], d, 2, d, a[1], p, 9, p, H, a[2], 9, None)
        assert rc == -1 and b"null" in err()
    for bad_d in (d - 1, d + 1):
        rc = lib.dsvgd_score_bnn(q, d + 1, 2, bad_d, q, p, q, 9, p, H, 1.0, 0.1, 1.0, q, d + 1, None)
        assert rc == -1 and b"H (p + 2) + 3" in err()
        rc = lib.dsvgd_bnn_predict(q, d + 1, 2, bad_d, q, p, 9, p, H, q, 9, None)
        assert rc == -1 and b"H (p + 2) + 3" in err()
    for bp, bh in ((0, 7), (65, 7), (5, 0), (5, 65)):
        bd = R.dim(bp, bh)
        rc = lib.dsvgd_score_bnn(q, bd, 2, bd, q, max(bp, 1), q, 9, bp, bh, 1.0, 0.1, 1.0, q, bd,
                                 None)
        assert rc == -1 and b"64" in err()
        rc = lib.dsvgd_bnn_predict(q, bd, 2, bd, q, max(bp, 1), 9, bp, bh, q, 9, None)
        assert rc == -1 and b"64" in err()
    # sizes: no particles, no rows, leading dimensions below the widths
    for n, N_, ldx, ldz, lds in ((0, 9, d, p, d), (2, 0, d, p, d), (2, 9, d - 1, p, d),
                                 (2, 9, d, p - 1, d), (2, 9, d, p, d - 1)):
        rc = lib.dsvgd_score_bnn(q, ldx, n, d, q, ldz, q, N_, p, H, 1.0, 0.1, 1.0, q, lds, None)
        assert rc == -1 and b"sizes" in err()
    rc = lib.dsvgd_bnn_predict(q, d, 2, d, q, p, 9, p, H, q, 8, None)
    assert rc == -1 and b"sizes" in err()
