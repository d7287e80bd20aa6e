"""Host-side checks of the AdaGrad steps and the minibatch BayesianNN target
(no GPU): the rule's arguments, the combinations the samplers refuse, the
target's batch argument, digest and full-data twin, the three new entry
points and their argument checks, and the fp64 minibatch score of
tests/adagrad_reference.py against fp64 autograd of the weighted log density."""
import ctypes

import numpy as np
import pytest
import torch

import adagrad_reference as A
import bnn_reference as R


def _target(Z, y, H, **kw):
    from dsvgd.targets import BayesianNN
    return BayesianNN(torch.from_numpy(Z), torch.from_numpy(y), hidden=H, **kw)


def test_adagrad_validates_and_prints():
    import dsvgd
    from dsvgd.adagrad import resolve_adagrad
    a = dsvgd.AdaGrad()
    assert (a.alpha, a.eps) == (0.9, 1e-6)
    assert repr(dsvgd.AdaGrad(0.5, 1e-3)) == "AdaGrad(alpha=0.5, eps=0.001)"
    dsvgd.AdaGrad(0.0, 1e-30)
    for alpha in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            dsvgd.AdaGrad(alpha=alpha)
    for eps in (0.0, -1e-6, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            dsvgd.AdaGrad(eps=eps)
    assert "AdaGrad" in dsvgd.__all__
    assert resolve_adagrad(None) is None and resolve_adagrad(False) is None
    assert resolve_adagrad(a) is a
    assert isinstance(resolve_adagrad(True), dsvgd.AdaGrad)
    with pytest.raises(ValueError):
        resolve_adagrad(0.9)


def test_sampler_refuses_adagrad_in_the_sequential_order():
    import dsvgd
    s = dsvgd.Sampler(3, dsvgd.targets.Gaussian(np.zeros(3), np.ones(3)), dsvgd.RBF(1.0))
    with pytest.raises(ValueError, match="sequential"):
        s.sample(8, 1, 0.1, order="sequential", adagrad=True, verbose=False)
    with pytest.raises(ValueError, match="sequential"):
        s.sample(8, 1, 0.1, adagrad=dsvgd.AdaGrad(), verbose=False)   # (the default order)
    with pytest.raises(ValueError, match="adagrad"):
        s.sample(8, 1, 0.1, order="jacobi", adagrad=0.5, verbose=False)


def test_distsampler_refuses_adagrad_where_blocks_travel():
    import dsvgd
    tgt = dsvgd.targets.Gaussian(np.zeros(3), np.ones(3))
    X = torch.zeros(8, 3)

    def make(S, xp, xs, w2, **kw):
        return dsvgd.DistSampler(0, S, tgt, dsvgd.RBF(1.0), X, 1, 1, xp, xs, w2, adagrad=True, **kw)
    with pytest.raises(ValueError, match="partitions"):
        make(2, False, False, False, order="jacobi")
    for lagged in ("local", "updateall"):
        with pytest.raises(ValueError, match="lagged"):
            make(2, False, False, False, order="jacobi", lagged=lagged)
    with pytest.raises(ValueError, match="sequential"):
        make(1, True, True, False, order="sequential")
    with pytest.raises(ValueError, match="sequential"):
        make(2, True, False, False)     # (the default order)
    with pytest.raises(ValueError, match="adagrad"):
        dsvgd.DistSampler(0, 1, tgt, dsvgd.RBF(1.0), X, 1, 1, True, True, False, order="jacobi",
                          adagrad="yes")


def test_bnn_batch_argument_digest_and_full_twin():
    _, Z, y = R.problem(1, 20, 4, 3, seed=2)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            _target(Z, y, 3, batch=bad)
    full = _target(Z, y, 3)
    assert full.batch is None and full.full is full
    for whole in (20, 21, 1000):    # batch >= N: the full-data target
        t = _target(Z, y, 3, batch=whole)
        assert t.batch is None and t.fingerprint() == full.fingerprint()
    mb = _target(Z, y, 3, batch=5)
    assert mb.batch == 5
    assert mb.fingerprint() != full.fingerprint()
    assert mb.fingerprint() != _target(Z, y, 3, batch=6).fingerprint()
    assert mb.fingerprint() == _target(Z.copy(), y.copy(), 3, batch=5).fingerprint()
    twin = mb.full
    assert twin is mb.full and twin.batch is None and twin.full is twin
    assert twin.x is mb.x and twin.y is mb.y and twin._dev is mb._dev
    assert twin.fingerprint() == full.fingerprint()
    assert (twin.hidden, twin.a0, twin.b0, twin.d) == (mb.hidden, mb.a0, mb.b0, mb.d)
    # logp stays the full-data density
    x = torch.from_numpy(R.problem(1, 20, 4, 3, seed=2)[0][0].astype(np.float64))
    assert float(mb.logp(x)) == float(full.logp(x))
    # the base class hooks do nothing
    from dsvgd.targets import Gaussian
    g = Gaussian(np.zeros(2), np.ones(2))
    assert g.next_batch() is None and g.reset_batch(3) is None
    assert full.next_batch() is None and full.reset_batch() is None


def test_library_exports_the_new_entry_points_and_abi_stays_4():
    from dsvgd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("dsvgd_adagrad_step", "dsvgd_score_bnn_window", "dsvgd_window_advance"):
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES
    assert _native.load().dsvgd_abi_version() == 4


def test_entry_points_validate_arguments_without_gpu():
    """Every call below fails a check: none reaches a launch."""
    from dsvgd import _native as N
    lib = N.load()
    buf = (ctypes.c_double * 64)()
    q = ctypes.addressof(buf)

    def err():
        return lib.dsvgd_last_error()
    # the AdaGrad update
    for null in range(3):
        a = [q, q, q]
        a[null] = None
        rc = lib.dsvgd_adagrad_step(a[0], 4, a[1], 4, a[2], 4, 2, 4, 0.1, 0.9, 1e-6, None)
        assert rc == -1 and b"null" in err()
    for ldx, ldp, ldg in ((3, 4, 4), (4, 3, 4), (4, 4, 3)):
        rc = lib.dsvgd_adagrad_step(q, ldx, q, ldp, q, ldg, 2, 4, 0.1, 0.9, 1e-6, None)
        assert rc == -1 and b">= d" in err()
    for m, d in ((0, 4), (2, 0), (-1, 4)):
        rc = lib.dsvgd_adagrad_step(q, 4, q, 4, q, 4, m, d, 0.1, 0.9, 1e-6, None)
        assert rc == -1 and b"m, d > 0" in err()
    for alpha in (-0.1, 1.0, float("nan")):
        rc = lib.dsvgd_adagrad_step(q, 4, q, 4, q, 4, 2, 4, 0.1, alpha, 1e-6, None)
        assert rc == -1 and b"alpha" in err()
    for eps in (0.0, -1.0, float("nan")):
        rc = lib.dsvgd_adagrad_step(q, 4, q, 4, q, 4, 2, 4, 0.1, 0.9, eps, None)
        assert rc == -1 and b"eps" in err()
    # the window score
    p, H = 5, 7
    d = R.dim(p, H)

    def window(a, d_=d, n=2, N_=9, ldx=d, ldz=p, lds=d, p_=p, H_=H, B=4):
        return lib.dsvgd_score_bnn_window(a[0], ldx, n, d_, a[1], ldz, a[2], N_, p_, H_, 1.0, 0.1,
                                          1.0, a[3], B, a[4], lds, None)
    for null in range(5):
        a = [q] * 5
        a[null] = None
        assert window(a) == -1 and b"null" in err()
    full = [q] * 5
    assert window(full, d_=d + 1, ldx=d + 1, lds=d + 1) == -1 and b"H (p + 2) + 3" in err()
    for bp, bh in ((0, 7), (65, 7), (5, 0), (5, 65)):
        bd = R.dim(bp, bh)
        assert window(full, d_=bd, ldx=bd, lds=bd, ldz=max(bp, 1), p_=bp, H_=bh) == -1
        assert b"64" in err()
    for kw in (dict(n=0), dict(N_=0, B=0), dict(ldx=d - 1), dict(ldz=p - 1), dict(lds=d - 1)):
        assert window(full, **kw) == -1 and b"sizes" in err()
    for B in (0, -3, 10):
        assert window(full, B=B) == -1 and b"1 <= B <= N" in err()
    # the cursor's advance
    assert lib.dsvgd_window_advance(None, 4, 9, None) == -1 and b"null" in err()
    for B, N_ in ((0, 9), (10, 9), (1, 0), (-1, 9)):
        assert lib.dsvgd_window_advance(q, B, N_, None) == -1 and b"1 <= B <= N" in err()


def test_update64_follows_the_rule_and_the_sentinel():
    X = np.array([[1.0, -2.0], [0.5, 3.0]])
    P = np.array([[0.3, -0.4], [2.0, 0.0]])
    G = np.array([[-1.0, 0.25], [-1.0, -1.0]])
    Xn, Gn = A.update64(X, P, G, 0.1, 0.9, 1e-6)
    assert Gn[0, 0] == 0.3 ** 2 and Gn[1, 0] == 4.0 and Gn[1, 1] == 0.0
    assert abs(Gn[0, 1] - (0.9 * 0.25 + 0.1 * 0.16)) < 1e-15
    assert abs(Xn[0, 0] - (1.0 + 0.1 * 0.3 / (1e-6 + 0.3))) < 1e-15
    assert Xn[1, 1] == 3.0     # p = 0: no move, no 0 / 0


def test_minibatch_score64_matches_fp64_autograd_of_the_weighted_density():
    n, N, p, H, B, c = 3, 11, 3, 2, 4, 9      # the window wraps: rows 9, 10, 0, 1
    X, Z, y = R.problem(n, N, p, H, seed=4)
    rows = A.window(N, B, c)
    assert rows.tolist() == [9, 10, 0, 1]
    tgt = _target(Z, y, H, a0=2.0, b0=0.5)
    S, Asc, bound, _ = A.minibatch_score64(X, Z, y, p, H, B, c, 2.0, 0.5)
    assert np.all(Asc > 0) and np.all(bound >= R.SCORE_TOL * Asc)
    w = N / B
    z64 = torch.from_numpy(Z[rows].astype(np.float64))
    y64 = torch.from_numpy(y[rows].astype(np.float64))
    d = tgt.d

    def weighted(x):
        W1, b1, w2, b2, lg, ll = tgt.unpack(x)
        r = y64 - (torch.relu(z64 @ W1 + b1) @ w2 + b2)
        th = x[:-2]
        lik = 0.5 * B * lg - 0.5 * torch.exp(lg) * (r * r).sum()
        prior = (0.5 * (d - 2) * ll - 0.5 * torch.exp(ll) * (th * th).sum()
                 + tgt.a0 * lg - tgt.b0 * torch.exp(lg) + tgt.a0 * ll - tgt.b0 * torch.exp(ll))
        return w * lik + prior
    for i in range(n):
        x = torch.from_numpy(X[i].astype(np.float64)).requires_grad_(True)
        (g,) = torch.autograd.grad(weighted(x), x)
        assert np.all(np.abs(g.numpy() - S[i]) <= 1e-12 * Asc[i])
    # B = N, any origin: the full-data score
    full = R.score64(X, Z, y, p, H, 2.0, 0.5)
    whole = A.minibatch_score64(X, Z, y, p, H, N, 5, 2.0, 0.5)
    assert np.all(np.abs(whole[0] - full[0]) <= 1e-12 * full[1])
    assert np.all(np.abs(whole[1] - full[1]) <= 1e-12 * full[1])
