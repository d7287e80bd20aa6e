"""Host-side checks of the Gaussian-mixture target (no GPU): the fp64 closed
form of tests/gmix_reference.py against fp64 autograd of GaussianMixture.logp
and against torch.distributions, its special cases against the oracle, the
target's validation and digest, the argument checks of its two entry points,
the experiment's seeded problem, and that an fp32 restatement of the kernel
stays within the bounds of tests/gmix_reference.py on every problem the GPU
tests use (so the inputs are known to be feasible before a GPU sees them)."""
import ctypes

import numpy as np
import pytest
import torch

import gmix_reference as R
from oracle import svgd_oracle as O


def _target(means, lam=1.0, w=None):
    from dsvgd.targets import GaussianMixture
    return GaussianMixture(means, lam, w)


def test_closed_form_matches_fp64_autograd_of_logp():
    X, means, lam, w = R.problem(6, 5, 7, 1.0, seed=1)
    tgt = _target(means, lam, w)
    assert (tgt.K, tgt.d) == (5, 7)
    ev = R.evaluate64(X, means, lam, w)
    Xt = torch.from_numpy(X.astype(np.float64))
    for i in range(len(X)):
        x = Xt[i].clone().requires_grad_(True)
        lp = tgt.logp(x)
        (g,) = torch.autograd.grad(lp, x)
        assert lp.dtype == torch.float64 and lp.shape == ()
        assert abs(float(lp) - ev["logp"][i]) <= 1e-12 * (abs(ev["logp"][i]) + 1)
        assert np.all(np.abs(g.numpy() - ev["S"][i]) <= 1e-12 * ev["A"][i])
    # a reference-style callable that batches under vmap(grad), in the caller's dtype
    assert tgt(Xt[0]) == tgt.logp(Xt[0])
    assert tgt.logp(torch.from_numpy(X[0])).dtype == torch.float32
    g = torch.func.vmap(torch.func.grad(tgt.logp))(Xt).numpy()
    assert np.all(np.abs(g - ev["S"]) <= 1e-12 * ev["A"])


def test_logp_matches_torch_distributions():
    from torch.distributions import Categorical, Independent, MixtureSameFamily, Normal
    X, means, lam, w = R.problem(9, 4, 3, 2.0, seed=2)
    mu, prec, wt = (torch.from_numpy(a.astype(np.float64)) for a in (means, lam, w))
    mix = MixtureSameFamily(Categorical(probs=wt / wt.sum()),
                            Independent(Normal(mu, prec.rsqrt()), 1))
    want = mix.log_prob(torch.from_numpy(X.astype(np.float64))).numpy()
    ev = R.evaluate64(X, means, lam, w)
    assert np.all(np.abs(ev["logp"] - want) <= 1e-12 * (np.abs(want) + 1))
    tgt = _target(means, lam, w)
    got = np.array([float(tgt.logp(torch.from_numpy(x.astype(np.float64)))) for x in X])
    assert np.all(np.abs(got - want) <= 1e-12 * (np.abs(want) + 1))
    assert torch.allclose(tgt.weights, wt / wt.sum(), rtol=1e-15, atol=0)


def test_one_component_is_the_gaussian_score():
    X, means, lam, w = R.problem(7, 1, 5, 1.0, seed=3)
    ev = R.evaluate64(X, means, lam, w)
    want = O.score_gaussian(X, means[0], lam[0])
    assert np.all(np.abs(ev["S"] - want) <= 1e-14 * ev["A"])
    assert np.all(ev["score_bound"] == R.SCORE_TOL * ev["A"])     # B vanishes for K = 1


def test_two_unit_modes_agree_with_the_1d_mixture():
    X = np.linspace(-6, 6, 41).reshape(-1, 1).astype(np.float32)
    means = np.array([[-2.0], [2.0]], np.float32)
    ev = R.evaluate64(X, means, np.ones_like(means), np.ones(2, np.float32))
    assert np.all(np.abs(ev["S"] - O.score_gmm(X)) <= 1e-13 * ev["A"])
    from dsvgd.targets import GaussianMixture1D
    tgt, old = _target(means), GaussianMixture1D()
    for x in torch.from_numpy(X.astype(np.float64)):
        # the 1-D target keeps the reference's unnormalised 1/3 weights
        assert abs(float(tgt.logp(x)) - float(old.logp(x)) - np.log(1.5)) <= 1e-12


def test_constructor_refusals():
    means = np.zeros((3, 4), np.float32)
    for bad in (np.zeros(4), np.zeros((3, 4, 1)), np.zeros((0, 4)), np.zeros((3, 0))):
        with pytest.raises(ValueError):
            _target(bad)
    bad_means = means.copy()
    bad_means[1, 2] = np.inf
    with pytest.raises(ValueError):
        _target(bad_means)
    for lam in (0.0, -1.0, float("nan"), float("inf"), np.ones((2, 4)), np.ones((3, 5)),
                np.array([1.0, 1.0, 0.0, 1.0])):
        with pytest.raises(ValueError):
            _target(means, lam)
    for w in (np.ones(2), np.ones((3, 1)), [1.0, 0.0, 1.0], [1.0, -2.0, 1.0],
              [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0]):
        with pytest.raises(ValueError):
            _target(means, 1.0, w)
    # what broadcasts to (K, d) is accepted: a scalar, a row, a column
    for lam in (2.0, np.full(4, 2.0), np.full((3, 1), 2.0)):
        assert torch.equal(_target(means, lam).precisions, torch.full((3, 4), 2.0))
    from dsvgd.targets import GaussianMixture
    assert GaussianMixture.MAX_D >= 1024
    _target(np.zeros((1, GaussianMixture.MAX_D), np.float32))
    with pytest.raises(ValueError):
        _target(np.zeros((1, GaussianMixture.MAX_D + 1), np.float32))
    tgt = _target(means)
    assert torch.equal(tgt.weights, torch.full((3,), 1.0 / 3.0, dtype=torch.float64))
    with pytest.raises(ValueError):
        tgt.logp(torch.zeros(5))
    with pytest.raises(AssertionError):
        tgt.score(torch.zeros(2, 5), torch.zeros(2, 5))


def test_fingerprint_follows_every_parameter():
    _, means, lam, w = R.problem(1, 4, 3, 1.0, seed=4)
    fp = _target(means, lam, w).fingerprint()
    assert _target(means.copy(), lam.copy(), w.copy()).fingerprint() == fp
    for which in range(3):
        args = [means.copy(), lam.copy(), w.copy()]
        flat = args[which].reshape(-1)
        flat[1] = np.nextafter(flat[1], np.float32(9))
        assert _target(*args).fingerprint() != fp
    assert _target(means[:3], lam[:3], w[:3]).fingerprint() != fp
    # the same bytes in another shape are another mixture
    assert _target(np.zeros((2, 6), np.float32)).fingerprint() != \
        _target(np.zeros((2, 3), np.float32)).fingerprint()
    assert _target(np.zeros((2, 6), np.float32)).fingerprint() != \
        _target(np.zeros((3, 4), np.float32), 1.0, [0.5, 0.25, 0.25]).fingerprint()
    if torch.cuda.is_available():   # the digest is of the values, wherever they live
        dev = _target(torch.from_numpy(means).cuda(), torch.from_numpy(lam).cuda(),
                      torch.from_numpy(w).cuda())
        assert dev.fingerprint() == fp


def test_engine_takes_the_per_row_path():
    from dsvgd.engine import _gs_score_kind
    assert _gs_score_kind(_target(np.zeros((2, 3), np.float32))) is None


def test_library_exports_the_gmix_entry_points_and_abi_stays_4():
    from dsvgd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("dsvgd_score_gmix", "dsvgd_gmix_assign"):
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES
    assert _native.ABI_VERSION == 4 and _native.load().dsvgd_abi_version() == 4


def test_entry_points_validate_arguments_without_gpu():
    """Every call below fails a check: none reaches a launch."""
    from dsvgd import _native as N
    lib = N.load()
    buf = (ctypes.c_double * 64)()
    q = ctypes.addressof(buf)
    d, K = 5, 3

    def err():
        return lib.dsvgd_last_error()

    def score(X=q, ldx=d, n=2, d_=d, mu=q, ldm=d, lam=q, ldl=d, c=q, K_=K, S=q, lds=d):
        return lib.dsvgd_score_gmix(X, ldx, n, d_, mu, ldm, lam, ldl, c, K_, 1.0, S, lds, None)

    def assign(X=q, ldx=d, n=2, d_=d, mu=q, ldm=d, lam=q, ldl=d, c=q, K_=K, lp=q, comp=q):
        return lib.dsvgd_gmix_assign(X, ldx, n, d_, mu, ldm, lam, ldl, c, K_, lp, comp, None)

    for name in ("X", "mu", "lam", "c", "S"):
        assert score(**{name: None}) == -1 and b"null" in err()
    for name in ("X", "mu", "lam", "c", "lp", "comp"):
        assert assign(**{name: None}) == -1 and b"null" in err()
    for fn in (score, assign):
        for bad_d in (0, -1, 1025):
            assert fn(d_=bad_d, ldx=2000, ldm=2000, ldl=2000) == -1 and b"1 <= d <= 1024" in err()
        for bad_K in (0, -3, 2 ** 30 + 1):
            assert fn(K_=bad_K) == -1 and b"K" in err()
        for kw in ({"n": 0}, {"n": -1}, {"n": 2 ** 31}, {"ldx": d - 1}, {"ldm": d - 1},
                   {"ldl": d - 1}):
            assert fn(**kw) == -1 and b"sizes" in err()
    assert score(lds=d - 1) == -1 and b"sizes" in err()


def experiment():
    import importlib.util
    import os

    from conftest import PKG
    spec = importlib.util.spec_from_file_location(
        "dsvgd_gmm_experiment", os.path.join(PKG, "experiments", "gmm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_experiment_problem_is_seeded_and_its_help_lists_the_options():
    E = experiment()
    means, lam, w = E.mixture()
    assert means.tolist() == [[-2.0], [2.0]] and lam.tolist() == [[1.0], [1.0]]
    assert w.tolist() == [0.5, 0.5]
    a, b = E.mixture(4, 5, 6.0, seed=3), E.mixture(4, 5, 6.0, seed=3)
    assert a[0].shape == (5, 4) and a[0].dtype == np.float32
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(E.mixture(4, 5, 6.0, seed=4)[0], a[0])
    assert np.array_equal(E.mixture(3, 2, 1.5)[0], [[-1.5, 0, 0], [1.5, 0, 0]])
    from click.testing import CliRunner
    res = CliRunner().invoke(E.cli, ['--help'])
    assert res.exit_code == 0
    for opt in ('--d', '--modes', '--spread', '--nparticles', '--niter', '--stepsize', '--order',
                '--kernel', '--every', '--seed'):
        assert opt in res.output
    # the reference's run is the default
    defaults = {p.name: p.default for p in E.cli.params}
    assert (defaults["d"], defaults["modes"], defaults["spread"]) == (1, 2, 2.0)
    assert (defaults["nparticles"], defaults["niter"], defaults["stepsize"]) == (50, 500, 1.0)
    assert defaults["kernel"] == "rbf"


# ---- the fp32 restatement against the bounds, on the GPU tests' problems --
def _gpu_problems():
    for i, (n, K, d, spread, far) in enumerate(R.SHAPES):
        yield "shape%d" % i, R.problem(n, K, d, spread, 100 + i, far)
    for pos in R.EDGE_POSITIONS:
        yield "edge%d" % pos, R.edge_problem(pos)
    split, merged = R.duplicate_problem()
    yield "split", split
    yield "merged", merged
    yield "assign", R.problem(257, 9, 6, 1.5, 31)


@pytest.mark.parametrize("name", [name for name, _ in _gpu_problems()])
def test_fp32_restatement_stays_within_both_bounds(name):
    prob = dict(_gpu_problems())[name]
    ev = R.evaluate64(*prob)
    arg, must = R.decided(ev)
    for pairwise in (False, True):
        S, logp, comp = R.fp32_restatement(*prob, pairwise=pairwise)
        assert np.isfinite(S).all() and np.isfinite(logp).all()
        es = np.abs(S.astype(np.float64) - ev["S"])
        el = np.abs(logp.astype(np.float64) - ev["logp"])
        print("%s pairwise=%d: score err/(1e-5 A) %.3g, err/bound %.3g; logp err/bound %.3g"
              % (name, pairwise, (es / (R.SCORE_TOL * ev["A"])).max(),
                 (es / ev["score_bound"]).max(), (el / ev["logp_bound"]).max()))
        assert np.all(es <= ev["score_bound"])
        assert np.all(el <= ev["logp_bound"])
        assert np.array_equal(comp[must], arg[must])
        if name == "split":     # exact ties by construction: the lower index wins
            assert not (comp == len(prob[3]) - 1).any()
    if name != "split":
        assert must.mean() >= 0.99
