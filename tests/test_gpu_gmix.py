"""GPU tests of the Gaussian-mixture target: the score kernel and its
evaluation twin against the fp64 closed form of tests/gmix_reference.py at
their edges (one particle, one component, d = 1, d either side of the engine's
direct path, K and d that are no multiple of any tile, K beyond one LDS tile,
d = 1024), particles far from every mode, the online softmax with the dominant
component first, last and at a tile boundary, duplicated components, strided
views, the scale and row calls (bit-identical to the batched call), the two
metrics, the target through Sampler (both orders, graphs on and off, IMQ with
KSD records) and DistSampler, mode coverage, and the experiment.

The bounds are those of tests/gmix_reference.py, which tests/test_gmix_host.py
shows an fp32 restatement of the kernel to meet on these same problems:
|S - S64| <= 1e-5 A + B and the log density's.  Trajectories: 1e-4 absolute,
as tests/test_gpu_bnn.py."""
import functools

import numpy as np
import pytest
import torch

import gmix_reference as R
from conftest import record_parity
from oracle import svgd_oracle as O

pytestmark = pytest.mark.gpu
TRAJ_TOL = 1e-4
DEV = "cuda:0"


def dsvgd():
    import dsvgd as m
    return m


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _target(means, lam, w):
    return dsvgd().targets.GaussianMixture(torch.from_numpy(means), torch.from_numpy(lam),
                                           torch.from_numpy(w))


def _frozen(prob):
    ev = R.evaluate64(*prob)
    for a in tuple(prob) + tuple(v for v in ev.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return prob, ev


@functools.lru_cache(maxsize=None)
def _case(i):
    """Problem i of R.SHAPES and its fp64 evaluation (computed once, shared and
    left unchanged); the seeds are those of tests/test_gmix_host.py."""
    n, K, d, spread, far = R.SHAPES[i]
    return _frozen(R.problem(n, K, d, spread, 100 + i, far))


@functools.lru_cache(maxsize=None)
def _edge(pos):
    return _frozen(R.edge_problem(pos))


@functools.lru_cache(maxsize=None)
def _assign_case():
    return _frozen(R.problem(257, 9, 6, 1.5, 31))


def _check_score(got, ev, scale=1.0):
    assert np.isfinite(got).all()
    err = np.abs(np.asarray(got, np.float64) - scale * ev["S"])
    over_a = float((err / (abs(scale) * R.SCORE_TOL * ev["A"])).max())
    over_b = float((err / (abs(scale) * ev["score_bound"])).max())
    print("worst err/(1e-5 A) %.3g, err/bound %.3g" % (over_a, over_b))
    record_parity(over_a * R.SCORE_TOL)
    assert np.all(err <= abs(scale) * ev["score_bound"])


def _check_logp(got, ev):
    assert np.isfinite(got).all()
    err = np.abs(np.asarray(got, np.float64) - ev["logp"])
    print("logp worst err/bound %.3g" % float((err / ev["logp_bound"]).max()))
    assert np.all(err <= ev["logp_bound"])


def _score(prob, scale=1.0):
    X, means, lam, w = prob
    Xg = gpu(X)
    out = torch.full_like(Xg, float("nan"))
    _target(means, lam, w).score(Xg, out, scale)
    return out.cpu().numpy()


# ---------------------------------------------------------------- score --
@pytest.mark.parametrize("i", range(len(R.SHAPES)), ids=lambda i: "n%d-K%d-d%d" % R.SHAPES[i][:3])
def test_score_and_logp_match_fp64(i):
    prob, ev = _case(i)
    _check_score(_score(prob), ev)
    tgt = _target(*prob[1:])
    lp, comp = tgt.assign(gpu(prob[0]))
    assert lp.shape == (len(prob[0]),) and comp.dtype == torch.int32
    _check_logp(lp.cpu().numpy(), ev)
    arg, must = R.decided(ev)
    assert np.array_equal(comp.cpu().numpy()[must], arg[must])


def test_far_particles_stay_finite():
    """Every third particle is 40 away from every mode in every coordinate:
    all of its exponents are below fp32's exp range (a condition on the
    inputs, asserted), and its score is finite and within the bound."""
    i = [s[4] for s in R.SHAPES].index(True)
    prob, ev = _case(i)
    far = np.arange(len(prob[0])) % 3 == 0
    assert (ev["l"][far] < -87.0).all() and (ev["l"][~far].max(1) > -87.0).all()
    got = _score(prob)
    assert np.isfinite(got[far]).all() and (np.abs(got[far]) > 1.0).all()
    _check_score(got, ev)
    _check_logp(dsvgd().metrics.gmix_logp(gpu(prob[0]), _target(*prob[1:])).cpu().numpy(), ev)


@pytest.mark.parametrize("pos", R.EDGE_POSITIONS)
def test_online_softmax_with_the_dominant_component_anywhere(pos):
    """The component the particles were drawn from at the first place, the
    last, and either side of a tile boundary: every order is the same mixture,
    so each result is within the bound of ONE fp64 evaluation."""
    _, ev = _edge(R.EDGE_POSITIONS[0])
    prob, own = _edge(pos)
    assert (own["r"][:, pos] > 0.5).all()                 # it is the dominant one
    assert np.abs(own["S"] - ev["S"]).max() <= 1e-12 * ev["A"].max()
    _check_score(_score(prob), ev)
    lp, comp = _target(*prob[1:]).assign(gpu(prob[0]))
    _check_logp(lp.cpu().numpy(), ev)
    assert (comp.cpu().numpy() == pos).all()


def test_two_equal_components_are_one_of_twice_the_weight():
    split, merged = R.duplicate_problem()
    ev_split, ev = R.evaluate64(*split), R.evaluate64(*merged)
    assert np.abs(ev_split["S"] - ev["S"]).max() <= 1e-12 * ev["A"].max()
    got = _score(split)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ev["S"])
    record_parity(float((err / ev["A"]).max()))
    assert np.all(err <= ev_split["score_bound"])
    _check_score(_score(merged), ev)
    # an exact tie (the twin is the last component): the lower index wins
    K = len(split[3])
    comp = _target(*split[1:]).assign(gpu(split[0]))[1].cpu().numpy()
    assert not (comp == K - 1).any() and (comp == 0).any()
    assert (ev_split["l"][:, 0] == ev_split["l"][:, K - 1]).all()


def test_views_scale_and_row_calls():
    i = 3
    prob, ev = _case(i)
    X = prob[0]
    n, d = X.shape
    assert n > 128 and d % 4 != 0
    tgt = _target(*prob[1:])
    wide_x = torch.full((n, d + 9), float("nan"), device=DEV)
    wide_o = torch.full((n, d + 5), float("nan"), device=DEV)
    Xv, Ov = wide_x[:, 3:3 + d], wide_o[:, 2:2 + d]
    Xv.copy_(gpu(X))
    tgt.score(Xv, Ov, scale=2.5)
    first = wide_o.cpu().numpy().copy()
    _check_score(first[:, 2:2 + d], ev, scale=2.5)
    assert np.isnan(first[:, :2]).all() and np.isnan(first[:, 2 + d:]).all()
    assert np.isnan(wide_x[:, :3].cpu().numpy()).all()
    assert np.isnan(wide_x[:, 3 + d:].cpu().numpy()).all()
    tgt.score(Xv, Ov, scale=2.5)
    assert wide_o.cpu().numpy().tobytes() == first.tobytes()
    # the contiguous call gives the view's bits
    plain = torch.empty(n, d, device=DEV)
    tgt.score(gpu(X), plain, scale=2.5)
    assert plain.cpu().numpy().tobytes() == np.ascontiguousarray(first[:, 2:2 + d]).tobytes()
    # one row, and a run of rows that starts inside a workgroup: the same bits
    rows = torch.full((n, d + 5), float("nan"), device=DEV)
    for j in (0, 17, n - 1):
        tgt.score(Xv[j:j + 1], rows[j:j + 1, 2:2 + d], scale=2.5)
        assert rows[j].cpu().numpy().tobytes() == first[j].tobytes()
    a, b = 41, 118
    rows.fill_(float("nan"))
    tgt.score(Xv[a:b], rows[a:b, 2:2 + d], scale=2.5)
    assert rows[a:b].cpu().numpy().tobytes() == first[a:b].tobytes()
    lp = tgt.assign(gpu(X))[0]
    assert torch.equal(tgt.assign(Xv[a:b])[0], lp[a:b])
    assert torch.equal(tgt.assign(Xv)[0], lp)


# -------------------------------------------------------------- metrics --
def test_gmix_logp_and_mode_shares():
    prob, ev = _assign_case()
    X, means, lam, w = prob
    M = dsvgd().metrics
    tgt = _target(means, lam, w)
    lp = M.gmix_logp(gpu(X), tgt)
    assert lp.shape == (len(X),) and lp.device.type == "cuda" and lp.dtype == torch.float32
    _check_logp(lp.cpu().numpy(), ev)
    assert torch.equal(M.gmix_logp(X, tgt), lp)              # host arrays too
    arg, must = R.decided(ev)
    print("particles too close to call: %d of %d" % (int((~must).sum()), len(must)))
    assert (~must).mean() <= 0.01
    comp = tgt.assign(gpu(X))[1].cpu().numpy()
    assert np.array_equal(comp[must], arg[must])
    shares = M.mode_shares(gpu(X), tgt)
    assert shares.shape == (tgt.K,) and shares.device.type == "cuda"
    want = np.bincount(comp, minlength=tgt.K) / len(X)
    assert np.array_equal(shares.cpu().numpy(), want)
    assert abs(float(shares.sum()) - 1.0) <= 1e-12
    if must.all():
        assert np.array_equal(want, np.bincount(arg, minlength=tgt.K) / len(X))
    with pytest.raises(ValueError):
        M.mode_shares(gpu(X), dsvgd().targets.GaussianMixture1D())
    with pytest.raises(ValueError):
        M.gmix_logp(gpu(X)[:, :3], tgt)


# ------------------------------------------------------------- samplers --
def _values(df, shape):
    return np.stack(df["value"].to_list()).reshape(shape)


def _sampler_problem(K=3, d=5, seed=41):
    _, means, lam, w = R.problem(1, K, d, 2.0, seed)
    return means, lam, w, (lambda X: R.evaluate64(X, means, lam, w)["S"])


def _traj_err(got, ref):
    e = float(np.abs(np.asarray(got, np.float64) - ref).max())
    record_parity(e)
    return e


def test_sampler_jacobi_matches_fp64_graphs_on_and_off():
    n, d, T, eps = 130, 5, 3, 0.1
    means, lam, w, score = _sampler_problem(3, d)
    m = dsvgd()
    out = {}
    for graphs in (True, False):
        torch.manual_seed(5)
        s = m.Sampler(d, _target(means, lam, w), m.RBF(float(d)))
        df = s.sample(n, T, eps, order="jacobi", device=DEV, verbose=False, graphs=graphs)
        out[graphs] = _values(df, (T + 1, n, d))
    assert out[True].tobytes() == out[False].tobytes()
    ref = O.sampler_jacobi(out[True][0], score, float(d), T, eps)
    assert _traj_err(out[True], ref) < TRAJ_TOL
    assert np.abs(ref[-1] - ref[0]).max() > 100 * TRAJ_TOL


def test_sampler_sequential_matches_fp64():
    n, d, T, eps = 33, 5, 2, 0.1
    means, lam, w, score = _sampler_problem(3, d)
    m = dsvgd()
    torch.manual_seed(6)
    s = m.Sampler(d, _target(means, lam, w), m.RBF(float(d)))
    df = s.sample(n, T, eps, order="sequential", device=DEV, verbose=False)
    vals = _values(df, (T + 1, n, d))
    ref = O.sampler_sequential(vals[0], score, float(d), T, eps)
    assert _traj_err(vals, ref) < TRAJ_TOL
    assert np.abs(ref[-1] - ref[0]).max() > 100 * TRAJ_TOL


def test_sampler_imq_with_ksd_records_stays_finite():
    n, d, T = 130, 5, 3
    means, lam, w, _ = _sampler_problem(3, d)
    m = dsvgd()
    torch.manual_seed(7)
    s = m.Sampler(d, _target(means, lam, w), m.IMQ("median", -0.5))
    df = s.sample(n, T, 0.1, order="jacobi", device=DEV, verbose=False, ksd_every=1)
    assert list(s.diagnostics.timestep) == [0, 1, 2, 3]
    assert np.isfinite(s.diagnostics.ksd.to_numpy()).all() and (s.diagnostics.ksd > 0).all()
    assert np.isfinite(_values(df, (T + 1, n, d))).all()


def test_distsampler_one_jacobi_step_matches_fp64():
    n, d, eps = 130, 5, 0.1
    means, lam, w, score = _sampler_problem(3, d)
    X = np.random.RandomState(12).randn(n, d).astype(np.float32)
    m = dsvgd()
    ds = m.DistSampler(0, 1, _target(means, lam, w), m.RBF(float(d)), gpu(X).clone(), 1, 1, False,
                       False, False, order="jacobi")
    ds.make_step(eps)
    torch.cuda.synchronize()
    ref = O.sampler_jacobi(X, score, float(d), 1, eps)
    assert _traj_err(ds.particles.cpu().numpy(), ref[1]) < TRAJ_TOL
    assert np.abs(ref[1] - ref[0]).max() > 100 * TRAJ_TOL


def test_mode_coverage():
    """The point of the target: from N(0, I) between three unit-variance
    modes 6 apart (weights 0.5, 0.3, 0.2), 300 Jacobi steps under a graph
    leave particles on every mode and raise the mean log density.  The shares
    themselves are printed, not bounded."""
    c = 2.0 * np.sqrt(3.0)       # the modes on a circle of this radius are 6 apart
    ang = np.deg2rad([90.0, 210.0, 330.0])
    means = np.stack([c * np.cos(ang), c * np.sin(ang)], 1).astype(np.float32)
    gaps = np.linalg.norm(means[:, None] - means[None], axis=2)[np.triu_indices(3, 1)]
    assert np.allclose(gaps, 6.0, atol=1e-5)
    m = dsvgd()
    tgt = m.targets.GaussianMixture(means, 1.0, [0.5, 0.3, 0.2])
    n, T = 512, 300
    torch.manual_seed(8)
    s = m.Sampler(2, tgt, m.RBF("median"))
    df = s.sample(n, T, 0.3, order="jacobi", device=DEV, verbose=False, graphs=True)
    hist = _values(df, (T + 1, n, 2))
    assert np.isfinite(hist).all()
    shares = m.metrics.mode_shares(gpu(hist[-1]), tgt).cpu().numpy()
    lp0 = float(m.metrics.gmix_logp(gpu(hist[0]), tgt).double().mean())
    lp1 = float(m.metrics.gmix_logp(gpu(hist[-1]), tgt).double().mean())
    print("shares %s against weights %s; mean logp %.4f -> %.4f"
          % (shares.round(4).tolist(), tgt.weights.tolist(), lp0, lp1))
    assert (shares > 0).all()
    assert lp1 > lp0


def test_experiment_runs_end_to_end():
    from click.testing import CliRunner

    from test_gmix_host import experiment
    E = experiment()
    res = CliRunner().invoke(E.cli, ['--d', '3', '--modes', '4', '--spread', '3', '--nparticles',
                                     '24', '--niter', '4', '--every', '2', '--order', 'jacobi',
                                     '--kernel', 'imq', '--seed', '1'])
    assert res.exit_code == 0, res.output
    lines = res.output.strip().splitlines()
    assert lines[0].startswith("weights [0.250 0.250 0.250 0.250]")
    assert [ln.split()[1] for ln in lines[1:4]] == ["0", "2", "4"]
    assert lines[-1].startswith("final ksd") and np.isfinite(float(lines[-1].split()[-1]))
    curve, ksd = E.run(16, 2, 1.0, 1, out=lambda s: None)     # the reference's model, d = 1
    assert [r["iteration"] for r in curve] == [0, 1, 2]
    assert all(abs(sum(r["shares"]) - 1.0) < 1e-12 and np.isfinite(r["logp"]) for r in curve)
    assert np.isfinite(ksd) and ksd >= 0
