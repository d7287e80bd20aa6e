"""GPU tests of the softmax-regression target (csrc/softmax.hip) against the
fp64 closed form of tests/softmax_reference.py: both forms at their edges (the
table there), missing and single classes, the minibatch window at its origins,
strided views and the scale, determinism, large logits, the two-class case
against LogisticRegression, the metrics, and the target through Sampler (both
orders, graphs on and off, minibatches, IMQ with KSD records), DistSampler,
metrics.ksd and the experiment.

The bound, per entry and with none left out: |S - S64| <= 1e-5 A, A the sum of
the absolute values of the entry's terms (tests/test_softmax_host.py shows an
fp32 restatement of the kernel to stay under a tenth of it on these same
problems).  Trajectories: 1e-4 absolute, as tests/test_gpu_gmix.py."""
import functools

import numpy as np
import pytest
import torch

import softmax_reference as R
from conftest import record_parity
from oracle import svgd_oracle as O
from test_softmax_host import case, experiment

pytestmark = pytest.mark.gpu
TRAJ_TOL = 1e-4
EXPERIMENT_ACC64 = 1.0       # test_experiment_runs_end_to_end's fp64 CPU run (30 of 30 test rows)
DEV = "cuda:0"


def dsvgd():
    import dsvgd as m
    return m


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _target(Xd, y, C, **kw):
    return dsvgd().targets.SoftmaxRegression(torch.from_numpy(np.array(Xd)),
                                             torch.from_numpy(np.array(y)), classes=C, **kw)


def _check(got, S, A, scale=1.0):
    assert np.isfinite(got).all()
    err = np.abs(np.asarray(got, np.float64) - scale * S)
    worst = float((err / (abs(scale) * A)).max())
    print("worst err/A %.3g" % worst)
    record_parity(worst)
    assert np.all(err <= abs(scale) * R.SCORE_TOL * A)
    return worst


def _score(tgt, X, scale=1.0, **kw):
    Xg = gpu(X)
    out = torch.full_like(Xg, float("nan"))
    tgt.score(Xg, out, scale, **kw)
    return out.cpu().numpy()


# ---------------------------------------------------------------- score --
@pytest.mark.parametrize("i", range(len(R.SHAPES)), ids=lambda i: "n%d-N%d-C%d-p%d" % R.SHAPES[i])
def test_score_matches_fp64(i):
    C = R.SHAPES[i][2]
    (X, Xd, y), S, A = case(i)
    _check(_score(_target(Xd, y, C), X), S, A)


@pytest.mark.parametrize("labels", ["missing", "single"])
@pytest.mark.parametrize("n", [9, 40])
def test_a_class_that_never_occurs_and_a_single_class(labels, n):
    N, C, p = 70, 4, 9
    X, Xd, y = R.problem(n, N, C, p, 7, labels=labels)
    assert (y != 1).all() and (labels == "missing" or (y == C - 1).all())
    S, A = R.score64(X, Xd, y, C)
    _check(_score(_target(Xd, y, C), X), S, A)


def test_other_hyper_priors_reach_the_kernels():
    for n in (5, 40):
        X, Xd, y = R.problem(n, 50, 3, 6, 8)
        S, A = R.score64(X, Xd, y, 3, 2.5, 0.25)
        _check(_score(_target(Xd, y, 3, a0=2.5, b0=0.25), X), S, A)


# --------------------------------------------------------------- window --
@functools.lru_cache(maxsize=None)
def _window_case(n):
    """B < N = 3 B + 7; the rows outside the window of each origin are 1e3 *
    randn in the copy scored for that origin."""
    B, C, p = 40, 5, 11
    N = 3 * B + 7
    X, Xd, y = R.problem(n, N, C, p, 21)
    out = {}
    for org in R.origins(N, B):
        xd = np.array(Xd)
        outside = np.setdiff1d(np.arange(N), R.window_rows(N, org, B))
        xd[outside] = 1e3 * np.random.RandomState(org).randn(len(outside), p)
        S, A = R.score64(X, xd, y, C, origin=org, B=B)
        # any one outside row joining the sum would break the bound: its
        # term (N/B) G_qc xd_qk is above 10 x 1e-5 A in some entry of some particle
        W = X[:, 1:].reshape(n, C, p).astype(np.float64)
        G = -R.softmax64(np.einsum("qk,ick->iqc", xd[outside], W))
        G[:, np.arange(len(outside)), y[outside]] += 1.0
        term = (N / B) * np.abs(G[:, :, :, None] * xd[outside][None, :, None, :])
        over = term.reshape(n, len(outside), C * p) / A[:, None, 1:]
        assert (over.max((0, 2)) > 10 * R.SCORE_TOL).all()
        out[org] = (xd.astype(np.float32), S, A)
    return (X, y, N, B, C), out


@pytest.mark.parametrize("n", [7, 70])
def test_window_at_its_origins(n):
    (X, y, N, B, C), cases = _window_case(n)
    assert sorted(cases) == sorted({0, N - B, N - B + 1, N - 1})
    for org, (xd, S, A) in cases.items():
        tgt = _target(xd, y, C, batch=B)
        tgt._origin = org            # where the cursor starts: any row, not only a multiple of B
        _check(_score(tgt, X), S, A)
        assert int(tgt._cursor[torch.device(DEV)][0]) == org


def test_next_batch_matches_reset_batch():
    n, N, B, C, p = 40, 127, 40, 3, 6
    X, Xd, y = R.problem(n, N, C, p, 22)
    walk, jump = _target(Xd, y, C, batch=B), _target(Xd, y, C, batch=B)
    for t in range(5):          # wraps after the third window
        S, A = R.score64(X, Xd, y, C, origin=(t * B) % N, B=B)
        a = _score(walk, X)
        jump.reset_batch(t)
        b = _score(jump, X)
        assert a.tobytes() == b.tobytes()
        _check(a, S, A)
        walk.next_batch()
    S, A = R.score64(X, Xd, y, C)
    _check(_score(walk.full, X), S, A)          # the full-data twin


# ---------------------------------------------------------------- views --
@pytest.mark.parametrize("i", [2, 6], ids=["tile-small", "tile-ragged"])
def test_views_and_scale(i):
    C = R.SHAPES[i][2]
    (X, Xd, y), S, A = case(i)
    n, d = X.shape
    tgt = _target(Xd, y, C)
    wide_x = torch.full((n, d + 9), float("nan"), device=DEV)
    wide_o = torch.full((n, d + 5), float("nan"), device=DEV)
    Xv, Ov = wide_x[:, 3:3 + d], wide_o[:, 2:2 + d]
    Xv.copy_(gpu(X))
    tgt.score(Xv, Ov, scale=2.5)
    first = wide_o.cpu().numpy().copy()
    _check(first[:, 2:2 + d], S, A, scale=2.5)
    assert np.isnan(first[:, :2]).all() and np.isnan(first[:, 2 + d:]).all()
    tgt.score(Xv, Ov, scale=2.5)
    assert wide_o.cpu().numpy().tobytes() == first.tobytes()
    plain = torch.empty(n, d, device=DEV)
    tgt.score(gpu(X), plain, scale=2.5)
    assert plain.cpu().numpy().tobytes() == np.ascontiguousarray(first[:, 2:2 + d]).tobytes()
    # the row form on views
    rows = torch.full((R.SMALL_ROWS, d + 5), float("nan"), device=DEV)
    tgt.score(Xv[:R.SMALL_ROWS], rows[:, 2:2 + d], scale=-0.5)
    got = rows.cpu().numpy()
    _check(got[:, 2:2 + d], S[:R.SMALL_ROWS], A[:R.SMALL_ROWS], scale=-0.5)
    assert np.isnan(got[:, :2]).all() and np.isnan(got[:, 2 + d:]).all()


# ---------------------------------------------------------- determinism --
def test_tile_form_is_deterministic_and_independent_of_the_row():
    n, N, C, p = 130, 100, 7, 54
    X, Xd, y = R.problem(n, N, C, p, 31)
    tgt = _target(Xd, y, C)
    a = _score(tgt, X)
    assert _score(tgt, X).tobytes() == a.tobytes()
    perm = np.random.RandomState(1).permutation(n)
    assert _score(tgt, X[perm]).tobytes() == np.ascontiguousarray(a[perm]).tobytes()
    # nor on the other particles: a run of rows that starts inside a workgroup
    assert _score(tgt, X[41:118]).tobytes() == np.ascontiguousarray(a[41:118]).tobytes()


def test_row_form_is_deterministic_and_a_row_call_gives_the_batch_bits():
    n, N, C, p = R.SMALL_ROWS, 100, 7, 54
    X, Xd, y = R.problem(n, N, C, p, 32)
    tgt = _target(Xd, y, C)
    a = _score(tgt, X)
    assert _score(tgt, X).tobytes() == a.tobytes()
    Xg = gpu(X)
    out = torch.full_like(Xg, float("nan"))
    for j in range(n):
        tgt.score(Xg[j:j + 1], out[j:j + 1])
    assert out.cpu().numpy().tobytes() == a.tobytes()
    # the forced row form at a tile-form n is the same kernel
    X2 = np.concatenate([X, X[:5]])
    assert _score(tgt, X2, form="rows")[:n].tobytes() == a.tobytes()


# --------------------------------------------------------- large logits --
@pytest.mark.parametrize("n", [8, 40])
def test_large_logits(n):
    N, C, p = 80, 5, 20
    X, Xd, y = R.problem(n, N, C, p, 33, wscale=64.0)
    z = np.einsum("qk,ick->iqc", Xd.astype(np.float64), X[:, 1:].reshape(n, C, p).astype(np.float64))
    assert 100 < np.abs(z).max() < 1000
    S, A = R.score64(X, Xd, y, C)
    _check(_score(_target(Xd, y, C), X), S, A)
    X3 = X.copy()
    X3[:, 1:] *= 64.0                         # logits past 1e4
    assert np.abs(z).max() * 64.0 > 1e4
    assert np.isfinite(_score(_target(Xd, y, C), X3)).all()


# --------------------------------------------------- against the logreg --
@pytest.mark.parametrize("n", [40, 8])
def test_two_classes_with_a_zero_row_are_the_logistic_regression(n):
    N, p = 90, 13
    X, Xd, y = R.problem(n, N, 2, p, 34)
    X[:, 1 + p:] = 0.0
    t = np.where(y == 0, 1.0, -1.0).astype(np.float32)
    m = dsvgd()
    Xl = np.ascontiguousarray(X[:, :1 + p])
    lr = torch.full((n, 1 + p), float("nan"), device=DEV)
    m.targets.LogisticRegression(torch.from_numpy(Xd), torch.from_numpy(t), gemm="f32").score(
        gpu(Xl), lr)
    alpha = np.exp(Xl[:, :1].astype(np.float64))
    lr_data = lr.cpu().numpy().astype(np.float64)[:, 1:] + alpha * Xl[:, 1:]
    got = _score(_target(Xd, y, 2), X).astype(np.float64)[:, 1:1 + p] + alpha * Xl[:, 1:]
    T, TA = R.data_term64(X, Xd, y, 2)
    # each side is within 1e-5 of the term's A of the fp64 term (plus the
    # rounding of the prior term taken out again)
    slack = R.SCORE_TOL * (TA[:, 0] + np.abs(alpha * Xl[:, 1:]))
    assert np.all(np.abs(got - T[:, 0]) <= slack)
    err = np.abs(got - lr_data)
    record_parity(float((err / TA[:, 0]).max()))
    assert np.all(err <= R.SCORE_TOL * TA[:, 0] + 2e-7 * np.abs(alpha * Xl[:, 1:]))


# -------------------------------------------------------------- metrics --
def test_predict_accuracy_and_loglik_match_fp64():
    n, N, C, p = 300, 150, 5, 9
    X, Xd, y = R.problem(n, N, C, p, 35, wscale=3.0)
    M = dsvgd().metrics
    tgt = _target(Xd, y, C)
    P = M.softmax_predict(gpu(X), tgt, Xd)
    assert P.shape == (N, C) and P.device.type == "cuda" and P.dtype == torch.float32
    P64 = R.predict64(X, Xd, C)
    got = P.cpu().numpy().astype(np.float64)
    record_parity(float(np.abs(got - P64).max()))
    assert np.abs(got - P64).max() <= 1e-5
    assert np.abs(got.sum(1) - 1.0).max() <= 1e-6
    assert torch.equal(M.softmax_predict(gpu(X), C, gpu(Xd)), P)      # the same bits
    assert torch.equal(M.softmax_predict(X, tgt, Xd), P)              # host arrays too
    margin = np.sort(P64, 1)
    assert (margin[:, -1] - margin[:, -2] > 1e-4).all()       # no test row is too close to call
    acc64 = float((P64.argmax(1) == y).mean())
    acc = M.softmax_accuracy(gpu(X), tgt, Xd, y)
    assert 0.0 < acc64 < 1.0 and abs(acc - acc64) <= 1e-5 * acc64
    ll64 = float(np.log(P64[np.arange(N), y]).mean())
    ll = M.softmax_loglik(gpu(X), tgt, Xd, y)
    assert abs(ll - ll64) <= 1e-5 * abs(ll64)
    with pytest.raises(ValueError):
        M.softmax_predict(gpu(X), tgt, Xd[:, :-1])
    # a handful of particles, and more than one slice of them
    for nn in (1, 256 * 64 + 300):
        Xs = np.resize(X, (nn, X.shape[1]))
        Ps = M.softmax_predict(gpu(Xs), tgt, Xd[:7]).cpu().numpy()
        assert np.abs(Ps - R.predict64(Xs, Xd[:7], C)).max() <= 1e-5


# ------------------------------------------------------------- samplers --
def _values(df, shape):
    return np.stack(df["value"].to_list()).reshape(shape)


def _sampler_problem(N=60, C=3, p=2, seed=41):
    _, Xd, y = R.problem(1, N, C, p, seed)
    return Xd, y, C, R.dim(C, p)


def _traj_err(got, ref):
    e = float(np.abs(np.asarray(got, np.float64) - ref).max())
    record_parity(e)
    return e


def test_sampler_jacobi_matches_fp64_graphs_on_and_off():
    n, T, eps = 130, 3, 0.01
    Xd, y, C, d = _sampler_problem()
    m = dsvgd()
    out = {}
    for graphs in (True, False):
        torch.manual_seed(5)
        s = m.Sampler(d, _target(Xd, y, C), m.RBF(float(d)))
        df = s.sample(n, T, eps, order="jacobi", device=DEV, verbose=False, graphs=graphs)
        out[graphs] = _values(df, (T + 1, n, d))
    assert out[True].tobytes() == out[False].tobytes()
    ref = O.sampler_jacobi(out[True][0], lambda X: R.score64(X, Xd, y, C)[0], float(d), T, eps)
    assert _traj_err(out[True], ref) < TRAJ_TOL
    assert np.abs(ref[-1] - ref[0]).max() > 100 * TRAJ_TOL


def test_sampler_sequential_matches_fp64():
    n, T, eps = 33, 2, 0.01
    Xd, y, C, d = _sampler_problem()
    m = dsvgd()
    torch.manual_seed(6)
    s = m.Sampler(d, _target(Xd, y, C), m.RBF(float(d)))
    df = s.sample(n, T, eps, order="sequential", device=DEV, verbose=False)
    vals = _values(df, (T + 1, n, d))
    ref = O.sampler_sequential(vals[0], lambda X: R.score64(X, Xd, y, C)[0], float(d), T, eps)
    assert _traj_err(vals, ref) < TRAJ_TOL
    assert np.abs(ref[-1] - ref[0]).max() > 100 * TRAJ_TOL


def test_sampler_with_minibatches_matches_fp64():
    n, T, eps, B = 130, 4, 0.01, 25
    Xd, y, C, d = _sampler_problem()
    N = len(y)
    m = dsvgd()
    out = {}
    for graphs in (True, False):
        torch.manual_seed(7)
        s = m.Sampler(d, _target(Xd, y, C, batch=B), m.RBF(float(d)))
        df = s.sample(n, T, eps, order="jacobi", device=DEV, verbose=False, graphs=graphs)
        out[graphs] = _values(df, (T + 1, n, d))
    assert out[True].tobytes() == out[False].tobytes()
    X = out[True][0].astype(np.float64)
    ref = [X]
    for t in range(T):           # window t starts at (t B) mod N: the third one wraps
        S = R.score64(X, Xd, y, C, origin=(t * B) % N, B=B)[0]
        X = X + eps * O.phi(X, S, float(d))
        ref.append(X)
    assert _traj_err(out[True], np.stack(ref)) < TRAJ_TOL


def test_sampler_imq_with_ksd_records_stays_finite():
    n, T = 130, 3
    Xd, y, C, d = _sampler_problem()
    m = dsvgd()
    torch.manual_seed(8)
    s = m.Sampler(d, _target(Xd, y, C), m.IMQ("median", -0.5))
    df = s.sample(n, T, 0.01, order="jacobi", device=DEV, verbose=False, ksd_every=1)
    assert list(s.diagnostics.timestep) == [0, 1, 2, 3]
    assert np.isfinite(s.diagnostics.ksd.to_numpy()).all() and (s.diagnostics.ksd > 0).all()
    assert np.isfinite(_values(df, (T + 1, n, d))).all()


def test_distsampler_one_jacobi_step_matches_fp64_and_ksd_runs():
    n, eps = 130, 0.01
    Xd, y, C, d = _sampler_problem()
    X = np.random.RandomState(12).randn(n, d).astype(np.float32)
    m = dsvgd()
    tgt = _target(Xd, y, C)
    ds = m.DistSampler(0, 1, tgt, m.RBF(float(d)), gpu(X).clone(), 1, 1, False, False, False,
                       order="jacobi")
    ds.make_step(eps)
    torch.cuda.synchronize()
    ref = O.sampler_jacobi(X, lambda Z: R.score64(Z, Xd, y, C)[0], float(d), 1, eps)
    assert _traj_err(ds.particles.cpu().numpy(), ref[1]) < TRAJ_TOL
    assert np.abs(ref[1] - ref[0]).max() > 100 * TRAJ_TOL
    k = m.metrics.ksd(gpu(X), tgt, m.RBF("median"))
    assert np.isfinite(k) and k > 0


def test_experiment_runs_end_to_end():
    """--classes 3 --p 5 --nparticles 24 --niter 30 --stepsize 0.05 --rows 300
    --seed 1.  An fp64 CPU run of the same seed (the sampler's own start, the
    oracle's Jacobi steps with the median bandwidth, the fp64 score) gives a
    test accuracy of 0.4 at the start, 1.0 after 15 and after the 30 iterations
    (EXPERIMENT_ACC64; log-likelihood -1.096 -> -0.037); the margin over 1/C is
    half of that run's excess over 1/C, so the bar is 2/3."""
    from click.testing import CliRunner
    E = experiment()
    args = ['--classes', '3', '--p', '5', '--nparticles', '24', '--niter', '30', '--stepsize',
            '0.05', '--rows', '300', '--seed', '1', '--every', '15']
    res = CliRunner().invoke(E.cli, args + ['--order', 'jacobi', '--kernel', 'rbf'])
    assert res.exit_code == 0, res.output
    lines = res.output.strip().splitlines()
    assert [ln.split()[1] for ln in lines[:3]] == ["0", "15", "30"]
    assert lines[-1].startswith("final ksd") and np.isfinite(float(lines[-1].split()[-1]))
    acc = float(lines[2].split()[4])
    assert np.isfinite(float(lines[2].split()[-1]))
    assert acc > 1.0 / 3 + 0.5 * (EXPERIMENT_ACC64 - 1.0 / 3)
    curve, ksd = E.run(16, 2, 0.01, 1, classes=3, p=4, rows=100, order="sequential", kernel="imq",
                       batch=20, out=lambda s: None)
    assert [r["iteration"] for r in curve] == [0, 1, 2]
    assert all(0 <= r["accuracy"] <= 1 and np.isfinite(r["loglik"]) for r in curve)
    assert np.isfinite(ksd) and ksd >= 0


