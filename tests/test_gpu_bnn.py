"""GPU tests of the Bayesian neural-network regression target: the score
kernel against the fp64 closed form of tests/bnn_reference.py at its edges
(one row, a ragged last chunk, p no multiple of 4, H no power of two, the
limits p = H = 64), dead units, strided views and the scale, the predictions
and their metrics, and the target through Sampler (both orders, graphs on and
off) and DistSampler.

The score bound, per entry: |S - S64| <= 1e-5 A + the ambiguity slack.  A is
the sum of the absolute values of the entry's terms (1e-5: the project's score
and KSD bound against such scales).  The slack covers the pre-activations a
with |a| <= 1e-5 (|b1| + sum_k |W1_kh| |z_qk|), which fp32 may round to the
other side of 0: the term of such a (q, h) in dW1[:, h] and db1[h] is then
present or absent as a whole.  How many there may be is a condition on the
inputs, asserted here: at most max(1, 2.5e-4 n N H).  Trajectories: 1e-4
absolute, as tests/test_gpu_imq.py."""
import functools

import numpy as np
import pytest
import torch

import bnn_reference as R
from conftest import record_parity
from oracle import svgd_oracle as O

pytestmark = pytest.mark.gpu
TRAJ_TOL = 1e-4
PRED_TOL = 1e-5
AMBIGUOUS_CAP = 2.5e-4
DEV = "cuda:0"

SCORE_SHAPES = [(1, 1, 1, 1, 2), (33, 37, 5, 7, 3), (130, 257, 13, 50, 4), (64, 1000, 8, 50, 5),
                (5, 70, 64, 64, 6)]


def dsvgd():
    import dsvgd as m
    return m


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def _case(n, N, p, H, seed):
    """The seeded problem and its fp64 score, scale and bound (computed once
    per shape, shared and left unchanged)."""
    X, Z, y = R.problem(n, N, p, H, seed)
    S, A, bound, count = R.score_bound(X, Z, y, p, H)
    for a in (X, Z, y, S, A, bound):
        a.setflags(write=False)
    return X, Z, y, S, A, bound, count


def _target(Z, y, H, **kw):
    return dsvgd().targets.BayesianNN(torch.from_numpy(Z), torch.from_numpy(y), hidden=H, **kw)


def _check_score(got, S, A, bound, scale=1.0):
    err = np.abs(np.asarray(got, np.float64) - scale * S)
    worst = float((err / (abs(scale) * A)).max())
    print("worst err/A %.3g (entries over 1e-5 A, within the slack: %d)"
          % (worst, int((err > abs(scale) * R.SCORE_TOL * A).sum())))
    record_parity(worst)
    assert np.all(err <= abs(scale) * bound)
    return worst


# ---------------------------------------------------------------- score --
@pytest.mark.parametrize("n,N,p,H,seed", SCORE_SHAPES)
def test_score_matches_fp64(n, N, p, H, seed):
    X, Z, y, S, A, bound, count = _case(n, N, p, H, seed)
    print("ambiguous triples: %d of %d" % (count, n * N * H))
    assert count <= max(1, AMBIGUOUS_CAP * n * N * H)
    tgt = _target(Z, y, H)
    Xg = gpu(X)
    out = torch.full_like(Xg, float("nan"))
    tgt.score(Xg, out)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    _check_score(got, S, A, bound)


def test_other_hyper_prior_parameters():
    n, N, p, H = 33, 37, 5, 7
    X, Z, y = _case(n, N, p, H, 3)[:3]
    S, A, bound, _ = R.score_bound(X, Z, y, p, H, 2.0, 0.5)
    out = torch.empty(n, R.dim(p, H), device=DEV)
    _target(Z, y, H, a0=2.0, b0=0.5).score(gpu(X), out)
    _check_score(out.cpu().numpy(), S, A, bound)


def test_dead_units_leave_the_prior():
    """b1 = -10 and |W1| <= 1e-3: no unit is ever active, so the entries of
    W1, b1 and w2 are -lambda theta and d b2 = gamma sum r - lambda b2."""
    n, N, p, H = 9, 300, 6, 10
    X, Z, y = R.problem(n, N, p, H, seed=8)
    X = X.copy()
    X[:, :p * H] = np.clip(X[:, :p * H], -1e-3, 1e-3)
    X[:, p * H:p * H + H] = -10.0
    assert (np.abs(Z).sum(1).max() * 1e-3) < 10.0
    out = torch.empty(n, R.dim(p, H), device=DEV)
    _target(Z, y, H).score(gpu(X), out)
    got = out.cpu().numpy().astype(np.float64)
    X64 = X.astype(np.float64)
    lam, gam = np.exp(X64[:, -1]), np.exp(X64[:, -2])
    want = -lam[:, None] * X64[:, :p * H + 2 * H]
    assert np.all(np.abs(got[:, :p * H + 2 * H] - want) <= 1e-6 * np.abs(want))
    r = y.astype(np.float64)[None, :] - X64[:, p * H + 2 * H][:, None]
    db2 = gam * r.sum(1) - lam * X64[:, p * H + 2 * H]
    scale = gam * np.abs(r).sum(1) + lam * np.abs(X64[:, p * H + 2 * H])
    assert np.all(np.abs(got[:, p * H + 2 * H] - db2) <= R.SCORE_TOL * scale)


def test_views_scale_and_row_calls():
    n, N, p, H, seed = 33, 37, 5, 7, 3
    X, Z, y, S, A, bound, _ = _case(n, N, p, H, seed)
    d = R.dim(p, H)
    tgt = _target(Z, y, H)
    wide_x = torch.full((n, d + 9), float("nan"), device=DEV)
    wide_o = torch.full((n, d + 5), float("nan"), device=DEV)
    Xv, Ov = wide_x[:, 4:4 + d], wide_o[:, 2:2 + d]
    Xv.copy_(gpu(X))
    tgt.score(Xv, Ov, scale=2.5)
    first = wide_o.cpu().numpy().copy()
    _check_score(first[:, 2:2 + d], S, A, bound, scale=2.5)
    assert np.isnan(first[:, :2]).all() and np.isnan(first[:, 2 + d:]).all()
    assert np.isnan(wide_x[:, :4].cpu().numpy()).all()
    assert np.isnan(wide_x[:, 4 + d:].cpu().numpy()).all()
    tgt.score(Xv, Ov, scale=2.5)
    assert wide_o.cpu().numpy().tobytes() == first.tobytes()
    # n = 1 through a row view: the same bits as the row of the batched call
    rows = torch.full((n, d + 5), float("nan"), device=DEV)
    for i in (0, 17, n - 1):
        tgt.score(Xv[i:i + 1], rows[i:i + 1, 2:2 + d], scale=2.5)
        assert rows[i].cpu().numpy().tobytes() == first[i].tobytes()


# -------------------------------------------------------------- predict --
@pytest.mark.parametrize("n,N,p,H,seed", [(33, 37, 5, 7, 3), (130, 257, 13, 50, 4)])
def test_predict_and_metrics_match_fp64(n, N, p, H, seed):
    X, Z, y = _case(n, N, p, H, seed)[:3]
    M = dsvgd().metrics
    tgt = _target(Z, y, H)
    F64, Fscale = R.predict64(X, Z, p, H)
    F = M.bnn_predict(gpu(X), tgt, gpu(Z))
    assert F.shape == (n, N) and F.device.type == "cuda"
    err = np.abs(F.cpu().numpy().astype(np.float64) - F64)
    record_parity(float((err / Fscale).max()))
    assert np.all(err <= PRED_TOL * Fscale)
    assert torch.equal(M.bnn_predict(X, H, Z), F)      # host arrays, the width alone
    y64 = y.astype(np.float64)
    rmse = np.sqrt(((F64.mean(0) - y64) ** 2).mean())
    lg = X[:, -2].astype(np.float64)
    comp = 0.5 * (lg[:, None] - np.log(2 * np.pi)) - 0.5 * np.exp(lg)[:, None] * (y64 - F64) ** 2
    mx = comp.max(0)
    ll = (mx + np.log(np.exp(comp - mx).sum(0)) - np.log(n)).mean()
    got_rmse, got_ll = M.bnn_rmse(gpu(X), tgt, Z, y), M.bnn_loglik(gpu(X), tgt, Z, y)
    print("rmse %.9g ref %.9g, loglik %.9g ref %.9g" % (got_rmse, rmse, got_ll, ll))
    assert abs(got_rmse - rmse) <= 1e-5 * abs(rmse)
    assert abs(got_ll - ll) <= 1e-5 * abs(ll)
    with pytest.raises(ValueError):
        M.bnn_predict(gpu(X), H + 1, gpu(Z))


# ------------------------------------------------------------- samplers --
def _values(df, shape):
    return np.stack(df["value"].to_list()).reshape(shape)


def _score_fn(Z, y, p, H):
    return lambda X: R.score64(X, Z, y, p, H)[0]


def _traj_err(got, ref):
    e = float(np.abs(np.asarray(got, np.float64) - ref).max())
    record_parity(e)
    return e


def test_sampler_jacobi_matches_fp64_graphs_on_and_off():
    n, N, p, H, T, eps = 130, 64, 13, 50, 3, 1e-5
    d = R.dim(p, H)
    _, Z, y = R.problem(1, N, p, H, seed=9)
    m = dsvgd()
    out = {}
    for graphs in (True, False):
        torch.manual_seed(5)
        s = m.Sampler(d, _target(Z, y, H), m.RBF(float(d)))
        df = s.sample(n, T, eps, order="jacobi", device=DEV, verbose=False, graphs=graphs)
        out[graphs] = _values(df, (T + 1, n, d))
    assert out[True].tobytes() == out[False].tobytes()
    ref = O.sampler_jacobi(out[True][0], _score_fn(Z, y, p, H), float(d), T, eps)
    assert _traj_err(out[True], ref) < TRAJ_TOL
    assert np.abs(ref[-1] - ref[0]).max() > 100 * TRAJ_TOL


def test_sampler_sequential_matches_fp64():
    n, N, p, H, T, eps = 12, 40, 5, 7, 2, 1e-4
    d = R.dim(p, H)
    _, Z, y = R.problem(1, N, p, H, seed=10)
    m = dsvgd()
    torch.manual_seed(6)
    s = m.Sampler(d, _target(Z, y, H), m.RBF(float(d)))
    df = s.sample(n, T, eps, order="sequential", device=DEV, verbose=False)
    vals = _values(df, (T + 1, n, d))
    ref = O.sampler_sequential(vals[0], _score_fn(Z, y, p, H), float(d), T, eps)
    assert _traj_err(vals, ref) < TRAJ_TOL
    assert np.abs(ref[-1] - ref[0]).max() > 100 * TRAJ_TOL


def test_experiment_runs_end_to_end():
    """experiments/bnn.py at a toy size: the curve has a row per record and
    finite numbers (its values are recorded in DESIGN.md, not asserted)."""
    from test_bnn_host import experiment
    lines = []
    curve, ksd = experiment().run(32, 4, 1e-4, 2, hidden=10, rows=200, p=4, device=DEV,
                                  out=lines.append)
    assert [r["iteration"] for r in curve] == [0, 2, 4]
    assert all(np.isfinite(r["rmse"]) and np.isfinite(r["loglik"]) for r in curve)
    assert np.isfinite(ksd) and ksd >= 0
    assert len(lines) == 4 and lines[-1].startswith("final ksd")


def test_distsampler_one_jacobi_step_matches_fp64():
    n, N, p, H, eps = 130, 64, 13, 50, 1e-4
    d = R.dim(p, H)
    X, Z, y = R.problem(n, N, p, H, seed=11)
    m = dsvgd()
    ds = m.DistSampler(0, 1, _target(Z, y, H), m.RBF(float(d)), gpu(X).clone(), N, N, False, False,
                       False, order="jacobi")
    ds.make_step(eps)
    torch.cuda.synchronize()
    ref = O.sampler_jacobi(X, _score_fn(Z, y, p, H), float(d), 1, eps)
    assert _traj_err(ds.particles.cpu().numpy(), ref[1]) < TRAJ_TOL
    assert np.abs(ref[1] - ref[0]).max() > 100 * TRAJ_TOL
