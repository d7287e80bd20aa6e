"""GPU tests of projected SVGD through every layer: the three dense kernels of
csrc/project.hip against fp64 on the same fp32 inputs, the engine-level object
(full rank = the plain PhiEngine direction), dsvgd.Projection (the learned
subspace against fp64 by the Davis-Kahan bound), Sampler.sample(project=...)
(the complement stays, trajectories against tests/projection_reference.py with
graphs on and off, a minibatch target under graph replay) and experiments/bnn.py.

Tolerances (the project's own): the kernels' entries within SCORE_TOL = 1e-5 of
their absolute-term scale A (the sum of the absolute values of the terms of an
entry); phi within 1e-5 of max |phi|; trajectories 1e-4 absolute, each moved by
more than 100 times that."""
import functools
import math

import numpy as np
import pytest
import torch

import gmix_reference as GM
import logreg_batch_reference as L
import projection_reference as P
from conftest import record_parity
from ksd_reference import KSD_TOL, ksd_reference, median_h64
from oracle import svgd_oracle as O

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-5
PHI_TOL = 1e-5
TRAJ_TOL = 1e-4
DEV = "cuda:0"
F32 = np.float32


def dsvgd():
    import dsvgd as m
    return m


def native():
    from dsvgd import _native as N
    return N


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def strided(a, extra=5, fill=7.5):
    """The array as a view of a wider device buffer (row stride cols + extra)."""
    a = np.asarray(a, F32)
    buf = torch.full((a.shape[0], a.shape[1] + extra), fill, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = gpu(a)
    return buf[:, :a.shape[1]], buf


@functools.lru_cache(maxsize=None)
def _inputs(n, d, seed=0):
    """Particles and scores in fp32 (made once per shape, left unchanged): the
    scores of a Gaussian with a shifted mean, so that S + X does not cancel."""
    rs = np.random.RandomState(1000 * seed + 7 * n + d)
    X = rs.randn(n, d).astype(F32)
    mu = (2.0 * rs.randn(d)).astype(F32)
    lam = rs.uniform(0.5, 2.0, d).astype(F32)
    S = O.score_gaussian(X, mu, lam).astype(F32)
    for a in (X, S, mu, lam):
        a.setflags(write=False)
    return X, S, mu, lam


@functools.lru_cache(maxsize=None)
def _basis(d, r, seed=0):
    """Orthonormal (d, r) in fp32: the QR of a seeded Gaussian."""
    Q = np.linalg.qr(np.random.RandomState(77 + 13 * seed + 1000 * d + r).randn(d, r))[0]
    Q = Q.astype(F32)
    Q.setflags(write=False)
    return Q


def first_split(d):
    """The smallest n whose Gram is split into two slices."""
    lib = native().load()
    n = next(n for n in range(1, 1 << 14) if lib.dsvgd_proj_gram_slices(n, d) == 2)
    assert lib.dsvgd_proj_gram_slices(n - 1, d) == 1
    return n


# ----------------------------------------------------------------- Gram --
def run_gram(Xv, Sv, add_x, ldh_extra=3):
    N = native()
    n, d = Sv.shape
    ws = torch.empty(N.load().dsvgd_proj_gram_workspace_bytes(n, d) // 4, device=DEV)
    Hbuf = torch.full((d, d + ldh_extra), -3.25, dtype=torch.float32, device=DEV)
    H = Hbuf[:, :d]
    N.call("dsvgd_proj_gram", N.ptr(Xv), N.ld(Xv) if Xv is not None else d, N.ptr(Sv), N.ld(Sv), n,
           d, int(add_x), N.ptr(ws), N.ptr(H), N.ld(H), N.stream(DEV))
    torch.cuda.synchronize()
    assert bool((Hbuf[:, d:] == -3.25).all())            # nothing past the d columns
    return H.cpu().numpy()


GRAM_SHAPES = [(1, 1), (33, 31), (385, 40), (64, 1024), ("split", 33)]


@pytest.mark.parametrize("add_x", [True, False])
@pytest.mark.parametrize("n,d", GRAM_SHAPES)
def test_gram_matches_fp64(n, d, add_x):
    if n == "split":
        n = first_split(d)
        assert native().load().dsvgd_proj_gram_slices(n, d) == 2
    X, S, _, _ = _inputs(n, d)
    Xv, _ = strided(X)
    Sv, _ = strided(S, extra=2)
    H = run_gram(Xv if add_x else None, Sv, add_x)
    H64, A = P.gram64(X, S, add_x)
    ratio = float((np.abs(H - H64) / np.maximum(A, 1e-300)).max())
    print("n %d d %d add_x %d: worst |H - H64| / A = %.3g" % (n, d, add_x, ratio))
    record_parity(ratio)
    assert np.isfinite(H).all()
    assert (np.abs(H - H64) <= SCORE_TOL * A).all(), ratio        # every entry
    assert H.tobytes() == H.T.copy().tobytes()                     # exactly symmetric
    H2 = run_gram(Xv if add_x else None, Sv, add_x)
    assert H.tobytes() == H2.tobytes()                             # the same bits


def test_gram_contiguous_equals_strided():
    n, d = 385, 40
    X, S, _, _ = _inputs(n, d)
    a = run_gram(gpu(X), gpu(S), True, ldh_extra=0)
    b = run_gram(strided(X)[0], strided(S)[0], True)
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------- apply and lift --
PROJ_SHAPES = [(33, 33, 1), (130, 40, 33), (64, 1024, 256), (257, 7, 7)]


def _ratio(got, ref, A):
    assert np.isfinite(got).all()
    ratio = float((np.abs(got - ref) / np.maximum(A, 1e-300)).max())
    record_parity(ratio)
    assert (np.abs(got - ref) <= SCORE_TOL * A).all(), ratio
    return ratio


@pytest.mark.parametrize("n,d,r", PROJ_SHAPES)
def test_apply_matches_fp64(n, d, r):
    N = native()
    X, S, _, _ = _inputs(n, d)
    Psi = _basis(d, r)
    Xv, _ = strided(X)
    Sv, _ = strided(S, extra=1)
    Pv, _ = strided(Psi, extra=3)
    Xr, Xrb = strided(np.zeros((n, r)), extra=2, fill=-1.5)
    Sr, Srb = strided(np.zeros((n, r)), extra=4, fill=-2.5)
    N.call("dsvgd_proj_apply", N.ptr(Xv), N.ld(Xv), N.ptr(Sv), N.ld(Sv), n, d, N.ptr(Pv), N.ld(Pv),
           r, N.ptr(Xr), N.ld(Xr), N.ptr(Sr), N.ld(Sr), N.stream(DEV))
    torch.cuda.synchronize()
    assert bool((Xrb[:, r:] == -1.5).all()) and bool((Srb[:, r:] == -2.5).all())
    P64 = Psi.astype(np.float64)
    for got, src in ((Xr, X), (Sr, S)):
        a = src.astype(np.float64)
        rr = _ratio(got.cpu().numpy(), a @ P64, np.abs(a) @ np.abs(P64))
        print("apply n %d d %d r %d: worst err / A = %.3g" % (n, d, r, rr))
    # contiguous arrays: the same bits
    Xr2, Sr2 = torch.empty(n, r, device=DEV), torch.empty(n, r, device=DEV)
    Xc, Sc, Pc = gpu(X), gpu(S), gpu(Psi)
    N.call("dsvgd_proj_apply", N.ptr(Xc), d, N.ptr(Sc), d, n, d, N.ptr(Pc), r, r, N.ptr(Xr2), r,
           N.ptr(Sr2), r, N.stream(DEV))
    assert torch.equal(Xr2, Xr) and torch.equal(Sr2, Sr)


@pytest.mark.parametrize("n,d,r", PROJ_SHAPES)
def test_lift_matches_fp64_and_moves_x_by_the_step(n, d, r):
    N = native()
    X, _, _, _ = _inputs(n, d)
    Psi = _basis(d, r)
    phir = (0.3 * np.random.RandomState(5 + n + r).randn(n, r)).astype(F32)
    Fv, _ = strided(phir, extra=3)
    Pv, _ = strided(Psi, extra=1)
    Xv, Xb = strided(X, extra=2, fill=-4.5)
    out, outb = strided(np.zeros((n, d)), extra=6, fill=-5.5)

    def lift(step, xv, ov):
        N.call("dsvgd_proj_lift", N.ptr(Fv), N.ld(Fv), N.ptr(Pv), N.ld(Pv), n, d, r, float(step),
               N.ptr(xv), N.ld(xv) if xv is not None else d, N.ptr(ov),
               N.ld(ov) if ov is not None else d, N.stream(DEV))
        torch.cuda.synchronize()
    # step 0 with Phi_out: X keeps its bits (and may be absent)
    before = Xb.clone()
    lift(0.0, Xv, out)
    assert torch.equal(Xb, before)
    phi = out.cpu().numpy()
    lift(0.0, None, out)
    assert out.cpu().numpy().tobytes() == phi.tobytes()
    assert bool((outb[:, d:] == -5.5).all())
    f64, p64 = phir.astype(np.float64), Psi.astype(np.float64)
    rr = _ratio(phi, f64 @ p64.T, np.abs(f64) @ np.abs(p64).T)
    print("lift n %d d %d r %d: worst err / A = %.3g" % (n, d, r, rr))
    # a step: X + eps Phi_out, rounded once (one ulp of the two terms)
    eps = 0.37
    out2, _ = strided(np.zeros((n, d)), extra=6)
    lift(eps, Xv, out2)
    assert out2.cpu().numpy().tobytes() == phi.tobytes()
    assert bool((Xb[:, d:] == -4.5).all())
    want = X.astype(np.float64) + np.float64(F32(eps)) * phi.astype(np.float64)
    ulp = 2.0 ** -23 * (np.abs(X) + abs(eps) * np.abs(phi))
    assert (np.abs(Xv.cpu().numpy() - want) <= ulp).all()
    assert np.abs(want - X).max() > 1e-2
    # without Phi_out: the same X
    Xv2, _ = strided(X)
    lift(eps, Xv2, None)
    assert torch.equal(Xv2, Xv)


# ------------------------------------------------- full-rank equivalence --
@pytest.mark.parametrize("kind", ["rbf_fixed", "imq_median"])
def test_full_rank_direction_is_the_plain_direction(kind):
    from dsvgd.projection import ProjectedEngine
    m = dsvgd()
    n, d = 256, 40
    X, S, _, _ = _inputs(n, d)
    kern, h = (m.RBF(1.0), 1.3 * d) if kind == "rbf_fixed" else (m.IMQ("median", -0.5), None)
    Xg, Sg = gpu(X), gpu(S)
    plain = m.PhiEngine(n, d, device=DEV, kernel=kern)
    plain.step(Xg, Sg, h=h)
    ref = plain.phi.cpu().numpy().astype(np.float64)
    peng = ProjectedEngine(n, d, d, device=DEV, kernel=kern)
    peng.set_basis(_basis(d, d))
    phi = peng.direction(Xg, Sg, h=h).cpu().numpy()
    assert torch.equal(Xg, gpu(X))                       # nothing moved
    e = float(np.abs(phi - ref).max() / np.abs(ref).max())
    record_parity(e)
    print("%s: |phi_projected - phi| / max |phi| = %.3g" % (kind, e))
    assert e <= PHI_TOL
    # and both are the fp64 direction
    beta = None if kind == "rbf_fixed" else -0.5
    hh = h if h is not None else median_h64(X)
    ref64 = P.phi64(X, S, hh, beta)
    assert np.abs(phi - ref64).max() <= 2 * PHI_TOL * np.abs(ref64).max()
    if h is None:     # the rotation keeps the median bandwidth
        assert abs(peng.engine.state.read()[1] - plain.state.read()[1]) <= 1e-5 * hh


# ------------------------------------------------------------- Sampler --
def _values(df, shape):
    return np.stack(df["value"].to_list()).reshape(shape)


def test_sampler_leaves_the_complement_where_it_was_drawn():
    m = dsvgd()
    n, d, r, T = 128, 40, 4, 5
    _, _, mu, lam = _inputs(n, d)
    Psi = _basis(d, r)
    proj = m.Projection(basis=Psi)
    torch.manual_seed(3)
    s = m.Sampler(d, m.targets.Gaussian(mu, lam), m.RBF("median"))
    df = s.sample(n, T, 0.3, order="jacobi", device=DEV, verbose=False, project=proj)
    vals = _values(df, (T + 1, n, d)).astype(np.float64)
    move = vals[-1] - vals[0]
    p64 = Psi.astype(np.float64)
    out = move - move @ p64 @ p64.T
    bound = 1e-5 * np.abs(move).max()
    print("moved %.3g, outside the subspace %.3g (bound %.3g)"
          % (np.abs(move).max(), np.abs(out).max(), bound))
    record_parity(np.abs(out).max() / np.abs(move).max())
    assert np.abs(out).max() <= bound
    assert np.abs(move).max() > 100 * bound and np.abs(move).max() > 0.1
    assert proj.refreshes == 0 and proj.eigenvalues is None and proj.captured is None
    assert proj.basis.shape == (d, r) and proj.basis.is_cuda
    assert torch.equal(proj.basis.cpu(), torch.from_numpy(Psi))


# ---------------------------------------------------- learned subspace --
@functools.lru_cache(maxsize=None)
def lowrank_logreg():
    """A logistic-regression posterior whose data have rank 3 (+ 0.01 noise):
    n = 384 particles from N(0, I), p = 39 features (d = 40), N = 200 rows."""
    rng = np.random.default_rng(7)
    n, p, N, r = 384, 39, 200, 3
    B = rng.standard_normal((p, r)) / np.sqrt(p) * 3
    Z = rng.standard_normal((N, r))
    Xd = Z @ B.T + 0.01 * rng.standard_normal((N, p))
    wt = rng.standard_normal(p)
    t = np.sign(Xd @ wt + 0.3 * rng.logistic(size=N))
    X = rng.standard_normal((n, p + 1))
    return X.astype(F32), Xd.astype(F32), t.astype(F32)


def test_learned_subspace_matches_fp64_by_davis_kahan():
    m = dsvgd()
    X, xd, t = lowrank_logreg()
    n, d = X.shape
    r = 4
    target = m.targets.LogisticRegression(xd, t)
    Xg = gpu(X)
    Sg = torch.empty_like(Xg)
    target.score(Xg, Sg)
    S = Sg.cpu().numpy()
    ref_s = O.score_logreg(X, xd, t)
    assert np.abs(S - ref_s).max() <= 1e-4 * np.abs(ref_s).max()
    proj = m.Projection(rank=r)
    eng = proj.begin(n, d, m.RBF("median"), DEV)
    proj.refresh(eng, Xg, Sg)
    H = eng.H.cpu().numpy().astype(np.float64)
    H64, A = P.gram64(X, S, True)
    assert (np.abs(H - H64) <= SCORE_TOL * A).all()
    Psi64, lam64 = P.basis64(H64, r)
    gap = lam64[r - 1] - lam64[r]
    print("fp64 eigenvalues", lam64[:6], "relative gap %.3f" % (gap / lam64[r - 1]))
    assert gap / lam64[r - 1] >= 0.5
    Psi = proj.basis.cpu().numpy().astype(np.float64)
    assert Psi.shape == (d, r) and proj.basis is eng.Psi
    assert np.abs(Psi.T @ Psi - np.eye(r)).max() <= 1e-6
    top = np.abs(Psi).argmax(0)
    assert (Psi[top, np.arange(r)] > 0).all()                   # the sign rule
    Pp, Pp64 = Psi @ Psi.T, Psi64 @ Psi64.T
    dk = 2.0 * math.sqrt(2.0) * np.linalg.norm(H - H64) / gap
    err = np.linalg.norm(Pp - Pp64)
    print("|P - P64|_F = %.3g, Davis-Kahan bound %.3g" % (err, dk))
    record_parity(err / dk)
    assert err <= dk
    lam = proj.eigenvalues
    lam = lam.numpy() if torch.is_tensor(lam) else np.asarray(lam)
    assert lam.shape == (d,) and lam.dtype == np.float64 and (np.diff(lam) <= 0).all()
    assert np.abs(lam - lam64).max() <= 1e-5 * lam64[0]
    assert abs(proj.captured - lam[:r].sum() / lam.sum()) <= 1e-12
    assert 0.99 < proj.captured <= 1.0
    assert proj.refreshes == 1 and proj.captured_history == [(0, proj.captured)]


# --------------------------------------------------------- trajectories --
N_T, D_T, R_T, T_T = 200, 12, 3, 6


def _traj_target(kind):
    m = dsvgd()
    if kind == "gmix":
        _, means, lam, w = GM.problem(N_T, 3, D_T, 1.5, seed=5)
        return (m.targets.GaussianMixture(means, lam, w), m.IMQ(2.0, -0.5), 2.0, -0.5,
                lambda X, l: GM.evaluate64(X, means, lam, w)["S"], 0.3)
    _, _, mu, lam = _inputs(N_T, D_T)
    score = lambda X, l: O.score_gaussian(X, mu, lam)                     # noqa: E731
    if kind == "gauss_median":
        return m.targets.Gaussian(mu, lam), m.RBF("median"), None, None, score, 0.2
    return m.targets.Gaussian(mu, lam), m.RBF(2.5), 2.5, None, score, 0.2


def _run(target, kern, eps, make_proj, seed=4, T=T_T):
    """The run with graphs on and off (the same bits), and the last Projection."""
    m = dsvgd()
    out = {}
    for graphs in (True, False):
        proj = make_proj()
        proj.record_bases = True
        torch.manual_seed(seed)
        s = m.Sampler(D_T, target, kern)
        df = s.sample(N_T, T, eps, order="jacobi", device=DEV, verbose=False, graphs=graphs,
                      project=proj)
        out[graphs] = _values(df, (T + 1, N_T, D_T))
    assert out[True].tobytes() == out[False].tobytes()
    return out[True], proj


def _check_traj(vals, ref):
    e = float(np.abs(vals.astype(np.float64) - ref).max())
    move = float(np.abs(ref[-1] - ref[0]).max())
    print("trajectory error %.3g, moved %.3g" % (e, move))
    record_parity(e)
    assert e < TRAJ_TOL
    assert move > 100 * TRAJ_TOL


def _recorded(proj):
    """basis(l, X, S) of jacobi64 from the bases the run recorded."""
    def basis(l, X, S):
        past = [b for it, b in proj.bases if it <= l]
        return past[-1].astype(np.float64)
    return basis


@pytest.mark.parametrize("kind", ["gauss_fixed", "gauss_median", "gmix"])
def test_sampler_fixed_basis_matches_fp64_graphs_on_and_off(kind):
    target, kern, h, beta, score, eps = _traj_target(kind)
    Psi = _basis(D_T, R_T)
    vals, proj = _run(target, kern, eps, lambda: dsvgd().Projection(basis=Psi))
    assert proj.refreshes == 0 and proj.bases == []
    ref = P.jacobi64(vals[0], score, Psi.astype(np.float64), T_T, eps, h, beta)
    _check_traj(vals, ref)


@pytest.mark.parametrize("kind", ["gauss_fixed", "gauss_median", "gmix"])
def test_sampler_learned_basis_matches_fp64_graphs_on_and_off(kind):
    """rank=3, every=2: the fp64 run takes each refresh's basis from the run,
    so the parity does not hinge on eigenvector perturbation; a replay that
    kept the first basis ends somewhere else."""
    target, kern, h, beta, score, eps = _traj_target(kind)
    vals, proj = _run(target, kern, eps, lambda: dsvgd().Projection(rank=R_T, every=2))
    assert proj.refreshes == 3 and [it for it, _ in proj.bases] == [0, 2, 4]
    assert [it for it, _ in proj.captured_history] == [0, 2, 4]
    ref = P.jacobi64(vals[0], score, _recorded(proj), T_T, eps, h, beta)
    _check_traj(vals, ref)
    assert torch.equal(proj.basis.cpu(), torch.from_numpy(proj.bases[-1][1]))
    # the basis moved between refreshes: replay read the new one
    assert np.abs(proj.bases[0][1] - proj.bases[-1][1]).max() > 1e-3
    stale = P.jacobi64(vals[0], score, proj.bases[0][1].astype(np.float64), T_T, eps, h, beta)
    assert np.abs(stale[-1] - ref[-1]).max() > 10 * TRAJ_TOL


def test_sampler_minibatch_window_advances_under_replay():
    m = dsvgd()
    p, N, B, eps, seed = D_T - 1, 90, 40, 2e-2, 84
    assert T_T * B > N                                         # the windows wrap the data
    xd, t = L.sorted_problem(N, p, seed)
    target = m.targets.LogisticRegression(xd, t, batch=B)
    kern = m.RBF(float(D_T))
    vals, proj = _run(target, kern, eps, lambda: dsvgd().Projection(rank=R_T, every=2), seed=seed)
    assert proj.refreshes == 3
    basis = _recorded(proj)
    ref = P.jacobi64(vals[0], L.window_score_fn(xd, t, B), basis, T_T, eps, float(D_T))
    _check_traj(vals, ref)
    # a window that stands still, or all of the data, is another trajectory
    still = P.jacobi64(vals[0], lambda X, l: L.window_score_fn(xd, t, B)(X, 0), basis, T_T, eps,
                       float(D_T))
    full = P.jacobi64(vals[0], lambda X, l: O.score_logreg(X, xd, t), basis, T_T, eps, float(D_T))
    apart = min(np.abs(still[-1] - ref[-1]).max(), np.abs(full[-1] - ref[-1]).max())
    print("still / full-data trajectories at least %.3g away" % apart)
    assert apart > 100 * TRAJ_TOL


def test_sampler_ksd_every_measures_in_the_full_space_and_moves_nothing():
    m = dsvgd()
    target, kern, h, beta, score, eps = _traj_target("gauss_median")
    Psi = _basis(D_T, R_T)
    out = []
    for every in (None, 3):
        torch.manual_seed(4)
        s = m.Sampler(D_T, target, kern)
        df = s.sample(N_T, T_T, eps, order="jacobi", device=DEV, verbose=False, ksd_every=every,
                      project=m.Projection(basis=Psi))
        out.append(_values(df, (T_T + 1, N_T, D_T)))
    assert out[0].tobytes() == out[1].tobytes()
    diag = s.diagnostics
    assert list(diag.timestep) == [0, 3, 6]
    worst = 0.0
    for _, row in diag.iterrows():
        X = out[1][int(row.timestep)]
        Xg = gpu(X)
        Sg = torch.empty_like(Xg)
        target.score(Xg, Sg)
        ref = ksd_reference(X, Sg.cpu().numpy(), float(row.h))
        ev = abs(row.ksd2_v - ref["V"]) / ref["A_v"]
        assert ev <= KSD_TOL
        assert abs(row.h - median_h64(X)) <= 1e-5 * row.h     # the d-dimensional median
        worst = max(worst, ev)
    record_parity(worst)


# ----------------------------------------------------------- experiment --
def test_experiment_runs_with_project():
    from test_bnn_host import experiment
    lines = []
    curve, ksd = experiment().run(32, 4, 1e-4, 2, hidden=10, rows=200, p=4, device=DEV,
                                  out=lines.append, project=8, project_every=2)
    assert [r["iteration"] for r in curve] == [0, 2, 4]
    assert all(np.isfinite(r["rmse"]) and np.isfinite(r["loglik"]) for r in curve)
    assert np.isfinite(ksd) and ksd >= 0
    cap = [ln for ln in lines if "captured" in ln]
    assert len(cap) == 2 and len(lines) == 6 and lines[-1].startswith("final ksd")
    for ln in cap:
        v = float(ln.split()[-1])
        assert 0.0 < v <= 1.0
