"""GPU tests of the AdaGrad steps and of the minibatch BayesianNN scores,
against the fp64 references of tests/adagrad_reference.py.

The update kernel alone: eight roundings lie between p and x' (square, scale,
fma, sqrt, add, divide, multiply, add), so every entry is within 8 * 2^-24 of
the fp64 rule, relative to G' and to |x| + step |p| / (eps + sqrt(G')).

Through the samplers the direction carries the project's phi bound, 1e-5 of
max |phi|, and the rule amplifies an error of p by at most 1 / eps (the slope
of p / (eps + |p|) at 0).  The conditioned cases take eps = 0.1 max |phi| of
step 0 and assert from the fp64 reference that step * 1e-5 max |phi_t| / eps
<= 1e-5 at every step, so the project's trajectory bound of 1e-4 applies.  The
default eps = 1e-6 is compared over one step on the entries with |phi| >=
1e-3 max |phi| (at most 1 % are left out, asserted): there the slope is
eps / (eps + |phi| - 1e-5 M)^2 <= 10.3 eps / M^2 per 1e-5 M of phi error.

The minibatch score: the bound form of tests/test_gpu_bnn.py, 1e-5 A + the
ambiguity slack, both with the likelihood part times N / B."""
import functools

import numpy as np
import pytest
import torch

import adagrad_reference as A
import bnn_reference as R
import imq_reference as I
from conftest import record_parity
from oracle import svgd_oracle as O

pytestmark = pytest.mark.gpu
TRAJ_TOL = 1e-4          # as tests/test_gpu_bnn.py
AMBIGUOUS_CAP = 2.5e-4   # as tests/test_gpu_bnn.py
U = 2.0 ** -24
DEV = "cuda:0"
ALPHA = float(np.float32(0.9))


def dsvgd():
    import dsvgd as m
    return m


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _values(df, shape):
    return np.stack(df["value"].to_list()).reshape(shape)


def _err(got, ref):
    e = float(np.abs(np.asarray(got, np.float64) - ref).max())
    record_parity(e)
    return e


def sampler_init(n, d, seed):
    """The particles Sampler.sample draws after torch.manual_seed(seed)."""
    from torch.distributions.normal import Normal
    torch.manual_seed(seed)
    q = Normal(0, 1)
    return torch.cat([q.sample((d, 1)) for _ in range(n)], dim=1).t().contiguous().numpy()


def gaussian(d, seed):
    rs = np.random.RandomState(seed)
    return rs.randn(d).astype(np.float32), rs.uniform(0.5, 2.0, d).astype(np.float32)


# ------------------------------------------------------ the update kernel --
UPDATE_SHAPES = [(1, 1, 1), (5, 3, 7), (33, 70, 70), (64, 256, 256), (130, 257, 257)]


@pytest.mark.parametrize("m,d,ldx", UPDATE_SHAPES)
def test_update_kernel_matches_fp64(m, d, ldx):
    from dsvgd import _native as N
    rs = np.random.RandomState(100 + m)
    X = rs.randn(m, d).astype(np.float32)
    P = (rs.randn(m, d) * np.exp(rs.uniform(-6, 2, (m, d)))).astype(np.float32)
    G = rs.uniform(0.0, 2.0, (m, d)).astype(np.float32)
    G[::2] = -1.0                                   # rows without history
    if m > 1:
        G[1, d // 2:] = -1.0                        # and a row with both kinds
    step, eps = float(np.float32(0.05)), float(np.float32(1e-6))
    X64, G64 = A.update64(X, P, G, step, ALPHA, eps)

    def run():
        Xb = torch.full((m, ldx), float("nan"), device=DEV)
        Xb[:, :d] = gpu(X)
        Pg, Gg = gpu(P), gpu(G)
        N.call("dsvgd_adagrad_step", N.ptr(Xb), ldx, N.ptr(Pg), d, N.ptr(Gg), d, m, d, step,
               ALPHA, eps, N.stream(torch.device(DEV)))
        torch.cuda.synchronize()
        return Xb.cpu().numpy(), Gg.cpu().numpy()
    Xb, Gn = run()
    assert np.isnan(Xb[:, d:]).all()                # the padding columns: untouched
    Xn = Xb[:, :d].astype(np.float64)
    eg = np.abs(Gn.astype(np.float64) - G64)
    ex = np.abs(Xn - X64)
    move = step * np.abs(P.astype(np.float64)) / (eps + np.sqrt(G64))
    bx = 8 * U * (np.abs(X.astype(np.float64)) + move)
    print("worst G err / G' %.3g ulp-halves, worst x err / bound %.3g"
          % (float((eg / np.maximum(G64, 1e-300)).max() / U), float((ex / bx).max())))
    record_parity(float((ex / bx).max()) * 8 * U)
    assert np.all(Gn >= 0.0)
    assert np.all(eg <= 8 * U * G64)
    assert np.all(ex <= bx)
    X2, G2 = run()                                  # the same inputs: the same bits
    assert X2.tobytes() == Xb.tobytes() and G2.tobytes() == Gn.tobytes()


# ------------------------------------------------- Sampler, conditioned --
def conditioned_case(kind, n, d, seed):
    """(target factory, kernel factory, fp64 score_fn(X, t), jacobi64 keywords)."""
    m = dsvgd()
    if kind == "gmm":
        target, score = m.targets.GaussianMixture1D, lambda X, t: O.score_gmm(X)
    else:
        mu, lam = gaussian(d, seed)
        target = lambda: m.targets.Gaussian(mu, lam)          # noqa: E731
        score = lambda X, t: O.score_gaussian(X, mu, lam)     # noqa: E731
    h = float(d)
    if kind == "imq":
        return target, lambda: m.IMQ(h, -0.5), score, dict(
            h=h, phi_fn=lambda X, S, hh: I.phi64(X, S, hh, -0.5))
    if kind == "median":
        return target, lambda: m.RBF("median"), score, dict(h=None, median=True)
    return target, lambda: m.RBF(h), score, dict(h=h)


def conditioned_reference(kind, n, d, seed, T, step):
    target, kernel, score, kw = conditioned_case(kind, n, d, seed)
    X0 = sampler_init(n, d, seed)
    _, dirs = A.jacobi64(X0, score, T=1, step=step, alpha=ALPHA, eps=1.0, **kw)
    eps = float(np.float32(0.1 * np.abs(dirs[0]).max()))
    ref, dirs = A.jacobi64(X0, score, T=T, step=step, alpha=ALPHA, eps=eps, **kw)
    return target, kernel, X0, eps, ref, dirs


CONDITIONED = [("rbf", 130, 5, 21), ("rbf", 64, 3, 22), ("imq", 130, 5, 23), ("imq", 64, 3, 24),
               ("median", 130, 5, 25), ("median", 64, 3, 26), ("gmm", 130, 1, 27),
               ("rbf", 130, 256, 28)]    # (d = 256: the one-operand K . W form)


@pytest.mark.parametrize("kind,n,d,seed", CONDITIONED)
def test_sampler_adagrad_matches_fp64_graphs_on_and_off(kind, n, d, seed):
    T, step = 3, 0.05
    target, kernel, X0, eps, ref, dirs = conditioned_reference(kind, n, d, seed, T, step)
    for p in dirs:    # the phi bound, amplified by at most 1 / eps
        assert step * 1e-5 * np.abs(p).max() / eps <= 1e-5
    m = dsvgd()
    out = {}
    for graphs in (True, False):
        torch.manual_seed(seed)
        s = m.Sampler(d, target(), kernel())
        df = s.sample(n, T, step, order="jacobi", device=DEV, verbose=False, graphs=graphs,
                      adagrad=m.AdaGrad(0.9, eps))
        out[graphs] = _values(df, (T + 1, n, d))
    assert out[True][0].tobytes() == X0.tobytes()
    assert out[True].tobytes() == out[False].tobytes()
    assert _err(out[True], ref) < TRAJ_TOL
    assert np.abs(ref[-1] - ref[0]).max() > 100 * TRAJ_TOL


# ---------------------------------------------- Sampler, default eps --
DEFAULT_EPS = [(130, 5, 31), (257, 70, 32)]


def default_eps_reference(n, d, seed, step):
    mu, lam = gaussian(d, seed)
    X0 = sampler_init(n, d, seed)
    eps = float(np.float32(1e-6))
    ref, dirs = A.jacobi64(X0, lambda X, t: O.score_gaussian(X, mu, lam), float(d), 1, step,
                           ALPHA, eps)
    return mu, lam, X0, eps, ref, dirs[0]


@pytest.mark.parametrize("n,d,seed", DEFAULT_EPS)
def test_sampler_adagrad_default_eps_one_step(n, d, seed):
    step = 0.05
    mu, lam, X0, eps, ref, phi = default_eps_reference(n, d, seed, step)
    M = np.abs(phi).max()
    keep = np.abs(phi) >= 1e-3 * M
    left = 1.0 - keep.mean()
    print("entries left out: %.3f %%" % (100 * left))
    assert left <= 0.01
    m = dsvgd()
    torch.manual_seed(seed)
    s = m.Sampler(d, m.targets.Gaussian(mu, lam), m.RBF(float(d)))
    df = s.sample(n, 1, step, order="jacobi", device=DEV, verbose=False, adagrad=True)
    vals = _values(df, (2, n, d))
    assert vals[0].tobytes() == X0.tobytes()
    got = vals[1].astype(np.float64)
    err = np.abs(got - ref[1])
    bound = step * (10.3 * eps / M + 8 * U)
    print("worst err %.3g of the bound %.3g" % (float(err[keep].max()), bound))
    record_parity(float(err[keep].max()))
    assert np.all(err[keep] <= bound)
    assert np.all(np.abs(got - X0.astype(np.float64)) <= step * (1 + 1e-6))


# ------------------------------------------------------- ksd_every --
def test_ksd_every_leaves_the_adagrad_trajectory_alone():
    n, d, seed, T, step = 130, 5, 21, 3, 0.05
    target, kernel, X0, eps, ref, _ = conditioned_reference("rbf", n, d, seed, T, step)
    m = dsvgd()
    out = {}
    for every in (None, 1):
        torch.manual_seed(seed)
        s = m.Sampler(d, target(), kernel())
        df = s.sample(n, T, step, order="jacobi", device=DEV, verbose=False, ksd_every=every,
                      adagrad=m.AdaGrad(0.9, eps))
        out[every] = _values(df, (T + 1, n, d))
        if every:
            diag = s.diagnostics
            assert list(diag["timestep"]) == [0, 1, 2, 3]
            assert np.isfinite(diag[["ksd", "ksd2_v", "ksd2_u", "h"]].to_numpy()).all()
    assert out[None].tobytes() == out[1].tobytes()


# ------------------------------------------------- DistSampler, S = 1 --
def dist1_reference(n, d, seed, steps, step, w2, hjko=10.0):
    """S = 1 over `steps` steps; with W2 the owned rows are shifted by a
    seeded perturbation before every step after the first (the previous
    particles are then not the current ones, and the h * W2 rows are live)."""
    mu, lam = gaussian(d, seed)
    rs = np.random.RandomState(seed)
    X0 = rs.randn(n, d).astype(np.float32)
    shifts = [None] + [(0.3 * rs.randn(n, d)).astype(np.float32) for _ in range(steps - 1)]
    h = float(d)
    score = lambda X: O.score_gaussian(X, mu, lam)     # noqa: E731

    def loop(eps):
        X, G = X0.astype(np.float64), np.full((n, d), -1.0)
        prev, out, dirs = None, [], []
        for t in range(steps):
            if w2 and shifts[t] is not None:
                # (what the particles setter stores: the fp32 sum)
                X = (X.astype(np.float32) + shifts[t]).astype(np.float64)
            p = O.phi(X, score(X), h)
            if w2 and prev is not None:
                p = p + hjko * O.w2_grad(X, prev)[0]
            dirs.append(p)
            X, G = A.update64(X, p, G, step, ALPHA, eps)
            prev = X.copy()
            out.append(X.copy())
        return out, dirs
    eps = float(np.float32(0.1 * np.abs(loop(1.0)[1][0]).max()))
    ref, dirs = loop(eps)
    return mu, lam, X0, shifts, eps, ref, dirs


def _dist1_run(n, d, seed, steps, step, w2, graphs, hjko=10.0):
    mu, lam, X0, shifts, eps, ref, dirs = dist1_reference(n, d, seed, steps, step, w2, hjko)
    m = dsvgd()
    ds = m.DistSampler(0, 1, m.targets.Gaussian(mu, lam), m.RBF(float(d)), gpu(X0).clone(), 1, 1,
                       False, False, w2, order="jacobi", adagrad=m.AdaGrad(0.9, eps))
    ds.graphs = graphs
    got = []
    for t in range(steps):
        if w2 and shifts[t] is not None:
            ds.particles = ds.particles + gpu(shifts[t])
        ds.make_step(step, h=hjko)
        torch.cuda.synchronize()
        got.append(ds.particles.cpu().numpy().copy())
    for p in dirs:
        assert step * 1e-5 * np.abs(p).max() / eps <= 1e-5
    return got, ref, dirs


def test_distsampler_adagrad_two_steps_match_fp64_graphs_on_and_off():
    n, d, steps, step = 130, 5, 2, 0.05
    on, ref, _ = _dist1_run(n, d, 41, steps, step, False, True)
    off, _, _ = _dist1_run(n, d, 41, steps, step, False, False)
    for t in range(steps):
        assert on[t].tobytes() == off[t].tobytes()
        assert _err(on[t], ref[t]) < TRAJ_TOL
    assert np.abs(ref[1] - ref[0]).max() > 100 * TRAJ_TOL


def test_distsampler_adagrad_with_the_w2_term_matches_fp64():
    n, d, steps, step = 130, 5, 2, 0.05
    got, ref, dirs = _dist1_run(n, d, 42, steps, step, True, True)
    for t in range(steps):
        assert _err(got[t], ref[t]) < TRAJ_TOL
    # the W2 rows are live in the second step's direction
    mu, lam, X0, shifts, eps, _, _ = dist1_reference(n, d, 42, steps, step, True)
    X1 = (ref[0].astype(np.float32) + shifts[1]).astype(np.float64)
    plain = O.phi(X1, O.score_gaussian(X1, mu, lam), float(d))
    assert np.abs(dirs[1] - plain).max() > 1e-2 * np.abs(plain).max()


# ------------------------------------------- DistSampler, S = 2 (gloo) --
def dist2_problem(seed=51, n=130, d=5):
    rs = np.random.RandomState(seed)
    X0 = rs.randn(n, d).astype(np.float32)
    params = [(rs.randn(d).astype(np.float32), rs.uniform(0.5, 2.0, d).astype(np.float32))
              for _ in range(2)]
    return X0, params


def dist2_reference(mode, steps, step, eps=None):
    """Every rank's owned rows after each step: the fp64 AdaGrad step over
    all n with that mode's scores (all_scores: the sum of the ranks' scores;
    all_particles: the rank's own, scaled N_global / N_local = 2)."""
    X0, params = dist2_problem()
    n, d = X0.shape
    per, h = n // 2, float(d)
    sc = [(lambda X, mu=mu, lam=lam: O.score_gaussian(X, mu, lam)) for mu, lam in params]

    def loop(eps):
        X, G = X0.astype(np.float64), np.full((n, d), -1.0)
        out, dirs = [], []
        for _ in range(steps):
            p = np.empty((n, d))
            for r in range(2):
                S = sc[0](X) + sc[1](X) if mode == "all_scores" else 2.0 * sc[r](X)
                rows = np.arange(r * per, (r + 1) * per)
                p[rows] = O.phi(X, S, h, rows=rows)
            dirs.append(p)
            X, G = A.update64(X, p, G, step, ALPHA, eps)
            out.append(X.copy())
        return out, dirs
    if eps is None:
        eps = float(np.float32(0.1 * np.abs(loop(1.0)[1][0]).max()))
    return eps, loop(eps)


def _dist2_worker(rank, port, mode, steps, step, eps, q):
    import os
    import sys
    import torch.distributed as dist
    from conftest import PKG, ROOT
    for p in (ROOT, PKG):
        sys.path.insert(0, p)
    import dsvgd as m
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    X0, params = dist2_problem()
    mu, lam = params[rank]
    ds = m.DistSampler(rank, 2, m.targets.Gaussian(mu, lam), m.RBF(float(X0.shape[1])),
                       torch.tensor(X0, device=DEV), 1, 2, exchange_particles=True,
                       exchange_scores=mode == "all_scores", include_wasserstein=False,
                       order="jacobi", adagrad=m.AdaGrad(0.9, eps))
    out = []
    for _ in range(steps):
        ds.make_step(step)
        torch.cuda.synchronize()
        out.append(ds.particles.cpu().numpy().copy())
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["all_scores", "all_particles"])
def test_distsampler_adagrad_two_ranks_match_fp64(mode):
    import torch.multiprocessing as mp
    steps, step = 2, 0.05
    eps, (ref, dirs) = dist2_reference(mode, steps, step)
    for p in dirs:
        assert step * 1e-5 * np.abs(p).max() / eps <= 1e-5
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29740 + ["all_scores", "all_particles"].index(mode)
    ps = [ctx.Process(target=_dist2_worker, args=(r, port, mode, steps, step, eps, q))
          for r in range(2)]
    for p in ps:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda r: r[0])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    per = ref[0].shape[0] // 2
    for rank, out in res:
        for t in range(steps):
            assert _err(out[t], ref[t][rank * per:(rank + 1) * per]) < TRAJ_TOL
    assert np.abs(ref[1] - ref[0]).max() > 100 * TRAJ_TOL


# ------------------------------------ DistSampler, the pair-split layout --
PS = dict(S=2, n=4096, d=256, N=1024, seed=71, h=2.0 * 256 * 0.01 / 8.0, steps=2, step=0.02)


def pair_split_problem():
    rs = np.random.RandomState(PS["seed"])
    d, N = PS["d"], PS["N"]
    x = (rs.randn(N, d - 1) / np.sqrt(d - 1)).astype(np.float32)
    t = np.where(rs.randn(N) > 0, 1.0, -1.0).astype(np.float32)
    X0 = (0.1 * rs.randn(PS["n"], d)).astype(np.float32)
    return x, t, X0


def pair_split_reference():
    """The fp64 AdaGrad loop over all n rows with the summed shard scores."""
    x, t, X0 = pair_split_problem()
    S, per = PS["S"], PS["N"] // PS["S"]

    def score(X):
        return sum(O.score_logreg(X, x[r * per:(r + 1) * per], t[r * per:(r + 1) * per])
                   for r in range(S))

    def loop(eps):
        X, G = X0.astype(np.float64), np.full(X0.shape, -1.0)
        out, dirs = [], []
        for _ in range(PS["steps"]):
            p = O.phi(X, score(X), PS["h"])
            dirs.append(p)
            X, G = A.update64(X, p, G, PS["step"], ALPHA, eps)
            out.append(X.copy())
        return out, dirs
    p0 = O.phi(X0.astype(np.float64), score(X0.astype(np.float64)), PS["h"])
    eps = float(np.float32(0.1 * np.abs(p0).max()))
    return (eps,) + loop(eps)


def _pair_split_worker(rank, port, eps, q):
    import os
    import sys
    import torch.distributed as dist
    from conftest import PKG, ROOT
    for p in (ROOT, PKG):
        sys.path.insert(0, p)
    import dsvgd as m
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    S = PS["S"]
    dist.init_process_group("gloo", rank=rank, world_size=S)
    x, t, X0 = pair_split_problem()
    per = PS["N"] // S
    tgt = m.targets.LogisticRegression(x[rank * per:(rank + 1) * per], t[rank * per:(rank + 1) * per])
    ds = m.DistSampler(rank, S, tgt, m.RBF(PS["h"]), torch.tensor(X0, device=DEV), per, per * S,
                       exchange_particles=True, exchange_scores=True, include_wasserstein=False,
                       order="jacobi", adagrad=m.AdaGrad(0.9, eps))
    out = []
    for _ in range(PS["steps"]):
        ds.make_step(PS["step"])
        torch.cuda.synchronize()
        eng = next(iter(ds._engines.values()))
        out.append((eng.plan is not None, ds.pair_split_check, len(ds._engines),
                    ds.particles.cpu().numpy().copy()))
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_distsampler_adagrad_pair_split_matches_fp64():
    """Two ranks in the pair-split layout: the first step is the layout's
    check (phi in both layouts, nothing moved, the rule applied once from the
    pair split's phi), the second a plain pair-split step on the history."""
    import torch.multiprocessing as mp
    eps, ref, dirs = pair_split_reference()
    for p in dirs:
        assert PS["step"] * 1e-5 * np.abs(p).max() / eps <= 1e-5
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_pair_split_worker, args=(r, 29745, eps, q)) for r in range(PS["S"])]
    for p in ps:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(PS["S"])], key=lambda r: r[0])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    per = PS["n"] // PS["S"]
    for rank, out in res:
        for t, (plan, check, engines, X) in enumerate(out):
            assert plan and engines == 1
            assert check is not None and check <= 1e-5
            assert _err(X, ref[t][rank * per:(rank + 1) * per]) < TRAJ_TOL
    assert np.abs(ref[1] - ref[0]).max() > 100 * TRAJ_TOL


# ------------------------------------------- the minibatch score kernel --
WINDOW_CASES = [(3, 2, 1, 1, 1, 1, 2), (33, 37, 5, 7, 10, 30, 3), (5, 300, 6, 10, 256, 0, 8),
                (5, 300, 6, 10, 257, 299, 8), (9, 70, 64, 64, 69, 5, 6)]


def iteration_of(N, B, c):
    """An iteration t whose window starts at c: (t B) mod N == c."""
    return next(t for t in range(N) if (t * B) % N == c)


@functools.lru_cache(maxsize=None)
def window_case(n, N, p, H, B, c, seed):
    X, Z, y = R.problem(n, N, p, H, seed)
    S, Asc, bound, count = A.minibatch_score64(X, Z, y, p, H, B, c)
    for a in (X, Z, y, S, Asc, bound):
        a.setflags(write=False)
    return X, Z, y, S, Asc, bound, count


def _bnn(Z, y, H, **kw):
    return dsvgd().targets.BayesianNN(torch.from_numpy(Z), torch.from_numpy(y), hidden=H, **kw)


@pytest.mark.parametrize("n,N,p,H,B,c,seed", WINDOW_CASES)
def test_window_score_matches_fp64(n, N, p, H, B, c, seed):
    X, Z, y, S, Asc, bound, count = window_case(n, N, p, H, B, c, seed)
    print("ambiguous triples: %d of %d" % (count, n * B * H))
    assert count <= max(1, AMBIGUOUS_CAP * n * B * H)
    tgt = _bnn(Z, y, H, batch=B)
    tgt.reset_batch(iteration_of(N, B, c))
    Xg = gpu(X)
    out = torch.full_like(Xg, float("nan"))
    tgt.score(Xg, out)
    assert int(tgt._cursor[Xg.device].cpu()[0]) == c
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - S)
    worst = float((err / Asc).max())
    print("worst err/A %.3g (entries over 1e-5 A, within the slack: %d)"
          % (worst, int((err > R.SCORE_TOL * Asc).sum())))
    record_parity(worst)
    assert np.all(err <= bound)
    # a scale applies to the sum
    tgt.score(Xg, out, scale=2.5)
    assert np.all(np.abs(out.cpu().numpy().astype(np.float64) - 2.5 * S) <= 2.5 * bound)


def test_window_cursor_and_full_batch_bits():
    n, N, p, H, B = 33, 37, 5, 7, 10
    X, Z, y = R.problem(n, N, p, H, 3)
    Xg = gpu(X)
    d = Xg.shape[1]
    # batch = N is the full-data target: its entry point, its bytes
    a, b = torch.empty_like(Xg), torch.empty_like(Xg)
    _bnn(Z, y, H).score(Xg, a)
    _bnn(Z, y, H, batch=N).score(Xg, b)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # next_batch() then score == reset_batch(1) then score, before and after
    # the cursor exists
    t1, t2 = _bnn(Z, y, H, batch=B), _bnn(Z, y, H, batch=B)
    t1.next_batch()
    t1.score(Xg, a)
    t2.reset_batch(1)
    t2.score(Xg, b)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    t1.next_batch()
    t1.score(Xg, a)
    t2.reset_batch(2)
    t2.score(Xg, b)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    S2 = A.minibatch_score64(X, Z, y, p, H, B, (2 * B) % N)
    assert np.all(np.abs(a.cpu().numpy().astype(np.float64) - S2[0]) <= S2[2])
    # the cursor after every advance, read back, past a whole cycle
    t2.reset_batch(0)
    for t in range(-(-N // B) * 2 + 3):
        assert int(t2._cursor[Xg.device].cpu()[0]) == (t * B) % N
        t2.next_batch()
    # the full-data twin scores all the data, with the same device tensors
    t2.full.score(Xg, b)
    _bnn(Z, y, H).score(Xg, a)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert d == R.dim(p, H)


# ------------------------------------ Sampler with a minibatch target --
BATCH_N, BATCH_B = 50, 20      # windows 0..19, 20..39, 40..49 + 0..9


def batch_problem(p, H, seed):
    _, Z, y = R.problem(1, BATCH_N, p, H, seed)
    return Z, y, A.minibatch_score_fn(Z, y, p, H, BATCH_B)


def test_sampler_minibatch_jacobi_matches_fp64_graphs_on_and_off():
    n, p, H, T, eps, seed = 130, 5, 7, 3, 1e-3, 61
    d = R.dim(p, H)
    Z, y, score = batch_problem(p, H, seed)
    m = dsvgd()
    out = {}
    for graphs in (True, False):
        torch.manual_seed(seed)
        s = m.Sampler(d, _bnn(Z, y, H, batch=BATCH_B), m.RBF(float(d)))
        df = s.sample(n, T, eps, order="jacobi", device=DEV, verbose=False, graphs=graphs)
        out[graphs] = _values(df, (T + 1, n, d))
    assert out[True].tobytes() == out[False].tobytes()
    ref = A.jacobi_fixed64(out[True][0], score, float(d), T, eps)
    assert _err(out[True], ref) < TRAJ_TOL
    assert np.abs(ref[-1] - ref[0]).max() > 100 * TRAJ_TOL
    # the windows matter: the full-data loop is far from this trajectory
    full = O.sampler_jacobi(out[True][0], lambda X: R.score64(X, Z, y, p, H)[0], float(d), T, eps)
    assert np.abs(full[-1] - ref[-1]).max() > 100 * TRAJ_TOL


def test_sampler_minibatch_sequential_matches_fp64_and_reruns_agree():
    n, p, H, T, eps, seed = 12, 5, 7, 2, 1e-3, 62
    d = R.dim(p, H)
    Z, y, score = batch_problem(p, H, seed)
    m = dsvgd()
    tgt = _bnn(Z, y, H, batch=BATCH_B)
    runs = []
    for _ in range(2):      # the same target twice: the cursor starts over
        torch.manual_seed(seed)
        s = m.Sampler(d, tgt, m.RBF(float(d)))
        df = s.sample(n, T, eps, order="sequential", device=DEV, verbose=False)
        runs.append(_values(df, (T + 1, n, d)))
    assert runs[0].tobytes() == runs[1].tobytes()
    ref = A.sequential64(runs[0][0], score, float(d), T, eps)
    assert _err(runs[0], ref) < TRAJ_TOL
    assert np.abs(ref[-1] - ref[0]).max() > 100 * TRAJ_TOL


def test_sampler_minibatch_jacobi_reruns_agree():
    n, p, H, T, eps, seed = 64, 5, 7, 3, 1e-3, 63
    d = R.dim(p, H)
    Z, y, _ = batch_problem(p, H, seed)
    m = dsvgd()
    tgt = _bnn(Z, y, H, batch=BATCH_B)
    runs = []
    for _ in range(2):
        torch.manual_seed(seed)
        s = m.Sampler(d, tgt, m.RBF(float(d)))
        df = s.sample(n, T, eps, order="jacobi", device=DEV, verbose=False, adagrad=True)
        runs.append(_values(df, (T + 1, n, d)))
    assert np.isfinite(runs[0]).all()
    assert runs[0].tobytes() == runs[1].tobytes()


# ------------------------------------------------------- experiment --
def test_experiment_runs_with_adagrad_and_minibatches():
    from test_bnn_host import experiment
    lines = []
    curve, ksd = experiment().run(32, 4, 1e-3, 2, hidden=10, rows=200, p=4, adagrad=True, batch=50,
                                  device=DEV, out=lines.append)
    assert [r["iteration"] for r in curve] == [0, 2, 4]
    assert all(np.isfinite(r["rmse"]) and np.isfinite(r["loglik"]) for r in curve)
    assert np.isfinite(ksd) and ksd >= 0
    assert len(lines) == 4 and lines[-1].startswith("final ksd")
