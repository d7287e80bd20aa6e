"""GPU tests of the minibatch logistic-regression score
(dsvgd_score_logreg_window, targets.LogisticRegression(batch=...)) and of the
samplers on it, against the fp64 references of tests/logreg_batch_reference.py.

The kernel: the two measures of tests/score_cases.py, the data rows taken
against the weighted data term (N / B) |g_i| with ROW_TOL = 1e-5
(tests/test_gpu_range.py) and column 0 with COL0_TOL; p = 1 by score_cases'
rule (the rows float32 itself cannot hold are judged against the sum of
magnitudes).  Every case runs at four origins -- 0, the window that ends on
the last row, the one that wraps by one row, the one that starts on the last
row -- over N = 3B + 7 data rows of which all but the window's hold 1e3 randn.

The samplers: the project's trajectory bound of 1e-4 (tests/test_gpu_adagrad.py)
on data sorted along the margin, where the fp64 references assert that the
particles move, and that the full-data trajectory lies away from the
minibatch one, by more than 100 times that bound."""
import functools

import numpy as np
import pytest
import torch

import adagrad_reference as A
import logreg_batch_reference as L
import score_cases as SC
from conftest import record_parity
from oracle import svgd_oracle as O
from test_gpu_adagrad import ALPHA, TRAJ_TOL, _values, sampler_init
from test_gpu_range import ROW_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
PATTERN = np.uint32(0x7fc0beef)   # a quiet NaN with a payload


def dsvgd():
    import dsvgd as m
    return m


def native():
    from dsvgd import _native as N
    return N


def gpu(a):
    return torch.as_tensor(np.array(a, order="C"), device=DEV)


def pattern(*shape):
    return np.full(shape, PATTERN, np.uint32).view(F32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _err(got, ref):
    e = float(np.abs(np.asarray(got, np.float64) - ref).max())
    record_parity(e)
    return e


def target(xd, t, **kw):
    return dsvgd().targets.LogisticRegression(torch.from_numpy(np.array(xd)),
                                              torch.from_numpy(np.array(t)), **kw)


# ----------------------------------------------------- kernel against fp64 --
KERNEL_CASES = L.table() + [L.window_case(65, 64, 128, "gen", strided=True),
                            L.window_case(129, 100, 1023, "pm1", strided=True),
                            L.window_case(1, 100, 255, "gen", strided=True),
                            L.window_case(33, 33, 33, "pm1", scale=2.5)]


def run_window(c, X, xd, t, origin):
    """One call of the entry point on NaN-padded buffers (strided cases: ldx =
    d + 3, lds = d + 1, ldxd = p + 2, the particles in the middle of their
    buffers); returns the n x d block after checking that no other cell of S
    changed.  The cursor holds origin + 5 N: it is taken mod N."""
    n, p, d, B = c.n, c.p, c.p + 1, c.N
    N = xd.shape[0]
    ldx, lds, ldxd, r0, s0 = (d + 3, d + 1, p + 2, 2, 1) if c.strided else (d, d, p, 0, 0)
    xb = np.full((N, ldxd), np.nan, F32)
    xb[:, :p] = xd
    Xb = np.full((n + 2 * r0, ldx), np.nan, F32)
    Xb[r0:r0 + n, :d] = X
    xg, tg, Xg = gpu(xb), gpu(np.asarray(t, F32)), gpu(Xb)
    Sg = gpu(pattern(n + 2 * s0, lds))
    cur = torch.tensor([origin + 5 * N], dtype=torch.int64, device=DEV)
    native().call("dsvgd_score_logreg_window", Xg[r0:].data_ptr(), ldx, n, d, xg.data_ptr(), ldxd,
                  tg.data_ptr(), N, float(c.scale), Sg[s0:].data_ptr(), lds, None, 0,
                  cur.data_ptr(), B, native().stream(torch.device(DEV)))
    torch.cuda.synchronize()
    assert int(cur.cpu()[0]) == origin + 5 * N          # read, never written
    full = Sg.cpu().numpy()
    out = full[s0:s0 + n, :d].copy()
    full[s0:s0 + n, :d] = pattern(n, d)
    assert same_bits(full, pattern(*full.shape)), "a cell outside the n x d block was written"
    return out


def judge(c, chk, S):
    k, ref, w, rows, absg, a32, _ = chk
    assert np.isfinite(S).all(), ("not finite", SC.case_id(c))
    got = S.astype(np.float64) / c.scale
    c0 = float(SC.col0_rows(got, ref, k.P).max())
    e = float(L.weighted_rows(got, ref, k.P.g, w)[rows].max(initial=0.0))
    if not rows.all():                      # the ill-conditioned rows of p = 1, by rule
        x = ~rows
        e = max(e, float((np.abs(got[x, 1] - ref[x, 1]) / (w * absg[x, 0])).max()))
    return e, c0


def kernel_id(c):
    return SC.case_id(c) + ("-scale%g" % c.scale if c.scale != 1.0 else "")


@pytest.mark.parametrize("c", KERNEL_CASES, ids=[kernel_id(c) for c in KERNEL_CASES])
def test_window_kernel_matches_fp64_at_every_origin(c):
    chk = L.checked(c, ROW_TOL)
    k = chk[0]
    worst, worst0, first = 0.0, 0.0, None
    for org in L.origins(c.N):
        xd, t = L.place(c, k, org)
        S = run_window(c, k.X, xd, t, org)
        e, c0 = judge(c, chk, S)
        print("%s origin %d: data %.3g (fp32 %.3g) col0 %.3g" % (SC.case_id(c), org, e, chk[5], c0))
        worst, worst0 = max(worst, e), max(worst0, c0)
        if first is None:
            first = S
            assert same_bits(run_window(c, k.X, xd, t, org), S)     # two runs: the same bits
    record_parity(worst, col0=worst0, group="W", draw=k.draw)
    assert worst <= ROW_TOL, ("data rows", SC.case_id(c), worst)
    assert worst0 <= SC.COL0_TOL, ("column 0", SC.case_id(c), worst0)


@pytest.mark.parametrize("n,B,p", [(1, 100, 255), (33, 33, 33), (64, 100, 255), (129, 100, 1023)])
def test_rows_outside_the_window_do_not_reach_the_result(n, B, p):
    """Every row and label outside the window NaN (row 0 among them; B is no
    multiple of 32, so the last chunk has pad rows): the same bits as with
    the finite filler."""
    c = L.window_case(n, B, p, "pm1")
    k = L.checked(c, ROW_TOL)[0]
    for org in (L.data_rows_total(B) - B, 5):
        xd, t = L.place(c, k, org)
        ref = run_window(c, k.X, xd, t, org)
        rest = np.setdiff1d(np.arange(xd.shape[0]), L.window(xd.shape[0], B, org))
        assert 0 in rest
        xd[rest], t[rest] = np.nan, np.nan
        got = run_window(c, k.X, xd, t, org)
        assert np.isfinite(got).all() and same_bits(got, ref)


# -------------------------------------------------------- cursor semantics --
def test_cursor_advance_equals_reset_across_a_wrap_and_full_batch_bits():
    c = L.window_case(33, 33, 33, "pm1")
    k = L.checked(c, ROW_TOL)[0]
    N, B = 80, 33                                   # windows 0, 33, 66 (wraps), 19, ...
    rs = np.random.RandomState(5)
    xd = (rs.randn(N, c.p) / np.sqrt(c.p)).astype(F32)
    t = np.where(rs.randn(N) > 0, 1.0, -1.0).astype(F32)
    Xg = gpu(k.X)
    a, b = torch.empty_like(Xg), torch.empty_like(Xg)
    # batch = N is the full-data target: its entry points, its bytes
    target(xd, t).score(Xg, a)
    tn = target(xd, t, batch=N)
    assert tn.batch is None
    tn.score(Xg, b)
    assert same_bits(a.cpu().numpy(), b.cpu().numpy())
    # next_batch() then score == reset_batch(it) then score, before and after
    # the cursor exists
    t1, t2 = target(xd, t, batch=B), target(xd, t, batch=B)
    for it in range(1, 6):
        t1.next_batch()
        t1.score(Xg, a)
        t2.reset_batch(it)
        t2.score(Xg, b)
        assert int(t1._cursor[Xg.device].cpu()[0]) == (it * B) % N
        assert same_bits(a.cpu().numpy(), b.cpu().numpy())
        ref = L.window_score64(k.X, xd, t, B, (it * B) % N)[0]
        assert np.abs(a.cpu().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()
    # two calls of one window: the same bits; the next window: other bits
    t2.score(Xg, a)
    assert same_bits(a.cpu().numpy(), b.cpu().numpy())
    t2.next_batch()
    t2.score(Xg, a)
    assert not same_bits(a.cpu().numpy(), b.cpu().numpy())
    # the full-data twin scores all the data
    t2.full.score(Xg, b)
    target(xd, t).score(Xg, a)
    assert same_bits(a.cpu().numpy(), b.cpu().numpy())


# ----------------------------------------------------- sampler trajectories --
@functools.lru_cache(maxsize=None)
def traj_case(n, p, N, B, T, eps, seed):
    """(xd, t, X0, the fp64 minibatch trajectory, the fp64 full-data one)."""
    xd, t = L.sorted_problem(N, p, seed)
    d = p + 1
    X0 = sampler_init(n, d, seed)
    ref = A.jacobi_fixed64(X0, L.window_score_fn(xd, t, B), float(d), T, eps)
    full = O.sampler_jacobi(X0, lambda X: O.score_logreg(X, xd, t), float(d), T, eps)
    return xd, t, X0, ref, np.asarray(full)


# (n, p, N, B, T, eps, seed); the last: d = 256, the MFMA path of the step
TRAJ = [(64, 7, 300, 50, 8, 1e-2, 81), (300, 15, 257, 100, 5, 5e-3, 82),
        (256, 255, 100, 40, 3, 5e-2, 83)]


@pytest.mark.parametrize("n,p,N,B,T,eps,seed", TRAJ)
def test_sampler_jacobi_matches_fp64_graphs_on_and_off(n, p, N, B, T, eps, seed):
    xd, t, X0, ref, full = traj_case(n, p, N, B, T, eps, seed)
    d = p + 1
    assert T * B > N                                          # the windows wrap the data
    move, apart = np.abs(ref[-1] - ref[0]).max(), np.abs(full[-1] - ref[-1]).max()
    print("fp64: moved %.3g, full-data trajectory %.3g away" % (move, apart))
    assert move > 100 * TRAJ_TOL and apart > 100 * TRAJ_TOL
    m = dsvgd()
    out = {}
    tgt = target(xd, t, batch=B)
    for graphs in (True, False, True):                         # (the third: a rerun)
        torch.manual_seed(seed)
        s = m.Sampler(d, tgt, m.RBF(float(d)))
        df = s.sample(n, T, eps, order="jacobi", device=DEV, verbose=False, graphs=graphs)
        vals = _values(df, (T + 1, n, d))
        if graphs in out:
            assert out[graphs].tobytes() == vals.tobytes()     # the same seed: the same bits
        out[graphs] = vals
    assert out[True][0].tobytes() == X0.tobytes()
    assert out[True].tobytes() == out[False].tobytes()
    assert _err(out[True], ref) < TRAJ_TOL


@pytest.mark.parametrize("n", [48, 130])
def test_sampler_sequential_takes_the_per_row_path(n):
    """n = 48: below the blocked sweeps anyway; n = 130: the blocked sweeps
    would refresh the scores from all of the data, so _gs_score_kind sends a
    batched target to the per-row path.  Either way the moved row's score
    comes from the one-particle window call."""
    p, N, B, T, eps, seed = 7, 300, 50, 2, 1e-2, 84 + n
    d = p + 1
    xd, t = L.sorted_problem(N, p, seed)
    X0 = sampler_init(n, d, seed)
    ref = A.sequential64(X0, L.window_score_fn(xd, t, B), float(d), T, eps)
    full = np.asarray(O.sampler_sequential(X0, lambda X: O.score_logreg(X, xd, t), float(d), T, eps))
    assert np.abs(ref[-1] - ref[0]).max() > 100 * TRAJ_TOL
    assert np.abs(full[-1] - ref[-1]).max() > 100 * TRAJ_TOL
    m = dsvgd()
    tgt = target(xd, t, batch=B)
    runs = []
    for _ in range(2):      # the same target twice: the cursor starts over
        torch.manual_seed(seed)
        s = m.Sampler(d, tgt, m.RBF(float(d)))
        df = s.sample(n, T, eps, order="sequential", device=DEV, verbose=False)
        runs.append(_values(df, (T + 1, n, d)))
    assert runs[0].tobytes() == runs[1].tobytes()
    assert _err(runs[0], ref) < TRAJ_TOL


def test_sampler_adagrad_with_batches_matches_fp64():
    n, p, N, B, T, step, seed = 130, 7, 300, 50, 4, 0.05, 87
    d = p + 1
    xd, t = L.sorted_problem(N, p, seed)
    X0 = sampler_init(n, d, seed)
    score = L.window_score_fn(xd, t, B)
    _, dirs = A.jacobi64(X0, score, float(d), 1, step, ALPHA, 1.0)
    eps = float(np.float32(0.1 * np.abs(dirs[0]).max()))
    ref, dirs = A.jacobi64(X0, score, float(d), T, step, ALPHA, eps)
    for q in dirs:    # the phi bound, amplified by at most 1 / eps
        assert step * 1e-5 * np.abs(q).max() / eps <= 1e-5
    full, _ = A.jacobi64(X0, lambda X, it: O.score_logreg(X, xd, t), float(d), T, step, ALPHA, eps)
    assert np.abs(ref[-1] - ref[0]).max() > 100 * TRAJ_TOL
    assert np.abs(full[-1] - ref[-1]).max() > 100 * TRAJ_TOL
    m = dsvgd()
    out = {}
    for graphs in (True, False):
        torch.manual_seed(seed)
        s = m.Sampler(d, target(xd, t, batch=B), m.RBF(float(d)))
        df = s.sample(n, T, step, order="jacobi", device=DEV, verbose=False, graphs=graphs,
                      adagrad=m.AdaGrad(0.9, eps))
        out[graphs] = _values(df, (T + 1, n, d))
    assert out[True].tobytes() == out[False].tobytes()
    assert _err(out[True], ref) < TRAJ_TOL


# ------------------------------------------------------------ DistSampler --
DIST = dict(n=130, p=7, N=300, B=40, steps=3, eps=1e-2, seed=91)


def dist_problem():
    xd, t = L.sorted_problem(DIST["N"], DIST["p"], DIST["seed"])
    rs = np.random.RandomState(DIST["seed"])
    X0 = (0.5 * rs.randn(DIST["n"], DIST["p"] + 1)).astype(F32)
    return xd, t, X0


def test_distsampler_one_rank_matches_fp64_graphs_on_and_off():
    xd, t, X0 = dist_problem()
    d, steps, eps, B = X0.shape[1], DIST["steps"], DIST["eps"], DIST["B"]
    ref = A.jacobi_fixed64(X0, L.window_score_fn(xd, t, B), float(d), steps, eps)
    full = np.asarray(O.sampler_jacobi(X0, lambda X: O.score_logreg(X, xd, t), float(d), steps, eps))
    assert np.abs(ref[-1] - ref[0]).max() > 100 * TRAJ_TOL
    assert np.abs(full[-1] - ref[-1]).max() > 100 * TRAJ_TOL
    m = dsvgd()
    out = {}
    for graphs in (True, False):
        ds = m.DistSampler(0, 1, target(xd, t, batch=B), m.RBF(float(d)), gpu(X0).clone(), 1, 1,
                           False, False, False, order="jacobi")
        ds.graphs = graphs
        got = []
        for _ in range(steps):
            ds.make_step(eps)
            torch.cuda.synchronize()
            got.append(ds.particles.cpu().numpy().copy())
        out[graphs] = np.stack(got)
    assert out[True].tobytes() == out[False].tobytes()
    assert _err(out[True], ref[1:]) < TRAJ_TOL


def _dist2_worker(rank, port, mode, q):
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
    xd, t, X0 = dist_problem()
    per = xd.shape[0] // 2
    tgt = m.targets.LogisticRegression(xd[rank * per:(rank + 1) * per],
                                       t[rank * per:(rank + 1) * per], batch=DIST["B"])
    xs = mode == "all_scores"
    refused = None
    if xs:
        try:
            m.DistSampler(rank, 2, tgt, m.RBF(float(X0.shape[1])), torch.tensor(X0, device=DEV), per,
                          2 * per, True, True, False, order="jacobi", gather_data=True)
        except ValueError as e:
            refused = str(e)
    ds = m.DistSampler(rank, 2, tgt, m.RBF(float(X0.shape[1])), torch.tensor(X0, device=DEV), per,
                       2 * per, exchange_particles=xs, exchange_scores=xs,
                       include_wasserstein=False, order="jacobi")
    before = ds._gdata
    out = []
    for _ in range(2):
        ds.make_step(DIST["eps"])
        torch.cuda.synchronize()
        out.append(ds.particles.cpu().numpy().copy())
    q.put((rank, out, before, ds._gdata, refused))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["all_scores", "partitions"])
def test_distsampler_two_ranks_match_the_oracle(mode):
    import torch.multiprocessing as mp
    xd, t, X0 = dist_problem()
    per = xd.shape[0] // 2
    shards = [(xd[r * per:(r + 1) * per], t[r * per:(r + 1) * per]) for r in range(2)]
    scores = L.RankScores(shards, DIST["B"])
    xs = mode == "all_scores"
    D = O.DistOracle([X0] * 2, scores.fns, per, 2 * per, xs, xs, h=float(X0.shape[1]),
                     sequential=False)
    plain = O.DistOracle([X0] * 2, [lambda X, s=s: O.score_logreg(X, *s) for s in shards], per,
                         2 * per, xs, xs, h=float(X0.shape[1]), sequential=False)
    ref = []
    for it in range(2):
        scores.it = it
        D.step(DIST["eps"])
        plain.step(DIST["eps"])
        ref.append([D.own(r).copy() for r in range(2)])
    assert max(np.abs(ref[1][r] - plain.own(r)).max() for r in range(2)) > 100 * TRAJ_TOL
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29760 + ["all_scores", "partitions"].index(mode)
    ps = [ctx.Process(target=_dist2_worker, args=(r, port, mode, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda r: r[0])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    for rank, out, before, after, refused in res:
        for it in range(2):
            assert _err(out[it], ref[it][rank]) < TRAJ_TOL
        if xs:
            # gather_data=None: undecided until the first step, then off; True: refused
            assert before is None and after is False
            assert refused is not None and "window" in refused
        else:
            assert before is False and after is False


# ------------------------------------------------------- KSD, experiment --
def test_ksd_scores_a_batched_target_on_all_of_its_data():
    xd, t, X0 = dist_problem()
    m = dsvgd()
    Xg = gpu(X0)
    a = m.metrics.ksd(Xg, target(xd, t, batch=DIST["B"]), m.RBF(8.0))
    b = m.metrics.ksd(Xg, target(xd, t, batch=DIST["B"]).full, m.RBF(8.0))
    c = m.metrics.ksd(Xg, target(xd, t), m.RBF(8.0))
    assert a == b == c and np.isfinite(a) and a > 0


def test_experiment_runs_with_batch_and_adagrad(tmp_path):
    import importlib.util
    import os
    from conftest import PKG
    spec = importlib.util.spec_from_file_location(
        "logreg_experiment", os.path.join(PKG, "experiments", "logreg.py"))
    exp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(exp)
    curve = exp.run(0, 1, "banana", 42, 40, 6, 1e-2, "partitions", False, str(tmp_path),
                    order="jacobi", device=DEV, batch=50, adagrad=True, curve=True)
    assert [r["timestep"] for r in curve] == list(range(7))
    assert all(np.isfinite(r["dsvgd"]) and 0.0 <= r["dsvgd"] <= 1.0 for r in curve)
    assert os.path.isfile(os.path.join(str(tmp_path), "shard-0.pkl"))


def test_experiment_cli_options_reach_the_target_and_the_sampler(tmp_path, monkeypatch):
    """Through the command line (one process): --batch and --adagrad arrive at
    the LogisticRegression target and at DistSampler, and without them both
    are built as before."""
    import importlib.util
    import os
    from click.testing import CliRunner
    from conftest import PKG
    spec = importlib.util.spec_from_file_location(
        "logreg_experiment_cli", os.path.join(PKG, "experiments", "logreg.py"))
    exp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(exp)
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    seen = []
    real = exp.dsvgd.DistSampler

    def spy(rank, S, tgt, *a, **kw):
        ds = real(rank, S, tgt, *a, **kw)
        seen.append((tgt.batch, kw.get("adagrad"), ds))
        return ds
    monkeypatch.setattr(exp.dsvgd, "DistSampler", spy)
    base = ["--nproc", "1", "--nparticles", "40", "--niter", "3", "--stepsize", "1e-2",
            "--order", "jacobi", "--no-plots", "--results-dir", str(tmp_path)]
    for flags, batch, ada in ((["--batch", "50", "--adagrad"], 50, True), ([], None, None)):
        res = CliRunner().invoke(exp.cli, base + flags, catch_exceptions=False)
        assert res.exit_code == 0, res.output
        got_batch, got_ada, ds = seen.pop()
        assert got_batch == batch and got_ada == ada
        assert (ds._ada is not None) == bool(ada)
        assert np.isfinite(ds.particles.cpu().numpy()).all()
