"""Host-side checks of the minibatch logistic-regression target (no GPU): the
fp64 window score of tests/logreg_batch_reference.py pinned to the project's
oracle, the kernel suite's case table and its preconditions, the target's
batch argument, digest, cursor and full-data twin, the combinations
DistSampler refuses, and the new entry point with its argument checks.

Figures of the table below at ROW_TOL = 1e-5 (every case at draw 0): the
worst float32 restatement of the weighted measure is 9.6e-7 (p = 1), and the
row outside the window that moves the measure least moves it by 2.6 (p = 1;
over 200 everywhere else), against the 1e-3 required."""
import ctypes

import numpy as np
import pytest
import torch

import logreg_batch_reference as L
import score_cases as SC
from oracle import svgd_oracle as O

ROW_TOL = 1e-5          # tests/test_gpu_range.py (importing it would ask for a GPU mark)
TABLE = L.table()


def _problem(n=7, N=23, p=5, seed=4):
    rs = np.random.RandomState(seed)
    X = np.empty((n, p + 1), np.float32)
    X[:, 1:] = 0.3 * rs.randn(n, p)
    X[:, 0] = rs.uniform(-3.0, -1.0, n)
    xd = (rs.randn(N, p) / np.sqrt(p)).astype(np.float32)
    t = np.where(rs.randn(N) > 0, 1.0, -1.0).astype(np.float32)
    return X, xd, t


def _target(xd, t, **kw):
    from dsvgd.targets import LogisticRegression
    return LogisticRegression(torch.from_numpy(xd), torch.from_numpy(t), **kw)


# ------------------------------------------------------ reference pinned --
def test_whole_window_is_the_oracle_score():
    X, xd, t = _problem()
    S, _, w = L.window_score64(X, xd, t, xd.shape[0], 0)
    ref = O.score_logreg(X, xd, t)
    assert w == 1.0
    assert np.abs(S - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("B", [1, 5, 22])
def test_mean_over_all_origins_is_the_full_score(B):
    """Each row lies in exactly B of the N windows: the estimate is unbiased."""
    X, xd, t = _problem()
    N = xd.shape[0]
    mean = sum(L.window_score64(X, xd, t, B, c)[0] for c in range(N)) / N
    ref = O.score_logreg(X, xd, t)
    assert np.abs(mean - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max())


def test_window_rows_wrap():
    assert list(L.window(10, 4, 8)) == [8, 9, 0, 1]
    assert L.origins(5) == [0, 17, 18, 21] and L.data_rows_total(5) == 22


# ----------------------------------------------------------- case table --
def test_table_holds_the_kernel_suite_shapes_with_both_label_kinds():
    got = {(c.n, c.N, c.p, c.labels) for c in TABLE}
    for n, B, p in L.SHAPES:
        for lab in L.LABELS:
            assert (n, B, p, lab) in got
    assert all(c.group == "W" and c.path == "window" for c in TABLE)


@pytest.mark.parametrize("c", TABLE, ids=[SC.case_id(c) for c in TABLE])
def test_case_meets_the_preconditions(c):
    k, ref, w, rows, absg, a32, change = L.checked(c, ROW_TOL)
    print("%s: draw %d, float32 %.3g, extra row %.3g" % (SC.case_id(c), k.draw, a32, change))
    assert k.draw == 0
    assert w == (3 * c.N + 7) / c.N
    assert a32 <= ROW_TOL / 10
    assert change >= SC.SENS * ROW_TOL
    assert rows.all() or c.p == 1
    # the placed data: the window's rows are the checked ones at every origin
    for org in L.origins(c.N):
        xd, t = L.place(c, k, org)
        win = L.window(xd.shape[0], c.N, org)
        assert np.array_equal(xd[win], k.xd) and np.array_equal(t[win], k.t)
        S, _, w2 = L.window_score64(k.X, xd, t, c.N, org)
        assert w2 == w and np.array_equal(S, ref)
        rest = np.setdiff1d(np.arange(xd.shape[0]), win)
        assert np.abs(xd[rest]).max() > 100 and set(np.unique(t[rest])) <= {-1.0, 1.0}


def test_skipped_mutations_stay_within_the_cap():
    """B = 1 has no row to drop, p = 1 no column: by rule, under the cap."""
    for cases in (L.table(L.SHAPES), TABLE):
        skipped = [c for c in cases if SC.mutations(c)[1]]
        assert all(c.N == 1 or c.p == 1 for c in skipped)
        assert len(skipped) <= SC.SKIP_CAP * len(cases)


# ------------------------------------------------ argument rules and twin --
def test_batch_argument_digest_and_full_twin():
    X, xd, t = _problem()
    N = xd.shape[0]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            _target(xd, t, batch=bad)
    full = _target(xd, t)
    assert full.batch is None and full.full is full
    for whole in (N, N + 1, 1000):
        tg = _target(xd, t, batch=whole)
        assert tg.batch is None and tg.fingerprint() == full.fingerprint()
    mb = _target(xd, t, batch=5)
    assert mb.batch == 5
    assert mb.fingerprint() != full.fingerprint()
    assert mb.fingerprint() != _target(xd, t, batch=6).fingerprint()
    assert mb.fingerprint() == _target(xd.copy(), t.copy(), batch=5).fingerprint()
    twin = mb.full
    assert twin is mb.full and twin.batch is None and twin.full is twin
    assert type(twin) is type(mb) and twin.gemm == mb.gemm
    assert twin.x is mb.x and twin.t is mb.t and twin._dev is mb._dev and twin._ws is mb._ws
    assert twin.fingerprint() == full.fingerprint()
    x = torch.from_numpy(X[0].copy())
    assert float(mb.logp(x)) == float(full.logp(x))      # logp stays the full-data density
    assert full.next_batch() is None and full.reset_batch(3) is None


def test_next_batch_before_any_device_moves_the_origin():
    _, xd, t = _problem()
    N = xd.shape[0]
    mb = _target(xd, t, batch=5)
    assert mb._origin == 0 and mb._cursor == {}
    for it in range(1, 12):
        mb.next_batch()
        assert mb._origin == (5 * it) % N
    mb.reset_batch(7)
    assert mb._origin == (7 * 5) % N
    mb.reset_batch()
    assert mb._origin == 0


def test_blocked_sweeps_leave_a_batched_target_to_the_per_row_path():
    from dsvgd.engine import _gs_score_kind
    _, xd, t = _problem()
    assert _gs_score_kind(_target(xd, t)) == 3
    assert _gs_score_kind(_target(xd, t, batch=5)) is None
    assert _gs_score_kind(_target(xd, t, batch=5).full) == 3


def test_distsampler_refuses_gathered_data_with_a_batch():
    import dsvgd
    _, xd, t = _problem()
    X = torch.zeros(80, xd.shape[1] + 1)

    def make(tgt, **kw):
        return dsvgd.DistSampler(0, 2, tgt, dsvgd.RBF(1.0), X, xd.shape[0], 2 * xd.shape[0], True,
                                 True, False, order="jacobi", **kw)
    with pytest.raises(ValueError, match="window"):
        make(_target(xd, t, batch=5), gather_data=True)
    with pytest.raises(ValueError, match="prior_weight"):
        _target(xd, t, batch=5).score(torch.zeros(40, 6), torch.zeros(40, 6), prior_weight=2.0)


# ------------------------------------------------------- library exports --
def test_library_exports_the_window_entry_point_and_abi_stays_4():
    import os
    from dsvgd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include",
                               "dsvgd.h")).read()
    for name in ("dsvgd_score_logreg_window", "dsvgd_logreg_window_workspace_bytes"):
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES
        assert name + "(" in header
    assert _native.load().dsvgd_abi_version() == 4
    assert _native.load().dsvgd_logreg_window_workspace_bytes(65536, 100, 255) == 0


def test_entry_point_validates_arguments_without_gpu():
    """Every call below fails a check: none reaches a launch."""
    from dsvgd import _native as N
    lib = N.load()
    buf = (ctypes.c_double * 64)()
    q = ctypes.addressof(buf)
    d = 6

    def call(a, n=2, d_=d, ldx=d, ldxd=d - 1, N_=9, lds=d, engine=0, B=4):
        return lib.dsvgd_score_logreg_window(a[0], ldx, n, d_, a[1], ldxd, a[2], N_, 1.0, a[3], lds,
                                             None, engine, a[4], B, None)

    def err():
        return lib.dsvgd_last_error()
    for null in range(5):
        a = [q] * 5
        a[null] = None
        assert call(a) == -1 and b"null" in err()
    full = [q] * 5
    for kw in (dict(n=0), dict(d_=1, ldxd=1), dict(N_=0, B=0), dict(ldx=d - 1), dict(lds=d - 1),
               dict(ldxd=d - 2)):
        assert call(full, **kw) == -1 and b"sizes" in err()
    assert call(full, d_=1025, ldx=1025, lds=1025, ldxd=1024) == -1 and b"1023" in err()
    for engine in (-1, 3):
        assert call(full, engine=engine) == -1 and b"engine" in err()
    for B in (0, -3, 10):
        assert call(full, B=B) == -1 and b"1 <= B <= N" in err()


# ------------------------------------------- the experiment's launch paths --
def _harness():
    import importlib.util
    import os
    from conftest import PKG
    spec = importlib.util.spec_from_file_location(
        "dsvgd_logreg_experiment_batch", os.path.join(PKG, "experiments", "logreg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Launch(object):
    """The experiment module with run() and the process-group calls recorded
    instead of executed: what each launch path hands to which."""

    def __init__(self, monkeypatch, gpus):
        self.H = H = _harness()
        self.runs, self.groups, self.spawned = [], [], []
        monkeypatch.setattr(H, "run", lambda *a, **kw: self.runs.append((a, kw)))
        monkeypatch.setattr(H.dist, "init_process_group",
                            lambda *a, **kw: self.groups.append((a, kw)))
        monkeypatch.setattr(H.dist, "barrier", lambda *a, **kw: None)
        monkeypatch.setattr(H.dist, "destroy_process_group", lambda *a, **kw: None)
        monkeypatch.setattr(H.torch.cuda, "device_count", lambda: gpus)
        monkeypatch.setattr(H.torch.multiprocessing, "spawn",
                            lambda fn, args, nprocs, join: self.spawned.append((fn, args, nprocs)))
        for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
            monkeypatch.delenv(name, raising=False)

    def cli(self, tmp_path, *flags):
        from click.testing import CliRunner
        res = CliRunner().invoke(self.H.cli, ["--no-plots", "--results-dir", str(tmp_path)]
                                 + list(flags), catch_exceptions=False)
        assert res.exit_code == 0, res.output
        return res


FLAGS = ["--batch", "50", "--adagrad", "--order", "jacobi"]
RUN_KEYS = {"batch", "adagrad", "device"}       # the keywords run() takes from a launch


@pytest.mark.parametrize("flags,want", [(FLAGS, dict(batch=50, adagrad=True)),
                                        ([], dict(batch=None, adagrad=False))])
def test_cli_single_process_hands_the_options_to_run(monkeypatch, tmp_path, flags, want):
    L_ = _Launch(monkeypatch, gpus=1)
    L_.cli(tmp_path, "--nproc", "1", *flags)
    (a, kw), = L_.runs
    assert a[:2] == (0, 1) and kw == want and not L_.groups


@pytest.mark.parametrize("gpus", [1, 2])         # gloo (ranks share a GPU) and nccl
@pytest.mark.parametrize("flags,want", [(FLAGS, dict(batch=50, adagrad=True)),
                                        ([], dict(batch=None, adagrad=False))])
def test_cli_under_torchrun_keeps_run_and_process_group_keywords_apart(monkeypatch, tmp_path,
                                                                       gpus, flags, want):
    L_ = _Launch(monkeypatch, gpus=gpus)
    for name, v in (("WORLD_SIZE", "2"), ("RANK", "1"), ("LOCAL_RANK", "1")):
        monkeypatch.setenv(name, v)
    L_.cli(tmp_path, *flags)
    (a, kw), = L_.runs
    assert a[:2] == (1, 2)
    assert set(kw) <= RUN_KEYS and {k: kw[k] for k in want} == want
    assert kw["device"] == "cuda:%d" % (1 % gpus)
    (ga, gkw), = L_.groups
    assert ga == ("nccl" if gpus >= 2 else "gloo",)
    assert ("device_id" in gkw) == (gpus >= 2) and not set(gkw) & RUN_KEYS


@pytest.mark.parametrize("gpus", [1, 2])
@pytest.mark.parametrize("flags,want", [(FLAGS, dict(batch=50, adagrad=True)),
                                        ([], dict(batch=None, adagrad=False))])
def test_cli_spawned_ranks_receive_the_options(monkeypatch, tmp_path, gpus, flags, want):
    L_ = _Launch(monkeypatch, gpus=gpus)
    L_.cli(tmp_path, "--nproc", "2", *flags)
    (fn, args, nprocs), = L_.spawned
    assert fn is L_.H._init_distributed and nprocs == 2 and not L_.runs
    fn(1, *args)                                   # what spawn runs as rank 1
    (a, kw), = L_.runs
    assert a[:2] == (1, 2) and kw == want
    (ga, gkw), = L_.groups
    assert ga == ("nccl" if gpus >= 2 else "gloo",)
    assert gkw["rank"] == 1 and gkw["world_size"] == 2
    assert ("device_id" in gkw) == (gpus >= 2) and not set(gkw) & RUN_KEYS
