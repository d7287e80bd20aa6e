"""Host-side checks of the softmax-regression target (no GPU): the fp64 closed
form of tests/softmax_reference.py against fp64 autograd of
SoftmaxRegression.logp, the target's validation and digest, the new symbols,
the argument checks of the entry points, and an fp32 restatement chunked like
the kernel, which stays under a tenth of the GPU bound on every table shape:
the bound is the kernel's to miss, not the inputs'."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import softmax_reference as R
from conftest import ROOT


def _target(Xd, y, **kw):
    from dsvgd.targets import SoftmaxRegression
    return SoftmaxRegression(torch.from_numpy(Xd), torch.from_numpy(y), **kw)


def test_score64_matches_fp64_autograd_of_logp():
    n, N, C, p = 3, 37, 4, 5
    X, Xd, y = R.problem(n, N, C, p, seed=3)
    tgt = _target(Xd, y)
    assert (tgt.N, tgt.p, tgt.C, tgt.d) == (N, p, C, R.dim(C, p))
    S, A = R.score64(X, Xd, y, C)
    for i in range(n):
        x = torch.from_numpy(X[i].astype(np.float64)).requires_grad_(True)
        (g,) = torch.autograd.grad(tgt.logp(x), x)
        assert np.all(np.abs(g.numpy() - S[i]) <= 1e-10 * np.abs(S[i]) + 1e-13 * A[i])
    la, W = tgt.unpack(torch.from_numpy(X[0]))
    assert la == X[0, 0] and W.shape == (C, p) and W[1, 2] == X[0, 1 + p + 2]
    # other hyper-prior parameters reach both the closed form and logp
    tgt2 = _target(Xd, y, a0=2.0, b0=0.5)
    S2, A2 = R.score64(X, Xd, y, C, 2.0, 0.5)
    x = torch.from_numpy(X[0].astype(np.float64)).requires_grad_(True)
    (g,) = torch.autograd.grad(tgt2.logp(x), x)
    assert np.all(np.abs(g.numpy() - S2[0]) <= 1e-10 * np.abs(S2[0]) + 1e-13 * A2[0])
    assert abs(S2[0, 0] - S[0, 0]) > 0.1
    # under vmap, as CallableTarget would run it
    g = torch.func.vmap(torch.func.grad(tgt.logp))(torch.from_numpy(X).double()).numpy()
    assert np.all(np.abs(g - S) <= 1e-10 * np.abs(S) + 1e-13 * A)
    assert tgt(torch.from_numpy(X[0])).shape == ()


def test_window_estimate_is_the_full_score_when_the_window_is_everything():
    n, N, C, p = 2, 23, 3, 4
    X, Xd, y = R.problem(n, N, C, p, seed=5)
    S, A = R.score64(X, Xd, y, C)
    for org in (0, 7, N - 1):
        Sw, _ = R.score64(X, Xd, y, C, origin=org, B=N)
        assert np.all(np.abs(Sw - S) <= 1e-12 * A)
    # the mean over all origins of the B-row estimate is the full score
    B = 5
    mean = np.mean([R.score64(X, Xd, y, C, origin=o, B=B)[0] for o in range(N)], 0)
    assert np.all(np.abs(mean - S) <= 1e-10 * A)


def test_constructor_refusals():
    from dsvgd.targets import SoftmaxRegression as T
    _, Xd, y = R.problem(1, 12, 3, 4, seed=2)
    x, yt = torch.from_numpy(Xd), torch.from_numpy(y)
    assert T(x, yt).C == 3 and T(x, yt, classes=5).C == 5 and T(x, yt.float()).C == 3
    assert T(x, yt).y.dtype == torch.int32
    for bad in (yt.float() + 0.5, yt - 1, yt.float() * float("nan"), yt == 1):
        with pytest.raises(ValueError):
            T(x, bad)
    for classes in (2, 1, 17, 2.5):            # labels reach 2; C out of range; not integral
        with pytest.raises(ValueError):
            T(x, yt, classes=classes)
    with pytest.raises(ValueError):
        T(x, torch.zeros(12, dtype=torch.int64))            # max + 1 = 1 class
    with pytest.raises(ValueError):
        T(x, yt[:11])
    with pytest.raises(ValueError):
        T(torch.zeros(12, 0), yt)
    with pytest.raises(ValueError):
        T(torch.zeros(0, 4), yt[:0])
    with pytest.raises(ValueError):
        T(torch.zeros(12, 342), yt)                         # d = 1 + 3 * 342 = 1027
    assert T(torch.zeros(12, 341), yt).d == 1024
    assert T(torch.zeros(4, 63), torch.arange(4) * 5, classes=16).d == 1009
    for batch in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            T(x, yt, batch=batch)
    assert T(x, yt, batch=12).batch is None and T(x, yt, batch=5).batch == 5
    tgt = T(x, yt, batch=5)
    assert tgt.full.batch is None and tgt.full.x is tgt.x and T(x, yt).full.batch is None
    with pytest.raises(ValueError):
        tgt.logp(torch.zeros(tgt.d + 1))
    with pytest.raises(AssertionError):
        tgt.score(torch.zeros(2, tgt.d + 1), torch.zeros(2, tgt.d + 1))
    from dsvgd.engine import _gs_score_kind
    assert _gs_score_kind(T(x, yt)) is None


def test_fingerprint_follows_the_data_the_model_and_the_batch():
    _, Xd, y = R.problem(1, 20, 3, 4, seed=2)
    fp = _target(Xd, y).fingerprint()
    assert _target(Xd.copy(), y.copy()).fingerprint() == fp
    x2 = Xd.copy()
    x2[7, 1] = np.nextafter(x2[7, 1], np.float32(9))
    assert _target(x2, y).fingerprint() != fp
    y2 = y.copy()
    y2[3] = (y2[3] + 1) % 3
    assert _target(Xd, y2).fingerprint() != fp
    assert _target(Xd, y, classes=4).fingerprint() != fp
    assert _target(Xd, y, a0=2.0).fingerprint() != fp
    assert _target(Xd, y, b0=0.2).fingerprint() != fp
    assert _target(Xd, y, batch=5).fingerprint() != fp
    assert _target(Xd, y, batch=5).fingerprint() != _target(Xd, y, batch=6).fingerprint()
    assert _target(Xd, y, batch=20).fingerprint() == fp        # the whole data: no window


def test_sampler_without_gpu_raises_native_unavailable(monkeypatch):
    import dsvgd
    from dsvgd._native import NativeUnavailable
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    _, Xd, y = R.problem(1, 6, 3, 4, seed=2)
    tgt = _target(Xd, y)
    with pytest.raises(NativeUnavailable):
        dsvgd.Sampler(tgt.d, tgt, dsvgd.RBF(1.0)).sample(4, 1, 0.1, verbose=False)


NEW = ("dsvgd_score_softmax", "dsvgd_score_softmax_window", "dsvgd_softmax_predict",
       "dsvgd_softmax_predict_workspace_bytes")


def test_new_symbols_are_in_the_header_the_table_and_the_library_and_abi_stays_4():
    from dsvgd import _native
    header = open(os.path.join(ROOT, "include", "dsvgd.h")).read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    m = re.search(r"#define DSVGD_SOFTMAX_MAX_CLASSES (\d+)", header)
    from dsvgd.targets import SoftmaxRegression
    assert m and int(m.group(1)) == SoftmaxRegression.MAX_CLASSES >= 16
    assert _native.load().dsvgd_abi_version() == 4
    assert _native.load().dsvgd_softmax_small_rows() == R.SMALL_ROWS


def test_entry_points_validate_arguments_without_gpu():
    """Every call below fails a check: none reaches a launch."""
    from dsvgd import _native as N
    lib = N.load()
    buf = (ctypes.c_double * 64)()
    q = ctypes.addressof(buf)
    C, p = 3, 5
    d = R.dim(C, p)

    def full(X=q, ldx=d, n=2, dd=d, Xd=q, ldxd=p, y=q, N_=9, C_=C, p_=p, S=q, lds=d):
        return lib.dsvgd_score_softmax(X, ldx, n, dd, Xd, ldxd, y, N_, C_, p_, 1.0, 1.0, 1.0, S,
                                       lds, None)

    def win(cursor=q, B=4, **kw):
        a = dict(X=q, ldx=d, n=2, dd=d, Xd=q, ldxd=p, y=q, N_=9, C_=C, p_=p, S=q, lds=d)
        a.update(kw)
        return lib.dsvgd_score_softmax_window(a["X"], a["ldx"], a["n"], a["dd"], a["Xd"],
                                              a["ldxd"], a["y"], a["N_"], a["C_"], a["p_"], 1.0,
                                              1.0, 1.0, cursor, B, a["S"], a["lds"], None)

    def err():
        return lib.dsvgd_last_error()
    for name in ("X", "Xd", "y", "S"):
        assert full(**{name: None}) == -1 and b"null" in err()
        assert win(**{name: None}) == -1 and b"null" in err()
    assert win(cursor=None) == -1 and b"null" in err()
    for bad_c in (1, 0, 17):
        assert full(C_=bad_c, dd=R.dim(bad_c, p)) == -1 and b"MAX_CLASSES" in err()
    assert full(p_=0, dd=1) == -1 and b"p >= 1" in err()
    for bad_d in (d - 1, d + 1):
        assert full(dd=bad_d, ldx=d + 1, lds=d + 1) == -1 and b"1 + C p" in err()
    assert full(C_=3, p_=342, dd=1027, ldx=1027, lds=1027, ldxd=342) == -1 and b"1024" in err()
    for kw in (dict(n=0), dict(N_=0), dict(ldx=d - 1), dict(ldxd=p - 1), dict(lds=d - 1)):
        assert full(**kw) == -1 and b"sizes" in err()
        assert win(**kw) == -1
    for B in (0, 10, -1):
        assert win(B=B) == -1 and b"1 <= B <= N" in err()
    assert lib.dsvgd_softmax_predict_workspace_bytes(300, 7, C) == 7 * 2 * C * 4
    assert lib.dsvgd_softmax_predict_workspace_bytes(10 ** 6, 7, C) == 7 * 64 * C * 4

    def pred(X=q, Xt=q, P=q, ws=q, dd=d, ldp=C, ldxt=p, n=2, Nt=9):
        return lib.dsvgd_softmax_predict(X, d, n, dd, Xt, ldxt, Nt, C, p, P, ldp, ws, None)
    for name in ("X", "Xt", "P", "ws"):
        assert pred(**{name: None}) == -1 and b"null" in err()
    assert pred(dd=d + 1) == -1 and b"1 + C p" in err()
    for kw in (dict(ldp=C - 1), dict(ldxt=p - 1), dict(n=0), dict(Nt=0)):
        assert pred(**kw) == -1 and b"sizes" in err()


@functools.lru_cache(maxsize=None)
def case(i, **kw):
    """Problem i of R.SHAPES (seed 200 + i) and its fp64 score; shared with
    tests/test_gpu_softmax.py, computed once and left unchanged."""
    n, N, C, p = R.SHAPES[i]
    prob = R.problem(n, N, C, p, 200 + i, **kw)
    S, A = R.score64(*prob, C)
    for a in prob + (S, A):
        a.setflags(write=False)
    return prob, S, A


@pytest.mark.parametrize("i", range(len(R.SHAPES)), ids=lambda i: "n%d-N%d-C%d-p%d" % R.SHAPES[i])
def test_fp32_restatement_stays_under_a_tenth_of_the_gpu_bound(i):
    C = R.SHAPES[i][2]
    (X, Xd, y), S, A = case(i)
    X, S, A = X[:48], S[:48], A[:48]          # the particles are independent: 48 of them do
    got = R.score32(X, Xd, y, C)
    worst = float((np.abs(got.astype(np.float64) - S) / A).max())
    print("worst err/A %.3g" % worst)
    assert worst <= 0.1 * R.SCORE_TOL


def experiment():
    import importlib.util

    from conftest import PKG
    spec = importlib.util.spec_from_file_location(
        "dsvgd_softmax_experiment", os.path.join(PKG, "experiments", "softmax.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_experiment_dataset_is_seeded_and_split():
    E = experiment()
    xtr, ytr, xte, yte = E.synthetic_classes(1000, 8, 4, seed=0)
    assert xtr.shape == (900, 8) and ytr.shape == (900,) and xte.shape == (100, 8)
    assert xtr.dtype == np.float32 and ytr.dtype == np.int64
    assert (xtr[:, -1] == 1).all() and set(np.unique(ytr)) == {0, 1, 2, 3}
    again = E.synthetic_classes(1000, 8, 4, seed=0)
    assert all(np.array_equal(a, b) for a, b in zip((xtr, ytr, xte, yte), again))
    assert not np.array_equal(E.synthetic_classes(1000, 8, 4, seed=1)[0], xtr)
    from click.testing import CliRunner
    res = CliRunner().invoke(E.cli, ['--help'])
    assert res.exit_code == 0
    for opt in ('--classes', '--p', '--nparticles', '--niter', '--stepsize', '--order', '--kernel',
                '--batch', '--adagrad', '--every'):
        assert opt in res.output
