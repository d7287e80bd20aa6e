"""CPU-only tests of the inverse multiquadric (IMQ) kernel: the `IMQ` class and
the kernel probe, the fp64 reference the GPU tests use (tests/imq_reference.py)
against the reference-run fixtures (tests/golden/imq_*.npz) and second-order
autograd, and the new C ABI entry points' exports and argument validation."""
import ctypes

import numpy as np
import pytest
import torch

from imq_reference import ksd_reference, phi64, sequential64, stein_matrix
from oracle import svgd_oracle as O

# The fixtures are the reference's own fp32 results (autograd scores and kernel
# gradients, n <= 60 fp32 terms summed per coordinate: ~n 2^-24 = 4e-6 of the
# summed magnitudes at worst), so the fp64 restatement is held to the
# project's phi and trajectory bounds (tests/test_gpu_parity.py).
PHI_TOL = 1e-5
TRAJ_TOL = 1e-4


def _score_fn(g):
    tgt = str(g["target"])
    if tgt == "gmm":
        return O.score_gmm
    if tgt == "gaussian":
        return lambda X: O.score_gaussian(X, g["mu"], g["lam"])
    return lambda X: O.score_logreg(X, g["x_train"], g["t_train"])


# ------------------------------------------------------------- the class --
def test_imq_validation_and_call():
    import dsvgd
    from dsvgd.kernels import IMQ
    assert dsvgd.IMQ is IMQ and "IMQ" in dsvgd.__all__
    k = IMQ()
    assert k.h == 1.0 and k.beta == -0.5 and not k.median
    assert IMQ("median").median and IMQ("median", -1).beta == -1.0
    assert repr(IMQ(1.7, -0.75)) == "IMQ(h=1.7, beta=-0.75)"
    assert repr(IMQ("median")) == "IMQ(h='median', beta=-0.5)"
    for bad_h in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            IMQ(bad_h)
    for bad_beta in (0.0, 0.5, -1.0001, -2.0, float("nan")):
        with pytest.raises(ValueError):
            IMQ(1.0, bad_beta)
    x, y = torch.tensor([0.3, -1.0, 2.0]), torch.tensor([1.0, 0.5, 0.25])
    want = (1.0 + float(((x - y) ** 2).sum()) / 1.7) ** -0.75
    assert float(IMQ(1.7, -0.75)(x, y)) == pytest.approx(want, rel=1e-6)
    assert float(IMQ(2.0)(x, x)) == 1.0
    with pytest.raises(ValueError):
        IMQ("median")(x, y)


# ------------------------------------------------------------- the probe --
def test_probe_resolves_imq_lambdas():
    from dsvgd.kernels import IMQ, RBF, resolve_kernel
    k = IMQ(2.5, -0.25)
    assert resolve_kernel(k, 3) is k
    for h, beta in ((1.0, -0.5), (1.7, -0.5), (3.3, -0.75), (0.4, -1.0), (12.5, -0.37)):
        for d in (1, 3, 50):
            r = resolve_kernel(lambda x, y: (1. + torch.dist(x, y, p=2) ** 2 / h) ** beta, d)
            assert isinstance(r, IMQ)
            assert r.h == pytest.approx(h, rel=1e-4) and r.beta == pytest.approx(beta, abs=1e-4)
    # the most likely spellings come back exactly
    r = resolve_kernel(lambda x, y: (1 + torch.dist(x, y) ** 2) ** -0.5, 4)
    assert (r.h, r.beta) == (1.0, -0.5)
    # an IMQ instance's own __call__ is an IMQ-shaped callable
    r = resolve_kernel(IMQ(1.7, -0.75).__call__, 5)
    assert (r.h, r.beta) == (1.7, -0.75)
    # RBF callables are probed as RBF first, exactly as before
    r = resolve_kernel(lambda x, y: torch.exp(-torch.dist(x, y) ** 2 / 3.7), 5)
    assert isinstance(r, RBF) and r.h == pytest.approx(3.7, rel=1e-5)
    assert resolve_kernel(None, 3).h == 1.0


@pytest.mark.parametrize("kernel", [
    lambda x, y: torch.exp(-torch.dist(x, y)),                 # Laplace (tests/test_host.py)
    lambda x, y: (x * y).sum(),                                # linear (tests/test_host.py)
    lambda x, y: (1 + torch.dist(x, y) ** 2) ** -2.0,          # beta outside [-1, 0)
    lambda x, y: (1 + torch.dist(x, y)) ** -0.5,               # not a function of |x - y|^2 / h + 1
    lambda x, y: 1.0 / (1 + torch.dist(x, y) ** 4),
], ids=["laplace", "linear", "beta-2", "imq-of-distance", "quartic"])
def test_probe_still_refuses_other_kernels(kernel):
    from dsvgd.kernels import resolve_kernel
    with pytest.raises(ValueError) as e:
        resolve_kernel(kernel, 3)
    msg = str(e.value)
    assert "RBF" in msg and "IMQ" in msg and "inverse multiquadric" in msg


def test_engine_and_distsampler_refusals_need_no_gpu():
    import dsvgd
    with pytest.raises(ValueError, match="RBF-only"):
        dsvgd.DistSampler(0, 1, dsvgd.targets.Gaussian([0, 0], [1, 1]), dsvgd.IMQ(1.0),
                          torch.zeros(8, 2), 1, 1, False, False, False)
    with pytest.raises(ValueError, match="RBF-only"):
        dsvgd.DistSampler(0, 1, dsvgd.targets.Gaussian([0, 0], [1, 1]),
                          lambda x, y: (1 + torch.dist(x, y) ** 2) ** -0.5,
                          torch.zeros(8, 2), 1, 1, False, False, False)
    with pytest.raises(ValueError, match="pair_split"):
        dsvgd.PhiEngine(2048, 256, m=1024, row0=0, pair_split=(0, 2), kernel=dsvgd.IMQ())
    with pytest.raises(ValueError):
        dsvgd.PhiEngine(8, 3, kernel=lambda x, y: x)     # callables are resolved by the samplers
    s = dsvgd.Sampler(3, dsvgd.targets.Gaussian([0, 0, 0], [1, 1, 1]),
                      lambda x, y: (1 + torch.dist(x, y) ** 2 / 1.7) ** -0.75)
    assert repr(s._rbf) == "IMQ(h=1.7, beta=-0.75)"


# -------------------------------------------------- the fp64 restatement --
@pytest.mark.parametrize("name", ["imq_gauss_n48_d5_h1p7", "imq_gmm_n40", "imq_logreg_n60"])
def test_reference_phi_matches_reference_run(golden, name):
    g = golden(name)
    X = g["X"]
    phi = phi64(X, _score_fn(g)(X), float(g["h"]), float(g["beta"]))
    err = np.abs(phi - g["phi"]).max() / np.abs(g["phi"]).max()
    print("%s: max-normalised error %.3g" % (name, err))
    assert err < PHI_TOL


def test_reference_sequential_matches_reference_run(golden):
    g = golden("imq_sample_gauss_n16_d3")
    assert g["values"].shape == (4, 16, 3)
    traj = sequential64(g["values"][0], _score_fn(g), float(g["h"]), float(g["beta"]),
                        int(g["T"]), float(g["eps"]))
    assert np.abs(traj - g["values"]).max() < TRAJ_TOL
    assert np.abs(traj[-1] - traj[0]).max() > 100 * TRAJ_TOL     # the particles did move


@pytest.mark.parametrize("beta", [-0.5, -1.0, -0.25])
def test_stein_matrix_matches_second_order_autograd(beta):
    """u(x, y) = s(x).s(y) k + s(x).grad_y k + s(y).grad_x k + tr(grad_x grad_y k)
    by torch.autograd on the reference-style IMQ lambda and a Gaussian logp."""
    n, d, h = 5, 3, 1.7
    gen = torch.Generator().manual_seed(5)
    X = torch.randn(n, d, generator=gen, dtype=torch.float64)
    mu = torch.randn(d, generator=gen, dtype=torch.float64)
    lam = torch.rand(d, generator=gen, dtype=torch.float64) + 0.5
    kernel = lambda x, y: (1.0 + ((x - y) ** 2).sum() / h) ** beta   # noqa: E731
    S = -lam * (X - mu)
    U = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            x = X[i].detach().clone().requires_grad_(True)
            y = X[j].detach().clone().requires_grad_(True)
            k = kernel(x, y)
            gx, gy = torch.autograd.grad(k, (x, y), create_graph=True)
            tr = sum(torch.autograd.grad(gx[c], y, retain_graph=True)[0][c] for c in range(d))
            U[i, j] = float(S[i] @ S[j] * k + S[i] @ gy + S[j] @ gx + tr)
    Uref, A = stein_matrix(X.numpy(), S.numpy(), h, beta)
    assert np.abs(Uref - U).max() <= 1e-12 * max(1.0, np.abs(U).max())
    assert (A >= np.abs(Uref) - 1e-12).all()          # A bounds the terms' magnitudes
    ref = ksd_reference(X.numpy(), S.numpy(), h, beta)
    assert abs(ref["V"] - U.sum() / n ** 2) <= 1e-12 * abs(ref["V"])
    off = U.sum() - np.trace(U)
    assert abs(ref["U"] - off / (n * (n - 1))) <= 1e-12 * max(1.0, abs(ref["U"]))
    assert np.abs(ref["t"] - (U.sum(1) - np.diag(U))).max() <= 1e-12 * np.abs(U).sum(1).max()
    c1 = -2.0 * beta / h
    assert np.allclose(ref["udiag"], (S.numpy() ** 2).sum(1) + c1 * d, rtol=1e-14)


# ------------------------------------------------------------- the C ABI --
NEW_ENTRY_POINTS = ("dsvgd_phi_mm_kern", "dsvgd_phi_mm_x3_kern", "dsvgd_phi_mm_h2_kern",
                    "dsvgd_phi_finish_imq", "dsvgd_phi_direct_kern", "dsvgd_phi_row_kern",
                    "dsvgd_phi_row_split_kern", "dsvgd_ksd_rows_kern", "dsvgd_ksd_finish_imq",
                    "dsvgd_ksd_direct_kern")


def test_library_exports_kernel_entry_points_and_abi_stays_4():
    from dsvgd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES
    assert _native.load().dsvgd_abi_version() == 4
    assert ctypes.sizeof(_native.Kernel) == 8


def _twin_cases(p):
    """(plain name, _kern name, what the _kern call takes after the shared
    arguments, failing argument sets without the trailing stream) of the eight
    operations that exist under two names: null pointers, a wrong ldd where
    there is one, and a bad sym or size (the sets of the test below and of
    tests/test_ksd_host.py).  p: a 16-byte aligned address."""
    mm = [(None, 128, None, 128, 0, 4, 4, None, 1, None, 128, None),
          (p, 256, p, 128, 0, 4, 4, p, 1, p, 128, p),            # ldd
          (p, 128, p, 128, 0, 0, 4, p, 1, p, 128, p),            # sizes
          (p, 128, p, 128, 2, 4, 4, p, 1, p, 128, p)]            # the row block
    return [
        ("dsvgd_phi_mm", "dsvgd_phi_mm_kern", "gate order", mm),
        ("dsvgd_phi_mm_gated", "dsvgd_phi_mm_kern", "order",
         [a + (None,) for a in mm[:1]] + [a + (p,) for a in mm[1:]]),
        ("dsvgd_phi_mm_x3", "dsvgd_phi_mm_x3_kern", "order",
         [(None, 128, None, 128, 0, 4, 4, None, 1, None, 128, None, 0, 0, None),
          (p, 256, p, 128, 0, 4, 4, p, 1, p, 128, p, 0, 0, None),
          (p, 128, p, 128, 0, 3, 4, p, 1, p, 128, p, 1, 0, None)]),          # sym, m < n
        ("dsvgd_phi_mm_h2", "dsvgd_phi_mm_h2_kern", "order",
         [(None, 128, None, 128, 0, 4, 4, None, 1, None, 128, None, 0, None, None),
          (p, 256, p, 128, 0, 4, 4, p, 1, p, 128, p, 0, p, None),
          (p, 128, p, 128, 0, 4, 4, p, 1, p, 128, p, 1, p, None)]),          # sym, ldy % 256
        ("dsvgd_phi_direct", "dsvgd_phi_direct_kern", "",
         [(None, 128, None, 128, 0, 4, 4, 1, None, 0.25, 0.0, None, 1, None, 1, None, 1, None, 0),
          (p, 256, p, 128, 0, 4, 4, 1, p, 0.25, 0.0, None, 1, None, 1, None, 1, None, 0),
          (p, 128, p, 256, 0, 4, 4, 65, p, 0.25, 0.0, None, 1, None, 1, None, 1, None, 0)]),
        ("dsvgd_phi_row", "dsvgd_phi_row_kern", "",
         [(None, 4, None, 4, 4, 3, 0, None, 0.1, None, None),
          (p, 4, p, 4, 4, 3, 7, p, 0.1, None, None),                         # i >= n
          (p, 8000, p, 8000, 4, 7950, 0, p, 0.1, None, None)]),              # d > 7936
        ("dsvgd_phi_row_split", "dsvgd_phi_row_split_kern", "",
         [(None, 4, None, 4, 4, 3, 0, None, 0.1, None, None, None, 2),
          (p, 4, p, 4, 4, 3, 0, p, 0.1, None, None, p, 0),                   # blocks
          (p, 5000, p, 5000, 4, 4100, 0, p, 0.1, None, None, p, 2)]),        # d > 4096
        ("dsvgd_ksd_rows", "dsvgd_ksd_rows_kern", "",
         [(None, 128, None, 128, 32, 3, 0, 4, 4, None, 0, 1, None, None),
          (p, 256, p, 128, 32, 3, 0, 4, 4, p, 0, 1, p, p),
          (p, 128, p, 128, 32, 3, 1, 3, 4, p, 1, 2, p, p)]),                 # sym, row0 > 0
        ("dsvgd_ksd_direct", "dsvgd_ksd_direct_kern", "",
         [(None, 128, 32, 1, 0, 4, 4, None, None, None, None),
          (p, 256, 128, 3, 2, 4, 4, p, p, p, p),                             # the row block
          (p, 256, 128, 65, 0, 4, 4, p, p, p, p)]),                          # d > 64
    ]


def test_plain_and_kern_names_are_one_body():
    """Each operation's plain name and its _kern name with an RBF description
    refuse the same invalid arguments with the same code and the same text;
    none of the calls reaches a launch."""
    from dsvgd import _native as N
    lib = N.load()
    rbf = N.Kernel(N.KERNEL_RBF, 0.0)
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    for plain, kern, extra, cases in _twin_cases(p):
        for args in cases:
            got = []
            tail = (None,) if "gate" in extra else ()
            tail += (rbf, 0) if "order" in extra else (rbf,)
            for name, a in ((plain, args), (kern, args + tail)):
                rc = getattr(lib, name)(*a, None)
                got.append((rc, lib.dsvgd_last_error()))
            assert got[0][0] == -1 and got[0][1], (plain, args, got)
            assert got[0] == got[1], (plain, args, got)


def test_kernel_calls_validate_arguments_without_gpu():
    """Every call below fails a check: none reaches a launch."""
    from dsvgd import _native as N
    lib = N.load()
    imq, rbf = N.Kernel(N.KERNEL_IMQ, -0.5), N.Kernel(N.KERNEL_RBF, 0.0)

    def err():
        return lib.dsvgd_last_error()
    # the kernel description itself
    for bad in (N.Kernel(N.KERNEL_IMQ, 0.0), N.Kernel(N.KERNEL_IMQ, -1.5), N.Kernel(7, -0.5)):
        rc = lib.dsvgd_phi_mm_kern(None, 128, None, 128, 0, 4, 4, None, 1, None, 128, None, None,
                                   bad, 0, None)
        assert rc == -1 and b"kern" in err()
        rc = lib.dsvgd_ksd_direct_kern(None, 128, 32, 1, 0, 4, 4, None, None, None, None, bad, None)
        assert rc == -1 and b"kern" in err()
    # order 1 is the IMQ's gradient matrix only; order 2 does not exist
    rc = lib.dsvgd_phi_mm_h2_kern(None, 128, None, 128, 0, 4, 4, None, 1, None, 128, None, 0, None,
                                  None, rbf, 1, None)
    assert rc == -1 and b"order" in err()
    rc = lib.dsvgd_phi_mm_x3_kern(None, 128, None, 128, 0, 4, 4, None, 1, None, 128, None, 0, 0,
                                  None, imq, 2, None)
    assert rc == -1 and b"order" in err()
    # null pointers, in both families (one body serves both)
    for kern in (imq, rbf):
        rc = lib.dsvgd_phi_mm_kern(None, 128, None, 128, 0, 4, 4, None, 1, None, 128, None, None,
                                   kern, 0, None)
        assert rc == -1 and b"null" in err()
        rc = lib.dsvgd_phi_mm_x3_kern(None, 128, None, 128, 0, 4, 4, None, 1, None, 128, None, 0,
                                      0, None, kern, 0, None)
        assert rc == -1 and b"null" in err()
        rc = lib.dsvgd_phi_mm_h2_kern(None, 128, None, 128, 0, 4, 4, None, 1, None, 128, None, 0,
                                      None, None, kern, 0, None)
        assert rc == -1 and b"null" in err()
        rc = lib.dsvgd_phi_direct_kern(None, 128, None, 128, 0, 4, 4, 1, None, 0.25, 0.0, None, 1,
                                       None, 1, None, 1, None, 0, kern, None)
        assert rc == -1 and b"null" in err()
        rc = lib.dsvgd_phi_row_kern(None, 4, None, 4, 4, 3, 0, None, 0.1, None, None, kern, None)
        assert rc == -1 and b"null" in err()
        rc = lib.dsvgd_phi_row_split_kern(None, 4, None, 4, 4, 3, 0, None, 0.1, None, None, None,
                                          2, kern, None)
        assert rc == -1 and b"null" in err()
        rc = lib.dsvgd_ksd_rows_kern(None, 128, None, 128, 32, 3, 0, 4, 4, None, 0, 1, None, None,
                                     kern, None)
        assert rc == -1 and b"null" in err()
        rc = lib.dsvgd_ksd_direct_kern(None, 128, 32, 1, 0, 4, 4, None, None, None, None, kern,
                                       None)
        assert rc == -1 and b"null" in err()
    # the two IMQ finishes take the IMQ family only
    rc = lib.dsvgd_phi_finish_imq(None, 128, None, 128, None, 1, None, 128, 0, 4, 3, 32, None, imq,
                                  0.25, 0.0, None, 3, None, 3, None, 3, None)
    assert rc == -1 and b"null" in err()
    rc = lib.dsvgd_ksd_finish_imq(None, 128, None, 128, None, 1, None, 128, 32, 3, 0, 4, 4, None,
                                  imq, 0, 1, None, None, None, None, None)
    assert rc == -1 and b"null" in err()
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    rc = lib.dsvgd_phi_finish_imq(p, 128, p, 128, p, 1, p, 128, 0, 4, 3, 32, p, rbf, 0.25, 0.0,
                                  None, 3, None, 3, None, 3, None)
    assert rc == -1 and b"IMQ" in err()
    rc = lib.dsvgd_ksd_finish_imq(p, 128, p, 128, p, 1, p, 128, 32, 3, 0, 4, 4, p, rbf, 0, 1, p, p,
                                  p, p, None)
    assert rc == -1 and b"IMQ" in err()
    # sizes are checked as in the calls beside them
    rc = lib.dsvgd_phi_mm_kern(p, 256, p, 128, 0, 4, 4, p, 1, p, 128, p, None, imq, 0, None)
    assert rc == -1 and b"ldd" in err()
    rc = lib.dsvgd_phi_mm_h2_kern(p, 128, p, 128, 0, 4, 4, p, 1, p, 128, p, 1, p, None, imq, 1, None)
    assert rc == -1 and b"sym" in err()
    rc = lib.dsvgd_phi_row_kern(p, 8000, p, 8000, 4, 7900, 0, p, 0.1, None, None, imq, None)
    assert rc == -1 and b"7808" in err()
    rc = lib.dsvgd_ksd_direct_kern(p, 256, 128, 65, 0, 4, 4, p, p, p, p, imq, None)
    assert rc == -1 and b"64" in err()
