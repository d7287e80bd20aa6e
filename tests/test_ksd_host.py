"""CPU-only tests of the KSD diagnostic: the fp64 reference the GPU tests use
(tests/ksd_reference.py) against second-order autograd, the new C ABI entry
points' exports and argument validation, and the public interface's refusals
without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from ksd_reference import ksd_reference, stein_matrix


def test_reference_matches_second_order_autograd():
    """u(x, y) = s(x).s(y) k + s(x).grad_y k + s(y).grad_x k + tr(grad_x grad_y k)
    by torch.autograd on the reference-style kernel and a Gaussian logp."""
    n, d, h = 6, 3, 1.7
    g = torch.Generator().manual_seed(5)
    X = torch.randn(n, d, generator=g, dtype=torch.float64)
    mu = torch.randn(d, generator=g, dtype=torch.float64)
    lam = torch.rand(d, generator=g, dtype=torch.float64) + 0.5
    kernel = lambda x, y: torch.exp(-((x - y) ** 2).sum() / h)   # noqa: E731
    logp = lambda x: -0.5 * (lam * (x - mu) ** 2).sum()          # noqa: E731

    def score(x):
        x = x.detach().clone().requires_grad_(True)
        return torch.autograd.grad(logp(x), x)[0]

    S = torch.stack([score(X[i]) for i in range(n)])
    U = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            x = X[i].detach().clone().requires_grad_(True)
            y = X[j].detach().clone().requires_grad_(True)
            k = kernel(x, y)
            gx, gy = torch.autograd.grad(k, (x, y), create_graph=True)
            tr = sum(torch.autograd.grad(gx[c], y, retain_graph=True)[0][c] for c in range(d))
            U[i, j] = float(S[i] @ S[j] * k + S[i] @ gy + S[j] @ gx + tr)
    Uref, _ = stein_matrix(X.numpy(), S.numpy(), h)
    assert np.abs(Uref - U).max() <= 1e-12 * max(1.0, np.abs(U).max())
    ref = ksd_reference(X.numpy(), S.numpy(), h)
    assert abs(ref["V"] - U.sum() / n ** 2) <= 1e-12 * abs(ref["V"])
    off = U.sum() - np.trace(U)
    assert abs(ref["U"] - off / (n * (n - 1))) <= 1e-12 * max(1.0, abs(ref["U"]))
    assert np.abs(ref["t"] - (U.sum(1) - np.diag(U))).max() <= 1e-12 * np.abs(U).sum(1).max()


def test_library_exports_ksd_entry_points():
    from dsvgd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("dsvgd_ksd_rows", "dsvgd_ksd_finish", "dsvgd_ksd_direct", "dsvgd_ksd_parts"):
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES


def test_ksd_parts_and_workspace_sizes():
    lib = __import__("dsvgd")._native.load()
    # full layout: enough column slices for ~2048 workgroups, >= 128 columns each
    assert lib.dsvgd_ksd_parts(300, 300, 0) == 3
    assert lib.dsvgd_ksd_parts(65536, 65536, 0) == 4
    assert lib.dsvgd_ksd_parts(100, 100, 0) == 1
    # symmetric layout: the row slices plus one column-sum slot per tile row
    assert lib.dsvgd_ksd_parts(384, 384, 1) == 3 + 3
    assert lib.dsvgd_ksd_parts(65536, 65536, 1) == 4 + 512
    assert lib.dsvgd_ksd_workspace_doubles(65) == 4


def test_ksd_calls_validate_arguments_without_gpu():
    lib = __import__("dsvgd")._native.load()
    rc = lib.dsvgd_ksd_rows(None, 128, None, 128, 32, 3, 0, 4, 4, None, 0, 1, None, None, None)
    assert rc == -1 and b"null" in lib.dsvgd_last_error()
    rc = lib.dsvgd_ksd_finish(None, 128, None, 1, None, 128, 32, 3, 0, 4, 4, None, 0, 1, None,
                              None, None, None, None)
    assert rc == -1 and b"null" in lib.dsvgd_last_error()
    rc = lib.dsvgd_ksd_direct(None, 128, 32, 1, 0, 4, 4, None, None, None, None, None)
    assert rc == -1 and b"null" in lib.dsvgd_last_error()
    rc = lib.dsvgd_ksd_gate(None, 1, 4, 4, None, None)
    assert rc == -1 and b"null" in lib.dsvgd_last_error()
    # mis-sized / misaligned arguments are refused before any launch too
    # (every call below fails a check: none reaches a launch)
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    rc = lib.dsvgd_ksd_rows(p, 256, p, 128, 32, 3, 0, 4, 4, p, 0, 1, p, p, None)
    assert rc == -1 and b"ldd" in lib.dsvgd_last_error()
    rc = lib.dsvgd_ksd_rows(p + 4, 128, p, 128, 32, 3, 0, 4, 4, p, 0, 1, p, p, None)
    assert rc == -1 and b"aligned" in lib.dsvgd_last_error()
    rc = lib.dsvgd_ksd_rows(p, 128, p, 128, 32, 3, 1, 3, 4, p, 1, 2, p, p, None)
    assert rc == -1 and b"sym" in lib.dsvgd_last_error()
    rc = lib.dsvgd_ksd_finish(p, 128, p, 1, p, 128, 32, 3, 0, 4, 4, p, 0, 7, p, p, p, p, None)
    assert rc == -1 and b"parts" in lib.dsvgd_last_error()
    rc = lib.dsvgd_ksd_direct(p, 256, 128, 65, 0, 4, 4, p, p, p, p, None)
    assert rc == -1 and b"64" in lib.dsvgd_last_error()


def test_public_interface_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import dsvgd
    from dsvgd import metrics
    from dsvgd._native import NativeUnavailable
    tgt = dsvgd.targets.Gaussian([0, 0, 0], [1, 1, 1])
    with pytest.raises(NativeUnavailable):
        metrics.ksd(torch.zeros(8, 3), tgt)
    with pytest.raises(NativeUnavailable):
        metrics.ksd(np.zeros((8, 3), np.float32), np.zeros((8, 3), np.float32), dsvgd.RBF(1.0))


@pytest.mark.parametrize("bad", [0, -1, -5, 1.5])
def test_sampler_rejects_bad_ksd_every_before_touching_the_device(bad):
    import dsvgd
    s = dsvgd.Sampler(3, dsvgd.targets.Gaussian([0, 0, 0], [1, 1, 1]), dsvgd.RBF("median"))
    with pytest.raises(ValueError):
        s.sample(8, 2, 0.1, order="jacobi", verbose=False, ksd_every=bad)
    assert s.diagnostics is None
