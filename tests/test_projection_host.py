"""Host-side checks of projected SVGD (no GPU): the two invariants of the fp64
reference tests/projection_reference.py (full rank = plain SVGD; the orthogonal
complement does not move), its basis rule, the arguments of dsvgd.Projection,
the combinations Sampler.sample(project=...) refuses before any GPU work, and
the new entry points with their argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import projection_reference as P
from oracle import svgd_oracle as O


def _problem(n, d, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, d)
    mu, lam = rs.randn(d), rs.uniform(0.5, 2.0, d)
    return X, O.score_gaussian(X, mu, lam), rs


def _orthonormal(rs, d, r):
    return np.linalg.qr(rs.randn(d, r))[0]


# ------------------------------------------------------- the reference --
def test_rbf_phi64_is_the_oracle_phi():
    X, S, _ = _problem(40, 5)
    ref = O.phi(X, S, 2.5)
    assert np.abs(P.rbf_phi64(X, S, 2.5) - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("beta,h", [(None, 7.0), (None, None), (-0.5, None), (-0.75, 3.0)])
def test_full_rank_is_the_plain_step(beta, h):
    """r = d and any orthonormal Psi: the radial kernels do not see the
    rotation (the median bandwidth included)."""
    n, d, eps = 60, 9, 0.1
    X, S, rs = _problem(n, d, 1)
    Psi = _orthonormal(rs, d, d)
    got = P.step64(X, S, Psi, eps, h, beta)
    hh = P.median_h64(X) if h is None else h
    ref = X + eps * P.phi64(X, S, hh, beta)
    assert np.abs(ref - X).max() > 1e-3
    assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max()


def test_the_complement_does_not_move():
    n, d, r = 50, 12, 3
    X, S, rs = _problem(n, d, 2)
    Q = _orthonormal(rs, d, d)
    Psi, rest = Q[:, :r], Q[:, r:]
    mu, lam = rs.randn(d), rs.uniform(0.5, 2.0, d)
    traj = P.jacobi64(X, lambda Y, l: O.score_gaussian(Y, mu, lam), Psi, 5, 0.2)
    move = traj[-1] - traj[0]
    assert np.abs(move).max() > 1e-2
    assert np.abs(move @ rest).max() <= 1e-13 * np.abs(move).max()
    assert np.abs(move - move @ Psi @ Psi.T).max() <= 1e-13 * np.abs(move).max()


def test_basis64_orders_signs_and_diagonalises():
    rs = np.random.RandomState(3)
    G = rs.randn(30, 7) * np.array([5, 4, 3, 1, 0.5, 0.1, 0.01])
    H, A = P.gram64(np.zeros_like(G), G, False)
    assert np.all(A >= np.abs(H) - 1e-15) and np.allclose(np.diag(A), np.diag(H))
    H2, _ = P.gram64(G, G, True)
    assert np.allclose(H2, 4 * H)
    Psi, lam = P.basis64(H, 3)
    assert np.all(np.diff(lam) <= 0) and lam.shape == (7,)
    assert np.abs(Psi.T @ Psi - np.eye(3)).max() < 1e-12
    assert np.abs(H @ Psi - Psi * lam[:3]).max() < 1e-10 * lam[0]
    top = np.abs(Psi).argmax(0)
    assert np.all(Psi[top, np.arange(3)] > 0)
    # the implementation's rule is the same one
    from dsvgd.projection import leading_basis
    Pt, lt = leading_basis(torch.from_numpy(H.astype(np.float32)), 3)
    H32 = H.astype(np.float32).astype(np.float64)
    Pr, lr = P.basis64(H32, 3)
    assert np.abs(lt.numpy() - lr).max() <= 1e-12 * lr[0]
    assert np.abs(Pt.numpy() - Pr).max() <= 1e-9
    assert Pt.dtype == torch.float64 and lt.dtype == torch.float64


def test_learned_basis_refreshes_on_schedule():
    calls = []
    b = P.learned(2, every=3)
    X, S, _ = _problem(20, 5, 4)
    for l in range(7):
        calls.append(b(l, X + l, S))
    assert calls[0] is calls[1] is calls[2] and calls[3] is calls[4] and calls[3] is not calls[0]
    once = P.learned(2, every=None)
    assert once(0, X, S) is once(5, X + 1, S)


# ------------------------------------------------------- the arguments --
def test_projection_validates_its_arguments():
    import dsvgd
    assert "Projection" in dsvgd.__all__
    p = dsvgd.Projection(rank=4)
    assert (p.rank, p.every, p.reference) == (4, 10, "normal")
    assert p.basis is None and p.eigenvalues is None and p.captured is None and p.refreshes == 0
    assert dsvgd.Projection(rank=2, every=None, reference=None).every is None
    with pytest.raises(ValueError, match="exactly one"):
        dsvgd.Projection()
    with pytest.raises(ValueError, match="exactly one"):
        dsvgd.Projection(rank=2, basis=np.eye(3)[:, :2])
    for rank in (0, -1, 2.5, True, 257):
        with pytest.raises(ValueError):
            dsvgd.Projection(rank=rank)
    for every in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="every"):
            dsvgd.Projection(rank=2, every=every)
    with pytest.raises(ValueError, match="reference"):
        dsvgd.Projection(rank=2, reference="uniform")
    # the schedule
    assert [l for l in range(7) if dsvgd.Projection(rank=2, every=3).due(l)] == [0, 3, 6]
    assert [l for l in range(7) if dsvgd.Projection(rank=2, every=None).due(l)] == [0]


def test_projection_checks_a_basis_once_in_fp64():
    import dsvgd
    rs = np.random.RandomState(5)
    Q = _orthonormal(rs, 8, 3)
    for B in (Q, Q.astype(np.float32), torch.from_numpy(Q)):
        p = dsvgd.Projection(basis=B, every=7)
        assert p.rank == 3 and p.every is None
        assert not any(p.due(l) for l in range(20))
    bad = Q.copy()
    bad[:, 0] *= 1.0 + 1e-5           # |Psi^T Psi - I| = 2e-5
    with pytest.raises(ValueError, match="orthonormal"):
        dsvgd.Projection(basis=bad)
    ok = Q.copy()
    ok[:, 0] *= 1.0 + 2e-7
    dsvgd.Projection(basis=ok)
    skew = Q.copy()
    skew[:, 1] += 1e-4 * Q[:, 0]
    with pytest.raises(ValueError, match="orthonormal"):
        dsvgd.Projection(basis=skew)
    for shape in ((8,), (3, 8), (8, 0)):
        with pytest.raises(ValueError, match="basis"):
            dsvgd.Projection(basis=np.zeros(shape))
    nan = Q.copy()
    nan[0, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        dsvgd.Projection(basis=nan)


def test_sampler_refusals_come_before_any_gpu_work():
    """Every call raises ValueError on a machine without a device (the GPU is
    first touched after the checks: anything else would raise
    NativeUnavailable here, or draw particles)."""
    import dsvgd
    d = 6
    s = dsvgd.Sampler(d, dsvgd.targets.Gaussian(np.zeros(d), np.ones(d)), dsvgd.RBF(1.0))
    proj = dsvgd.Projection(rank=2)
    state = torch.random.get_rng_state()
    with pytest.raises(ValueError, match="jacobi"):
        s.sample(8, 1, 0.1, project=proj, verbose=False)               # (the default order)
    with pytest.raises(ValueError, match="jacobi"):
        s.sample(8, 1, 0.1, order="sequential", project=proj, verbose=False)
    with pytest.raises(ValueError, match="adagrad"):
        s.sample(8, 1, 0.1, order="jacobi", adagrad=True, project=proj, verbose=False)
    with pytest.raises(ValueError, match="dsvgd.Projection"):
        s.sample(8, 1, 0.1, order="jacobi", project=2, verbose=False)
    with pytest.raises(ValueError, match="rank 7 exceeds d = 6"):
        s.sample(8, 1, 0.1, order="jacobi", project=dsvgd.Projection(rank=7), verbose=False)
    with pytest.raises(ValueError, match="5 rows"):
        s.sample(8, 1, 0.1, order="jacobi", project=dsvgd.Projection(basis=np.eye(5)[:, :2]),
                 verbose=False)
    wide = dsvgd.Sampler(1025, dsvgd.targets.Gaussian(np.zeros(1025), np.ones(1025)),
                         dsvgd.RBF(1.0))
    with pytest.raises(ValueError, match="1024"):
        wide.sample(8, 1, 0.1, order="jacobi", project=proj, verbose=False)
    assert torch.equal(torch.random.get_rng_state(), state)      # no particle was drawn


def test_distsampler_has_no_project_keyword():
    import inspect

    import dsvgd
    assert "project" in inspect.signature(dsvgd.Sampler.sample).parameters
    assert inspect.signature(dsvgd.Sampler.sample).parameters["project"].default is None
    assert "project" not in inspect.signature(dsvgd.DistSampler.__init__).parameters


# ---------------------------------------------------- the entry points --
NAMES = ("dsvgd_proj_gram_slices", "dsvgd_proj_gram_workspace_bytes", "dsvgd_proj_gram",
         "dsvgd_proj_apply", "dsvgd_proj_lift")


def test_library_exports_the_entry_points_and_abi_stays_4():
    from dsvgd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES
    assert _native.ABI_VERSION == 4
    assert _native.load().dsvgd_abi_version() == 4


def test_gram_slices_and_workspace():
    from dsvgd import _native as N
    lib = N.load()
    assert lib.dsvgd_proj_gram_slices(1, 1) == 1
    assert lib.dsvgd_proj_gram_slices(256, 33) == 1
    assert lib.dsvgd_proj_gram_slices(257, 33) == 2          # the first split
    for n, d in ((1, 1), (257, 33), (385, 40), (64, 1024), (65536, 256), (65536, 1024),
                 (1 << 22, 1024)):
        s = lib.dsvgd_proj_gram_slices(n, d)
        nb = -(-d // 128)
        assert s >= 1 and lib.dsvgd_proj_gram_workspace_bytes(n, d) == s * (nb * (nb + 1) // 2) * 65536
        per = -(-n // s)
        assert per <= 8192 + 32              # the longest chain of one accumulator
    for n, d in ((0, 4), (4, 0), (4, 1025)):
        assert lib.dsvgd_proj_gram_slices(n, d) == 0
        assert lib.dsvgd_proj_gram_workspace_bytes(n, d) == 0


def test_entry_points_validate_arguments_without_gpu():
    """Every call below fails a check: none reaches a launch."""
    from dsvgd import _native as N
    lib = N.load()
    buf = (ctypes.c_double * 64)()
    q = ctypes.addressof(buf)

    def err():
        return lib.dsvgd_last_error()

    def gram(a=(q, q, q, q), ldx=4, lds=4, n=3, d=4, add_x=1, ldh=4):
        return lib.dsvgd_proj_gram(a[0], ldx, a[1], lds, n, d, add_x, a[2], a[3], ldh, None)

    def apply(a=(q,) * 5, ldx=4, lds=4, n=3, d=4, ldpsi=2, r=2, ldxr=2, ldsr=2):
        return lib.dsvgd_proj_apply(a[0], ldx, a[1], lds, n, d, a[2], ldpsi, r, a[3], ldxr, a[4],
                                    ldsr, None)

    def lift(a=(q, q, q, q), ldphi=2, ldpsi=2, n=3, d=4, r=2, step=0.1, ldx=4, ldo=4):
        return lib.dsvgd_proj_lift(a[0], ldphi, a[1], ldpsi, n, d, r, step, a[2], ldx, a[3], ldo,
                                   None)
    for null in range(4):
        a = [q] * 4
        a[null] = None
        assert gram(a) == -1 and b"null" in err()
    for null in range(5):
        a = [q] * 5
        a[null] = None
        assert apply(a) == -1 and b"null" in err()
    for null in range(3):          # (Phi_out may be null)
        a = [q] * 4
        a[null] = None
        assert lift(a) == -1 and b"null" in err()
    for fn in (gram, apply, lift):
        assert fn(n=0) == -1 and b"n >= 1" in err()
        assert fn(d=0) == -1 and b"1 <= d <= 1024" in err()
        assert fn(d=1025) == -1 and b"1 <= d <= 1024" in err()
    for fn in (apply, lift):
        for r in (0, 5, -1):
            assert fn(r=r) == -1 and b"1 <= r <= min(d, 256)" in err()
        big = dict(d=300, ldx=300, r=257, ldpsi=257)
        assert fn(**big) == -1 and b"1 <= r <= min(d, 256)" in err()
    for kw in (dict(ldx=3), dict(lds=3), dict(ldh=3)):
        assert gram(**kw) == -1 and b"sizes" in err()
    for kw in (dict(ldx=3), dict(lds=3), dict(ldpsi=1), dict(ldxr=1), dict(ldsr=1)):
        assert apply(**kw) == -1 and b"sizes" in err()
    for kw in (dict(ldphi=1), dict(ldpsi=1), dict(ldx=3), dict(ldo=3)):
        assert lift(**kw) == -1 and b"sizes" in err()
