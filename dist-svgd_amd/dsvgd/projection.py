"""Projected SVGD (Chen & Ghattas, NeurIPS 2020): the particles interact in a
learned r-dimensional subspace and keep the orthogonal complement they were
drawn with.

Above a few dozen dimensions the pairwise distances of a radial kernel
concentrate, the repulsion of the SVGD direction vanishes and the particles
collapse towards the mode.  The target usually differs from the reference law
of the initial particles in a few directions only: the leading eigenvectors of
H = (1/n) sum_i g_i g_i^T, g = grad log(p / reference) (Zahm et al.'s certified
dimension reduction).  Per Jacobi iteration l, with particles X and scores S:

  refresh   (l % every == 0; once at l = 0 for every=None; never with a basis)
            G = S + X (reference="normal": N(0, I), the law Sampler.sample
            draws from) or S (reference=None), H = G^T G / n on the device
            (dsvgd_proj_gram), eigh(H) in fp64 on the host, Psi = the r leading
            eigenvectors, each signed so that its largest entry is positive
  project   Xr = X Psi, Sr = S Psi                      (dsvgd_proj_apply)
  step      phi_r of (Xr, Sr) on an r-wide PhiEngine, with the sampler's
            bandwidth rule (fixed h, or the median of the projected distances)
  lift      X += step . phi_r Psi^T                     (dsvgd_proj_lift)

With r = d the step is the plain SVGD step (the kernels are rotation
invariant), and X v is unchanged for every v orthogonal to span Psi.
"""
import numpy as np
import torch

from . import _native as N
from .engine import PhiEngine

MAX_D, MAX_RANK = 1024, 256      # dsvgd_proj_* (include/dsvgd.h)
ORTHO_TOL = 1e-6


def leading_basis(H, r):
    """(Psi, lam): eigh of the symmetric H in fp64 on the host; lam (d,)
    descending, Psi (d, r) the eigenvectors of the r largest, each signed so
    that its largest-magnitude entry is positive."""
    H = torch.as_tensor(H).detach().to("cpu", torch.float64)
    lam, V = torch.linalg.eigh(H)
    lam, V = lam.flip(0), V.flip(1)
    Psi = V[:, :r].clone()
    top = Psi.abs().argmax(dim=0)
    sign = torch.sign(Psi[top, torch.arange(r)])
    sign[sign == 0] = 1.0
    return Psi * sign, lam


class Projection(object):
    """The subspace of Sampler.sample(project=...).

    rank=r      learn an r-dimensional basis from the particles, refreshed
                every `every` iterations (every=None: once, at iteration 0);
    basis=Psi   a fixed (d, r) array or tensor with orthonormal columns
                (max |Psi^T Psi - I| <= 1e-6, checked once in fp64); `every`
                is ignored;
    reference   "normal": the particles were drawn from N(0, I), G = S + X;
                None: G = S.
    After a run: `basis` (d, r) on the device, `eigenvalues` (d,) fp64
    descending and `captured` = sum of the r leading / sum of all, both of the
    last refresh (None with a fixed basis), `refreshes` their number and
    `captured_history` the (iteration, captured) of each.
    `record_bases = True` keeps (iteration, Psi as fp32 numpy) of every refresh
    in `bases` (tests replay a run with them)."""

    def __init__(self, rank=None, basis=None, every=10, reference="normal"):
        if (rank is None) == (basis is None):
            raise ValueError("Projection takes exactly one of rank= and basis=")
        if reference not in ("normal", None):
            raise ValueError("reference must be 'normal' or None, got %r" % (reference,))
        self.reference = reference
        self._fixed = None
        if basis is not None:
            B = torch.as_tensor(np.asarray(basis.detach().cpu() if torch.is_tensor(basis)
                                           else basis)).to(torch.float64)
            if B.dim() != 2 or B.shape[1] < 1 or B.shape[1] > B.shape[0]:
                raise ValueError("basis must be a (d, r) array with 1 <= r <= d, got shape %s"
                                 % (tuple(B.shape),))
            if not bool(torch.isfinite(B).all()):
                raise ValueError("basis has non-finite entries")
            dev = float((B.t() @ B - torch.eye(B.shape[1], dtype=torch.float64)).abs().max())
            if dev > ORTHO_TOL:
                raise ValueError("basis columns are not orthonormal: max |Psi^T Psi - I| = %.3g "
                                 "> %g" % (dev, ORTHO_TOL))
            self._fixed = B
            self.rank = int(B.shape[1])
            self.every = None
        else:
            if isinstance(rank, bool) or int(rank) != rank or rank < 1:
                raise ValueError("rank must be a positive integer, got %r" % (rank,))
            self.rank = int(rank)
            if every is not None:
                if isinstance(every, bool) or int(every) != every or every < 1:
                    raise ValueError("every must be a positive integer (or None), got %r"
                                     % (every,))
                every = int(every)
            self.every = every
        if self.rank > MAX_RANK:
            raise ValueError("rank %d exceeds %d" % (self.rank, MAX_RANK))
        self.record_bases = False
        self._reset()

    def _reset(self):
        self.basis = None
        self.eigenvalues = None
        self.captured = None
        self.refreshes = 0
        self.captured_history = []
        self.bases = []

    def check(self, d):
        """The refusals that need the dimension (no GPU work)."""
        if not (1 <= d <= MAX_D):
            raise ValueError("projected SVGD needs 1 <= d <= %d, got d = %d" % (MAX_D, d))
        if self._fixed is not None and self._fixed.shape[0] != d:
            raise ValueError("basis has %d rows but the particles have d = %d"
                             % (self._fixed.shape[0], d))
        if self.rank > d:
            raise ValueError("rank %d exceeds d = %d" % (self.rank, d))

    def due(self, l):
        """Whether iteration l refreshes the basis."""
        if self._fixed is not None:
            return False
        return l == 0 if self.every is None else l % self.every == 0

    def begin(self, n, d, kernel, device):
        """The engine of a run that starts now (the results start afresh)."""
        self.check(d)
        self._reset()
        eng = ProjectedEngine(n, d, self.rank, device=device, kernel=kernel,
                              reference=self.reference)
        if self._fixed is not None:
            eng.set_basis(self._fixed)
        self.basis = eng.Psi
        return eng

    def refresh(self, eng, X, S, l=0):
        lam = eng.refresh(X, S)
        self.eigenvalues = lam
        total = float(lam.sum())
        self.captured = float(lam[:self.rank].sum()) / total if total > 0.0 else float("nan")
        self.refreshes += 1
        self.captured_history.append((l, self.captured))
        if self.record_bases:
            self.bases.append((l, eng.Psi.cpu().numpy().copy()))

    def __repr__(self):
        if self._fixed is not None:
            return "Projection(basis=<%d x %d>)" % tuple(self._fixed.shape)
        return "Projection(rank=%d, every=%r, reference=%r)" % (self.rank, self.every,
                                                                self.reference)


class ProjectedEngine(object):
    """Device side of projected SVGD for n particles in d dimensions and an
    r-dimensional subspace: the r-wide PhiEngine, the basis Psi (d, r) in a
    fixed buffer (a captured iteration reads it: replay stays valid across
    refreshes), the projected particles and scores Xr, Sr (n, r), H (d, d) and
    the Gram workspace."""

    def __init__(self, n, d, r, device=None, kernel=None, reference="normal"):
        if not (1 <= d <= MAX_D) or not (1 <= r <= min(d, MAX_RANK)) or n < 1:
            raise ValueError("ProjectedEngine needs n >= 1, 1 <= d <= %d and 1 <= r <= "
                             "min(d, %d); got n = %d, d = %d, r = %d" % (MAX_D, MAX_RANK, n, d, r))
        if reference not in ("normal", None):
            raise ValueError("reference must be 'normal' or None, got %r" % (reference,))
        dev = N.require_gpu(device if device is not None else "cuda")
        lib = N.load()
        self.n, self.d, self.r, self.device = n, d, r, dev
        self.add_x = reference == "normal"
        f32 = dict(dtype=torch.float32, device=dev)
        self.engine = PhiEngine(n, r, device=dev, kernel=kernel)
        self.Psi = torch.zeros(d, r, **f32)
        self.Xr = torch.empty(n, r, **f32)
        self.Sr = torch.empty(n, r, **f32)
        self.H = torch.empty(d, d, **f32)
        self.slices = int(lib.dsvgd_proj_gram_slices(n, d))
        self.ws = torch.empty(lib.dsvgd_proj_gram_workspace_bytes(n, d) // 4, **f32)
        self.phi = None          # direction()'s (n, d) output, allocated on first use

    def _check(self, X, S):
        if X.shape != (self.n, self.d) or S.shape != (self.n, self.d):
            raise ValueError("expected (%d, %d) particles and scores, got %s and %s"
                             % (self.n, self.d, tuple(X.shape), tuple(S.shape)))

    def set_basis(self, Psi):
        """Write a (d, r) basis (any float array or tensor) into the buffer."""
        Psi = torch.as_tensor(Psi)
        if tuple(Psi.shape) != (self.d, self.r):
            raise ValueError("basis must be (%d, %d), got %s"
                             % (self.d, self.r, tuple(Psi.shape)))
        self.Psi.copy_(Psi.to(torch.float32))

    def gram(self, X, S):
        """H = (1/n) G^T G into self.H (stream-ordered, no host work)."""
        self._check(X, S)
        N.call("dsvgd_proj_gram", N.ptr(X), N.ld(X), N.ptr(S), N.ld(S), self.n, self.d,
               int(self.add_x), N.ptr(self.ws), N.ptr(self.H), N.ld(self.H),
               N.stream(self.device))
        return self.H

    def refresh(self, X, S):
        """A new basis from the particles and their scores: the Gram on the
        device, eigh in fp64 on the host (this synchronises), Psi back into
        the fixed buffer.  Returns the eigenvalues (d,) fp64, descending."""
        H = self.gram(X, S).cpu()
        Psi, lam = leading_basis(H, self.r)
        self.set_basis(Psi)
        return lam

    def project(self, X, S):
        """Xr = X Psi, Sr = S Psi."""
        self._check(X, S)
        N.call("dsvgd_proj_apply", N.ptr(X), N.ld(X), N.ptr(S), N.ld(S), self.n, self.d,
               N.ptr(self.Psi), N.ld(self.Psi), self.r, N.ptr(self.Xr), N.ld(self.Xr),
               N.ptr(self.Sr), N.ld(self.Sr), N.stream(self.device))

    def lift(self, step, X=None, phi_out=None):
        """X += step . phi_r Psi^T from the r-wide engine's direction;
        phi_out (n, d), if given, is set to phi_r Psi^T."""
        pr = self.engine.phi
        N.call("dsvgd_proj_lift", N.ptr(pr), N.ld(pr), N.ptr(self.Psi), N.ld(self.Psi), self.n,
               self.d, self.r, float(step), N.ptr(X), N.ld(X) if X is not None else self.d,
               N.ptr(phi_out), N.ld(phi_out) if phi_out is not None else self.d,
               N.stream(self.device))

    def _subspace(self, X, S, h):
        self.project(X, S)
        self.engine.step(self.Xr, self.Sr, step=0.0, h=h, write_phi=True)

    def step(self, X, S, step, h=None):
        """One projected Jacobi step of X in place (h=None: the median of the
        projected distances / log n).  Kernel launches only: capturable."""
        self._subspace(X, S, h)
        self.lift(step, X=X)

    def direction(self, X, S, h=None):
        """phi = phi_r Psi^T (n, d) without moving anything."""
        if self.phi is None:
            self.phi = torch.empty(self.n, self.d, dtype=torch.float32, device=self.device)
        self._subspace(X, S, h)
        self.lift(0.0, phi_out=self.phi)
        return self.phi
