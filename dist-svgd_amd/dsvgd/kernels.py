"""Kernel functions accepted by Sampler / DistSampler.

The reference takes an arbitrary Python callable `kernel(x, y) -> 0-d tensor`
(dsvgd/sampler.py:7-17, dsvgd/distsampler.py:9-25) and differentiates it by
autograd per pair.  Both experiment drivers pass the RBF kernel
exp(-||x - y||^2) (experiments/logreg.py:60-61, experiments/gmm.py:23-24).
The MI355X engine implements two radial families in closed form (fused into
the distance / phi kernels): the RBF exp(-||x-y||^2 / h) and the inverse
multiquadric (1 + ||x-y||^2 / h)^beta, -1 <= beta < 0.  A kernel argument is
resolved to an :class:`RBF` or an :class:`IMQ`:

* an :class:`RBF` or :class:`IMQ` instance is used as is (``RBF(h)`` fixed
  bandwidth, ``RBF("median")`` the median heuristic h = median(D) / log n;
  ``IMQ(h, beta)`` likewise);
* any other callable is probed on a few point pairs and accepted iff it
  behaves as exp(-||x-y||^2 / h) for one h (the reference's own kernels pass),
  or else as (1 + ||x-y||^2 / h)^beta for one (h, beta); anything else raises
  ``ValueError`` -- there is no per-pair autograd path.
"""
import math

import torch

MEDIAN = "median"


class RBF(object):
    """k(x, y) = exp(-||x - y||^2 / h); h a positive float or "median"."""

    def __init__(self, h=1.0):
        if h != MEDIAN:
            h = float(h)
            if not (h > 0.0 and math.isfinite(h)):
                raise ValueError("RBF bandwidth must be finite and > 0 (or 'median')")
        self.h = h

    @property
    def median(self):
        return self.h == MEDIAN

    def __call__(self, x, y):
        """Reference-compatible scalar evaluation (fixed h only)."""
        if self.median:
            raise ValueError("RBF('median') has no bandwidth outside a particle set")
        return torch.exp(-1. * torch.dist(x, y, p=2) ** 2 / self.h)

    def __repr__(self):
        return "RBF(h=%r)" % (self.h,)


class IMQ(object):
    """k(x, y) = (1 + ||x - y||^2 / h)^beta, the inverse multiquadric; h a
    positive float or "median" (the RBF's rule, h = median(D) / log n), beta
    in [-1, 0)."""

    def __init__(self, h=1.0, beta=-0.5):
        if h != MEDIAN:
            h = float(h)
            if not (h > 0.0 and math.isfinite(h)):
                raise ValueError("IMQ bandwidth must be finite and > 0 (or 'median')")
        beta = float(beta)
        if not (-1.0 <= beta < 0.0):
            raise ValueError("IMQ exponent beta must lie in [-1, 0), got %r" % (beta,))
        self.h = h
        self.beta = beta

    @property
    def median(self):
        return self.h == MEDIAN

    def __call__(self, x, y):
        """Reference-compatible scalar evaluation (fixed h only)."""
        if self.median:
            raise ValueError("IMQ('median') has no bandwidth outside a particle set")
        return (1. + torch.dist(x, y, p=2) ** 2 / self.h) ** self.beta

    def __repr__(self):
        return "IMQ(h=%r, beta=%r)" % (self.h, self.beta)


def resolve_kernel(kernel, d):
    """Return the RBF or IMQ equivalent to `kernel` or raise ValueError."""
    if isinstance(kernel, (RBF, IMQ)):
        return kernel
    if kernel is None:
        return RBF(1.0)
    if not callable(kernel):
        raise ValueError("kernel must be callable")
    try:
        return RBF(_probe_bandwidth(kernel, d))
    except ValueError as rbf_err:
        try:
            return IMQ(*_probe_imq(kernel, d))
        except ValueError as imq_err:
            raise ValueError(
                "dsvgd on MI355X supports two kernel families: the RBF exp(-||x-y||^2/h) "
                "(dsvgd.kernels.RBF) and the inverse multiquadric (1 + ||x-y||^2/h)^beta, "
                "-1 <= beta < 0 (dsvgd.kernels.IMQ).  As RBF: %s.  As IMQ: %s."
                % (rbf_err, imq_err))


def _probe_imq(kernel, d):
    """(h, beta) of a callable that behaves as (1 + ||x-y||^2/h)^beta on the
    probe radii of _probe_bandwidth, or ValueError.  With L(r2) = log k =
    beta log(1 + r2/h), the two largest radii a < b fix h as the root of
    log(1 + b/h) / log(1 + a/h) = L(b) / L(a) (monotone in h: bisection on
    log h), beta follows, and every radius must then agree."""
    gen = torch.Generator().manual_seed(1234)
    x = torch.randn(d, generator=gen)
    u = torch.randn(d, generator=gen)
    u = u / u.norm()
    if abs(float(kernel(x.clone(), x.clone())) - 1.0) > 1e-6:
        raise ValueError("kernel(x, x) != 1")
    pts = []
    for r2 in (1e-4, 1e-3, 1e-2, 1e-1, 1.0, 10.0):
        y = x + math.sqrt(r2) * u
        kxy = float(kernel(x.clone(), y.clone()))
        kyx = float(kernel(y.clone(), x.clone()))
        if abs(kxy - kyx) > 1e-6 * max(1.0, abs(kxy)):
            raise ValueError("kernel is not symmetric")
        if not (0.0 < kxy <= 1.0 + 1e-6):
            raise ValueError("kernel value %g outside (0, 1]" % kxy)
        pts.append((float(((x.double() - y.double()) ** 2).sum()), kxy))
    (ra, ka), (rb, kb) = pts[-2], pts[-1]
    if not (kb < ka < 1.0 - 1e-4):
        raise ValueError("kernel does not decrease with the distance")
    ratio = math.log(kb) / math.log(ka)

    def f(lh):     # increasing in h: from 1 (h -> 0) up to b / a (h -> inf)
        h = math.exp(lh)
        return math.log1p(rb / h) / math.log1p(ra / h) - ratio
    lo, hi = math.log(1e-6), math.log(1e6)
    if not (f(lo) < 0.0 < f(hi)):
        raise ValueError("no bandwidth in [1e-6, 1e6] fits the two largest radii")
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        if f(mid) < 0.0:
            lo = mid
        else:
            hi = mid
    h = math.exp(0.5 * (lo + hi))
    # fp32 kernel values pin the pair (h, beta) only loosely (a wide h moves
    # the ratio little): snap beta to the value a user most likely wrote,
    # take h from the largest radius with it, snap h too; the agreement test
    # below then decides
    beta = math.log(kb) / math.log1p(rb / h)
    for cand in (-1.0, -0.75, -0.5, -0.25, round(beta, 3)):
        if abs(cand - beta) <= 5e-3:
            beta = cand
            break
    if not (-1.0 <= beta < 0.0):
        raise ValueError("fitted exponent beta = %g outside [-1, 0)" % beta)
    h = rb / math.expm1(math.log(kb) / beta)
    for cand in (1.0, float("%.4g" % h)):
        if abs(cand - h) <= 1e-4 * h:
            h = cand
            break
    for r2, k in pts:    # every radius agrees (fp32 kernel values: ~1e-7 relative)
        want = (1.0 + r2 / h) ** beta
        if abs(k - want) > 2e-6 * max(1.0, want):
            raise ValueError("k = %.8g at |x-y|^2 = %g but (1 + r2/%.6g)^%.6g = %.8g"
                             % (k, r2, h, beta, want))
    return h, beta


def _probe_bandwidth(kernel, d):
    gen = torch.Generator().manual_seed(1234)
    x = torch.randn(d, generator=gen)
    u = torch.randn(d, generator=gen)
    u = u / u.norm()
    try:
        k0 = float(kernel(x.clone(), x.clone()))
    except Exception as e:  # noqa: BLE001
        raise ValueError("could not evaluate the kernel on CPU tensors of shape (%d,): %s" % (d, e))
    if abs(k0 - 1.0) > 1e-6:
        raise ValueError("kernel(x, x) = %g != 1: not an RBF kernel; dsvgd on MI355X supports "
                         "exp(-||x-y||^2/h) (use dsvgd.kernels.RBF)" % k0)
    hs = []
    for r2 in (1e-4, 1e-3, 1e-2, 1e-1, 1.0, 10.0):
        y = x + math.sqrt(r2) * u
        kxy = float(kernel(x.clone(), y.clone()))
        kyx = float(kernel(y.clone(), x.clone()))
        if abs(kxy - kyx) > 1e-6 * max(1.0, abs(kxy)):
            raise ValueError("kernel is not symmetric: not an RBF kernel")
        if 1e-30 < kxy < 1.0 - 1e-4:
            dist2 = float(((x.double() - y.double()) ** 2).sum())
            hs.append((abs(math.log(kxy)), -dist2 / math.log(kxy)))
    if not hs:
        raise ValueError("could not identify an RBF bandwidth for the given kernel")
    # the pair with the largest |log k| pins h best (fp32 kernel: err ~ 1e-7/|log k|)
    h = max(hs)[1]
    for lk, v in hs:
        if abs(v - h) > (1e-5 / lk + 1e-4) * h:
            raise ValueError("kernel is not of the form exp(-||x-y||^2/h) (bandwidth estimates "
                             "%s); dsvgd on MI355X supports RBF kernels only" % [e[1] for e in hs])
    # snap to the value a user most likely wrote (h=1 reference kernel)
    for cand in (1.0, round(h, 6)):
        if abs(cand - h) <= 1e-5 * h:
            return cand
    return h
