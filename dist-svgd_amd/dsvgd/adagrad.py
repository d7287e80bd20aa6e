"""The AdaGrad step rule of Liu & Wang's SVGD code, for the Jacobi order.

With p = phi (+ the h * W2 rows) the whole direction of a moved row, per entry

    G' = p^2                          on the row's first step
    G' = alpha G + (1 - alpha) p^2    afterwards
    x += step_size * p / (eps + sqrt(G'))

The history G lives on the device beside the particles it belongs to
(dsvgd.engine.AdaGradState) and the update is one elementwise kernel behind
the direction (dsvgd_adagrad_step, csrc/adagrad.hip).  Absent in the
reference, whose samplers take fixed steps.
"""
import math


class AdaGrad(object):
    """Step rule for Sampler.sample(adagrad=...) and DistSampler(adagrad=...):
    alpha in [0, 1) the history's decay, eps > 0 the floor of the divisor."""

    def __init__(self, alpha=0.9, eps=1e-6):
        alpha, eps = float(alpha), float(eps)
        if not (0.0 <= alpha < 1.0):
            raise ValueError("AdaGrad decay alpha must lie in [0, 1), got %r" % (alpha,))
        if not (eps > 0.0 and math.isfinite(eps)):
            raise ValueError("AdaGrad eps must be finite and > 0, got %r" % (eps,))
        self.alpha = alpha
        self.eps = eps

    def __repr__(self):
        return "AdaGrad(alpha=%r, eps=%r)" % (self.alpha, self.eps)


def resolve_adagrad(adagrad):
    """None / False -> None (fixed steps), True -> AdaGrad(), an AdaGrad as is."""
    if adagrad is None or adagrad is False:
        return None
    if adagrad is True:
        return AdaGrad()
    if isinstance(adagrad, AdaGrad):
        return adagrad
    raise ValueError("adagrad must be None, True or a dsvgd.AdaGrad, got %r" % (adagrad,))
