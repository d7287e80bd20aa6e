"""Posterior-predictive test accuracy of the logistic-regression experiment
(reference: experiments/logreg_plots.py:42-50, `_test_acc`), on the GPU.

    acc = mean_q[ (mean_j sigma(xt_q . w_j) > 0.5) == (t_q > 0) ]

over the particles x_j = [log alpha, w_j] (no bias; alpha unused, as the
reference).  The ensemble mean runs in `dsvgd_logreg_predict` (NT MFMA tiles
+ a fixed-order reduction over particle blocks); the reference evaluates it
in fp64 with numpy, this in fp32, so a test point whose mean probability is
within ~1e-6 of 0.5 may land on the other side.

`ksd` is the sampler's own convergence measure, for any target: the
kernelized Stein discrepancy of a particle set (no counterpart in the
reference; csrc/ksd.hip).  `mmd` is its two-sample counterpart: the maximum
mean discrepancy between two particle sets (csrc/mmd.hip).

`bnn_predict`, `bnn_rmse` and `bnn_loglik` evaluate the particles of the
Bayesian neural-network regression target (dsvgd.targets.BayesianNN) on a
test set: every particle's predictions in `dsvgd_bnn_predict` (csrc/bnn.hip),
the two reductions over them in fp64 torch on the device.

`gmix_logp` and `mode_shares` evaluate particles under a
dsvgd.targets.GaussianMixture: every particle's log density and its most
responsible component in `dsvgd_gmix_assign` (csrc/gmix.hip), the shares by a
bincount on the device.

`softmax_predict`, `softmax_accuracy` and `softmax_loglik` evaluate the
particles of dsvgd.targets.SoftmaxRegression on a test set: the mixture's
class probabilities in `dsvgd_softmax_predict` (csrc/softmax.hip), the two
reductions over them in torch on the device (the log-likelihood in fp64).
"""
import math

import torch

from . import _native as N


def _device_f32(a, dev):
    t = torch.as_tensor(a)
    if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
        t = t.to(device=dev, dtype=torch.float32).contiguous()
    return t


def ksd(particles, logp, kernel=None, *, statistic="v", squared=False, device=None):
    """Kernelized Stein discrepancy (Liu, Lee and Jordan 2016; Chwialkowski et
    al. 2016) between the particles and the target, for the RBF or the IMQ kernel: a
    convergence measure that needs only the particles, their scores and the
    kernel -- the quantity the SVGD direction descends on.

    particles: (n, d) tensor or array; logp: anything a Sampler takes, or an
    (n, d) tensor / array of precomputed scores grad log p(x_i); kernel:
    anything a Sampler takes (default RBF("median")).  A target with
    minibatches is scored on all of its data (its `full` twin).  statistic "v": the
    V-statistic (1/n^2) sum_ij u_ij (>= 0 up to rounding); "u": the unbiased
    U-statistic over i != j (may be negative; NaN for n = 1).  Returns a Python
    float: sqrt(max(., 0)), or the statistic itself with squared=True.

    Runs one engine evaluation on the GPU (PhiEngine.ksd): pack, distances,
    bandwidth, the K.[Xc | S] product with step 0 and the KSD sweep."""
    from .engine import PhiEngine
    from .kernels import RBF, resolve_kernel
    from .targets import resolve_target
    if statistic not in ("v", "u"):
        raise ValueError("statistic must be 'v' or 'u'")
    X = torch.as_tensor(particles)
    if X.dim() != 2:
        raise ValueError("particles must be (n, d), got shape %s" % (tuple(X.shape),))
    if device is None:
        device = X.device if X.is_cuda else "cuda"
    dev = N.require_gpu(device)
    X = _device_f32(X, dev)
    n, d = X.shape
    rbf = resolve_kernel(RBF("median") if kernel is None else kernel, d)
    scores = None
    if not callable(logp):
        scores = torch.as_tensor(logp)
        if tuple(scores.shape) != (n, d):
            raise ValueError("precomputed scores must have the particles' shape %s" % ((n, d),))
    if scores is not None:
        S = _device_f32(scores, dev)
    else:
        S = torch.empty(n, d, dtype=torch.float32, device=dev)
        target = resolve_target(logp)
        getattr(target, "full", target).score(X, S)
    eng = PhiEngine(n, d, device=dev, kernel=rbf)
    eng.pack(X, S)
    eng.distances(median=rbf.median)
    if rbf.median:
        eng.median_bandwidth()
    else:
        eng.fixed_bandwidth(rbf.h)
    eng.direction(step=0.0, write_phi=False)
    out = eng.ksd().cpu()
    val = float(out[2] if statistic == "v" else out[3])
    return val if squared else math.sqrt(max(val, 0.0))


def mmd(x, y, kernel=None, *, statistic="u", squared=False, details=False, device=None):
    """Maximum mean discrepancy (Gretton et al. 2012) between two particle
    sets x (n, d) and y (m, d), for the RBF or the IMQ kernel: how far one set
    is from another -- a run from exact draws of its target, an approximate
    exchange mode from the exact one -- where the KSD says how far a set is
    from a target.  Unlike the score-based KSD it sees wrong mixing
    proportions between well-separated modes.

    kernel: anything a Sampler takes.  None or a "median" kernel: h is the
    lower median of the pooled (n + m)^2 squared distances, diagonal included
    (1 if that is 0) -- WITHOUT the sampler's 1 / log N factor, under which
    typical pairs have k ~ 1 / N and the statistic degenerates to its
    diagonal.  A kernel with a number (RBF(h), IMQ(h, beta)) is used as given:
    that evaluates a run at the sampler's own bandwidth.

    statistic "u": the unbiased U-statistic (may be negative; NaN if a set has
    one point); "v": the V-statistic (>= 0 up to rounding).  Returns a Python
    float: sqrt(max(., 0)), or the statistic itself with squared=True.  With
    details=True a dict: mmd (that float), mmd2_v, mmd2_u, h, witness (the
    (n + m,) device tensor mean_j k(z_i, x_j) - mean_j k(z_i, y_j) over the
    pooled points z = [x; y]), n, m.

    Runs one engine evaluation on the GPU (PhiEngine.mmd): pack of the pooled
    set, distances, bandwidth and the MMD sweep.  The pooled (n + m)^2
    distance matrix is materialised; the engine refuses sets whose matrix does
    not fit the device, and a chunked path is out of scope."""
    from .engine import PhiEngine
    from .kernels import RBF, resolve_kernel
    if statistic not in ("v", "u"):
        raise ValueError("statistic must be 'v' or 'u'")
    X, Y = torch.as_tensor(x), torch.as_tensor(y)
    if X.dim() != 2 or Y.dim() != 2:
        raise ValueError("x and y must be (n, d) and (m, d), got shapes %s and %s"
                         % (tuple(X.shape), tuple(Y.shape)))
    if X.shape[1] != Y.shape[1]:
        raise ValueError("x and y must share the dimension d, got %d and %d"
                         % (X.shape[1], Y.shape[1]))
    n, m, d = X.shape[0], Y.shape[0], X.shape[1]
    if n < 1 or m < 1 or d < 1:
        raise ValueError("x and y must be non-empty, got shapes %s and %s"
                         % (tuple(X.shape), tuple(Y.shape)))
    kern = resolve_kernel(RBF("median") if kernel is None else kernel, d)
    if device is None:
        device = X.device if X.is_cuda else (Y.device if Y.is_cuda else "cuda")
    dev = N.require_gpu(device)
    Z = torch.cat([_device_f32(X, dev), _device_f32(Y, dev)], 0)
    eng = PhiEngine(n + m, d, device=dev, kernel=kern)
    eng.pack(Z)
    eng.distances(median=kern.median)
    if kern.median:
        eng.median_bandwidth()
        med = eng.state.read()[0]
        h = med if med > 0.0 else 1.0
    else:
        h = kern.h
    eng.fixed_bandwidth(h)
    if details:
        out, _, _, witness = eng.mmd(n, rows=True)
    else:
        out = eng.mmd(n)
    out = out.cpu()
    v, u = float(out[3]), float(out[4])
    val = v if statistic == "v" else u
    res = val if squared else math.sqrt(max(val, 0.0))   # (NaN -> NaN)
    if not details:
        return res
    return {"mmd": res, "mmd2_v": v, "mmd2_u": u, "h": eng.state.read()[1], "witness": witness,
            "n": n, "m": m}


def bnn_predict(particles, target_or_hidden, x_test):
    """(n, Nt) device tensor F[i][q] = f_i(x_test_q): every particle's network
    (dsvgd.targets.BayesianNN's layout) at the test rows, through
    `dsvgd_bnn_predict`.  target_or_hidden: the BayesianNN target, or its
    hidden width."""
    hidden = getattr(target_or_hidden, "hidden", target_or_hidden)
    X = torch.as_tensor(particles)
    dev = N.require_gpu(X.device if X.is_cuda else "cuda")
    X = _device_f32(X, dev)
    n, d = X.shape
    xt = _device_f32(x_test, dev)
    if xt.dim() != 2 or d != hidden * (xt.shape[1] + 2) + 3:
        raise ValueError("x_test must be (Nt, p) with d = hidden (p + 2) + 3 = %d" % d)
    Nt, p = xt.shape
    F = torch.empty(n, Nt, dtype=torch.float32, device=dev)
    N.call("dsvgd_bnn_predict", N.ptr(X), N.ld(X), n, d, N.ptr(xt), N.ld(xt), Nt, p, int(hidden),
           N.ptr(F), N.ld(F), N.stream(dev))
    return F


def bnn_rmse(particles, target, x_test, y_test):
    """RMSE of the particle-mean prediction on the test set (a Python float)."""
    F = bnn_predict(particles, target, x_test).double()
    y = torch.as_tensor(y_test).to(device=F.device, dtype=torch.float64).reshape(-1)
    return float(((F.mean(0) - y) ** 2).mean().sqrt())


def bnn_loglik(particles, target, x_test, y_test):
    """Mean test log-likelihood of the particle mixture,
    mean_q log (1/n) sum_i N(y_q; F_iq, 1 / gamma_i), gamma_i = exp(x_i[d-2]);
    reduced in fp64 on the device (a Python float)."""
    F = bnn_predict(particles, target, x_test).double()
    dev = F.device
    y = torch.as_tensor(y_test).to(device=dev, dtype=torch.float64).reshape(-1)
    lg = torch.as_tensor(particles)[:, -2].to(device=dev, dtype=torch.float64)
    comp = 0.5 * (lg[:, None] - math.log(2.0 * math.pi)) - 0.5 * torch.exp(lg)[:, None] * (y - F) ** 2
    return float((torch.logsumexp(comp, 0) - math.log(F.shape[0])).mean())


def _gmix_assign(particles, target):
    from .targets import GaussianMixture
    if not isinstance(target, GaussianMixture):
        raise ValueError("target must be a dsvgd.targets.GaussianMixture")
    X = torch.as_tensor(particles)
    if X.dim() != 2 or X.shape[1] != target.d:
        raise ValueError("particles must be (n, d) with d = %d, got shape %s"
                         % (target.d, tuple(X.shape)))
    dev = N.require_gpu(X.device if X.is_cuda else "cuda")
    return target.assign(_device_f32(X, dev))


def gmix_logp(particles, target):
    """(n,) device tensor: the normalised log density of every particle under
    the dsvgd.targets.GaussianMixture `target` (dsvgd_gmix_assign)."""
    return _gmix_assign(particles, target)[0]


def mode_shares(particles, target):
    """(K,) device tensor (fp64): the fraction of the particles whose most
    responsible component is k -- the mode-coverage diagnostic, to compare
    with `target.weights`.  The components come from dsvgd_gmix_assign (the
    lowest index on a tie), the count is torch.bincount on the device."""
    comp = _gmix_assign(particles, target)[1]
    counts = torch.bincount(comp.long(), minlength=target.K)
    return counts.double() / comp.numel()


def softmax_predict(particles, target_or_classes, x_test):
    """(Nt, C) device tensor P[q][c] = (1/n) sum_i softmax_c(W_i x_test_q): the
    posterior-predictive class probabilities of the particle mixture
    (dsvgd.targets.SoftmaxRegression's layout), through `dsvgd_softmax_predict`
    (the sum over the particles in a fixed order: the same bits on every
    call).  target_or_classes: the SoftmaxRegression target, or its C."""
    C = int(getattr(target_or_classes, "classes", target_or_classes))
    X = torch.as_tensor(particles)
    dev = N.require_gpu(X.device if X.is_cuda else "cuda")
    X = _device_f32(X, dev)
    n, d = X.shape
    xt = _device_f32(x_test, dev)
    if xt.dim() != 2 or d != 1 + C * xt.shape[1]:
        raise ValueError("x_test must be (Nt, p) with d = 1 + C p = %d" % d)
    Nt, p = xt.shape
    nbytes = N.load().dsvgd_softmax_predict_workspace_bytes(n, Nt, C)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device=dev)
    P = torch.empty(Nt, C, dtype=torch.float32, device=dev)
    N.call("dsvgd_softmax_predict", N.ptr(X), N.ld(X), n, d, N.ptr(xt), N.ld(xt), Nt, C, p,
           N.ptr(P), N.ld(P), N.ptr(ws), N.stream(dev))
    return P


def softmax_accuracy(particles, target, x_test, y_test):
    """Fraction of the test rows whose most probable class under
    softmax_predict is y_test (a Python float)."""
    P = softmax_predict(particles, target, x_test)
    y = torch.as_tensor(y_test).reshape(-1).to(device=P.device, dtype=torch.int64)
    return int((P.argmax(1) == y).sum()) / P.shape[0]


def softmax_loglik(particles, target, x_test, y_test):
    """Mean test log-likelihood of the particle mixture, mean_q log P[q, y_q],
    reduced in fp64 on the device (a Python float)."""
    P = softmax_predict(particles, target, x_test).double()
    y = torch.as_tensor(y_test).reshape(-1).to(device=P.device, dtype=torch.int64)
    return float(torch.log(torch.gather(P, 1, y[:, None])[:, 0]).mean())


def predictive_prob(particles, x_test):
    """(Nt,) device tensor: mean over particles of sigma(x_test . w)."""
    X = particles
    dev = N.require_gpu(X.device if X.is_cuda else "cuda")
    X = _device_f32(X, dev)
    n, d = X.shape
    xt = _device_f32(x_test, dev).reshape(-1, d - 1)
    Nt = xt.shape[0]
    nbytes = N.load().dsvgd_logreg_predict_workspace_bytes(n, Nt, d - 1)
    ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device=dev)
    aligned = (ws.data_ptr() + 255) // 256 * 256
    prob = torch.empty(Nt, dtype=torch.float32, device=dev)
    N.call("dsvgd_logreg_predict", N.ptr(X), N.ld(X), n, d, N.ptr(xt), N.ld(xt), Nt,
           N.ptr(prob), aligned, N.stream(dev))
    return prob


def test_accuracy(particles, x_test, t_test):
    """Fraction of test points whose ensemble-mean probability > 0.5 agrees
    with t_test > 0 (logreg_plots.py:42-50)."""
    prob = predictive_prob(particles, x_test)
    t = _device_f32(t_test, prob.device).reshape(-1)
    return int(((prob > 0.5) == (t > 0)).sum()) / prob.numel()
