"""Target densities: batched scores grad log p(X) for all particles at once.

The reference differentiates a per-particle Python `logp(x) -> 0-d tensor`
with autograd, once per interacting pair (dsvgd/sampler.py:28-33,
dsvgd/distsampler.py:77-82).  Here a target computes the scores of ALL n
particles in one batched device call:

* built-in targets run hand-written gfx950 kernels (libdsvgd_hip.so):
  :class:`Gaussian`, :class:`GaussianMixture1D` (experiments/gmm.py:16-21),
  :class:`LogisticRegression` (experiments/logreg.py:45-58, two MFMA GEMMs),
  :class:`BayesianNN` (beyond the reference: one kernel, csrc/bnn.hip),
  :class:`GaussianMixture` (K components with diagonal precisions in d
  dimensions: one kernel, csrc/gmix.hip),
  :class:`SoftmaxRegression` (multiclass logistic regression: two f32 MFMA
  products around a lane-local softmax, csrc/softmax.hip);
* any other `logp` callable is wrapped by :class:`CallableTarget`, which runs
  the user's own torch code under ``torch.func.vmap(torch.func.grad(logp))``
  on the particles' device (user code, not a dsvgd compute path).

Every target is also a reference-compatible callable ``target(x) -> log p(x)``
so it can be handed to the reference implementation unchanged.
"""
import math

import numpy as np
import torch

from . import _native as N


def _host_bytes(t):
    """The bytes of a tensor's values wherever it lives (a target built from
    device tensors digests the same as one built from host tensors)."""
    return t.detach().cpu().contiguous().numpy().tobytes()


class Target(object):
    def score(self, X, out, scale=1.0):
        """out[:] = scale * grad log p(X) for X (n, d) on the device."""
        raise NotImplementedError

    def next_batch(self):
        """Move to the next minibatch of the data (the samplers call this once
        per iteration, after its last score call).  Full-data targets: nothing."""

    def reset_batch(self, t=0):
        """Set the minibatch of iteration t.  Full-data targets: nothing."""

    def __call__(self, x):
        return self.logp(x)


class BuiltinTarget(Target):
    """Targets whose score is a libdsvgd_hip kernel sequence (graph-capturable)."""


class _Windowed(object):
    """The minibatch window of a data target (BayesianNN, LogisticRegression):
    batch=B with 1 <= B < N scores the cyclic window of B rows that starts at a
    cursor kept on the device, one per device.  The host keeps only where a
    cursor made from now on starts."""

    def _init_batch(self, batch):
        if batch is not None:
            if isinstance(batch, bool) or int(batch) != batch or batch < 1:
                raise ValueError("batch must be a positive integer (or None), got %r" % (batch,))
            batch = int(batch) if batch < self.N else None    # the whole data: no window
        self.batch = batch
        self._cursor = {}     # device -> int64[1], the window's first row
        self._origin = 0      # where a cursor made from now on starts
        self._last = None     # the device of the last score call
        self._full = None

    @property
    def full(self):
        """The full-data target over the same tensors (itself without a batch)."""
        if self.batch is None:
            return self
        if self._full is None:
            twin = type(self).__new__(type(self))
            twin.__dict__.update(self.__dict__)
            twin.batch, twin._cursor, twin._full = None, {}, None
            self._full = twin
        return self._full

    def _window(self, dev):
        """The cursor of `dev` (made on first use, outside any capture: the
        samplers' first iteration runs eagerly)."""
        cur = self._cursor.get(dev)
        if cur is None:
            cur = self._cursor[dev] = torch.full((1,), self._origin, dtype=torch.int64, device=dev)
        self._last = dev
        return cur

    def next_batch(self):
        """The window of the device in use (the last one scored on) moves by
        `batch` rows, on that device's current stream."""
        if self.batch is None:
            return
        if self._last is None:     # no device yet: the first cursor starts a window on
            self._origin = (self._origin + self.batch) % self.N
            return
        N.call("dsvgd_window_advance", N.ptr(self._cursor[self._last]), self.batch, self.N,
               N.stream(self._last))

    def reset_batch(self, t=0):
        """Every cursor (and any made later) to iteration t's window, (t batch) mod N."""
        if self.batch is None:
            return
        self._origin = (int(t) * self.batch) % self.N
        for cur in self._cursor.values():
            cur.fill_(self._origin)


class Gaussian(BuiltinTarget):
    """N(mu, diag(1/lam)): log p = -1/2 sum_c lam_c (x_c - mu_c)^2 (+ const)."""

    def __init__(self, mu, lam):
        self.mu = torch.as_tensor(mu, dtype=torch.float32).reshape(-1)
        self.lam = torch.as_tensor(lam, dtype=torch.float32).reshape(-1)
        self._dev = {}

    def logp(self, x):
        mu, lam = self.mu.to(x.device), self.lam.to(x.device)
        return -0.5 * (lam * (x - mu) ** 2).sum()

    def _params(self, dev):
        if dev not in self._dev:
            self._dev[dev] = (self.mu.to(dev).contiguous(), self.lam.to(dev).contiguous())
        return self._dev[dev]

    def fingerprint(self):
        import hashlib
        return hashlib.sha1(b"gauss" + _host_bytes(self.mu) + _host_bytes(self.lam)).hexdigest()

    def score(self, X, out, scale=1.0):
        n, d = X.shape
        assert d == self.mu.numel(), "Gaussian target has d=%d" % self.mu.numel()
        mu, lam = self._params(X.device)
        N.call("dsvgd_score_gaussian", N.ptr(X), N.ld(X), n, d, N.ptr(mu), N.ptr(lam),
               float(scale), N.ptr(out), N.ld(out), N.stream(X.device))


class GaussianMixture1D(BuiltinTarget):
    """log(1/3 N(x; -2, 1) + 1/3 N(x; 2, 1)) per coordinate (experiments/gmm.py:16-21;
    the code uses equal 1/3 weights although its comment says 1/3, 2/3)."""

    def logp(self, x):
        a = -0.5 * (x + 2.0) ** 2
        b = -0.5 * (x - 2.0) ** 2
        return (torch.logaddexp(a, b) + math.log(1.0 / 3.0) - 0.5 * math.log(2 * math.pi)).sum()

    def fingerprint(self):
        return "gmm1d"

    def score(self, X, out, scale=1.0):
        n, d = X.shape
        N.call("dsvgd_score_gmm", N.ptr(X), N.ld(X), n, d, float(scale), N.ptr(out),
               N.ld(out), N.stream(X.device))


class LogisticRegression(_Windowed, BuiltinTarget):
    """Bayesian logistic regression of experiments/logreg.py:45-58.

    x = [log alpha, w] (d = 1 + p); alpha ~ Gamma(1, 1) (no log-Jacobian, as in
    the reference), w ~ N(0, I/alpha), labels t in {-1, +1}.

    batch=B with 1 <= B < N scores a minibatch, by BayesianNN's rules: the
    likelihood over the cyclic window of B rows that starts at a cursor kept
    on the device, weighted N / B, the prior once (dsvgd_score_logreg_window,
    exact fp32 whatever `gemm` is, for every n).  next_batch() moves the window
    by B rows, reset_batch(t) puts it at (t B) mod N; `logp` stays the
    full-data density and `full` is the full-data twin (evaluation,
    dsvgd.metrics.ksd; it shares this target's prepared workspaces).
    batch=None or batch >= N is the full-data target.
    """

    ENGINES = {"h2": 0, "x3": 1, "f32": 2}   # dsvgd_score_logreg_engine
    SMALL_ROWS = 32      # one-block-per-particle path (no workspace), csrc/logreg.hip

    def __init__(self, x_train, t_train, gemm="h2", batch=None):
        self.x = torch.as_tensor(x_train, dtype=torch.float32)
        self.t = torch.as_tensor(t_train, dtype=torch.float32).reshape(-1)
        assert self.x.shape[0] == self.t.shape[0]
        if gemm not in self.ENGINES:
            raise ValueError("gemm must be one of %s" % sorted(self.ENGINES))
        self.gemm = gemm
        self._init_batch(batch)
        self._dev = {}
        self._ws = {}             # workspace key -> buffer, least recently used first
        self._prepared = {}       # workspace key -> engine whose data image it holds
        self._pinned = set()      # keys a captured HIP graph holds (never evicted)

    @property
    def N(self):
        return self.x.shape[0]

    def logp(self, x):
        from torch.distributions.gamma import Gamma
        from torch.distributions.multivariate_normal import MultivariateNormal
        xt, tt = self.x.to(x.device), self.t.to(x.device)
        p = xt.shape[1]
        alpha = torch.exp(x[0])
        w = x[1:].reshape(-1)
        lp = Gamma(torch.tensor(1., device=x.device), torch.tensor(1., device=x.device)).log_prob(alpha)
        lp = lp + MultivariateNormal(torch.zeros(p, device=x.device),
                                     torch.eye(p, device=x.device) / alpha).log_prob(w)
        lp = lp + (-torch.log(1. + torch.exp(-1. * torch.mv(tt[:, None] * xt, w))).sum())
        return lp

    def _params(self, dev):
        if dev not in self._dev:
            self._dev[dev] = (self.x.to(dev).contiguous(), self.t.to(dev).contiguous())
        return self._dev[dev]

    def _params_aligned(self, dev):
        """(data with 16-byte rows -- ld = roundup(p, 4), zero pad -- labels)
        on dev: the Gauss-Seidel walk's one-pass score refresh
        (dsvgd_gsw_block_sweep, score_kind 3) reads the rows as dwordx4."""
        key = ("aligned", dev)
        if key not in self._dev:
            xd, t = self._params(dev)
            p = xd.shape[1]
            pa = -(-p // 4) * 4
            buf = torch.zeros(xd.shape[0], pa, dtype=torch.float32, device=dev)
            buf[:, :p] = xd
            self._dev[key] = (buf, t)
        return self._dev[key]

    def fingerprint(self):
        """Digest of the data, and of the batch of a minibatch target
        (DistSampler: ranks whose targets agree on it hold the same data, so
        their scores of a particle are the same)."""
        import hashlib
        import struct
        h = hashlib.sha1(b"logreg")
        if self.batch is not None:
            h.update(struct.pack("<q", self.batch))
        h.update(_host_bytes(self.x))
        h.update(_host_bytes(self.t))
        return h.hexdigest()

    MAX_WORKSPACES = 4   # unpinned score workspaces kept (least recently used evicted)

    def _workspace(self, key, n, d, dev):
        ws = self._ws.pop(key, None)
        if ws is None:
            nbytes = N.load().dsvgd_logreg_workspace_bytes(n, self.N, d - 1) if key[1] else 256
            ws = torch.empty(nbytes // 4 + 64, dtype=torch.float32, device=dev)
        self._ws[key] = ws                     # most recently used last
        if torch.cuda.is_current_stream_capturing():
            self._pinned.add(key)              # a graph now holds its address
        free = [k for k in self._ws if k not in self._pinned and k != key]
        for k in free[:max(0, len(free) + 1 - self.MAX_WORKSPACES)]:
            del self._ws[k]
            self._prepared.pop(k, None)
        return ws

    def score(self, X, out, scale=1.0, prior_weight=1.0):
        """out = scale * grad log p(X); prior_weight != 1 weighs the prior
        terms (DistSampler's gathered-data all_scores: the prior of S ranks'
        logp, distsampler.py:160-170), on the prepared path only.  A minibatch
        target scores its window for every n (no workspace) and refuses a
        prior_weight: the gathered-data mode has no windows."""
        n, d = X.shape
        assert d == self.x.shape[1] + 1, "logreg target has d = 1 + p = %d" % (self.x.shape[1] + 1)
        xd, t = self._params(X.device)
        if self.batch is not None:
            if prior_weight != 1.0:
                raise ValueError("prior_weight needs the full-data target (batch=None)")
            N.call("dsvgd_score_logreg_window", N.ptr(X), N.ld(X), n, d, N.ptr(xd), N.ld(xd),
                   N.ptr(t), self.N, float(scale), N.ptr(out), N.ld(out), None,
                   self.ENGINES[self.gemm], N.ptr(self._window(X.device)), self.batch,
                   N.stream(X.device))
            return
        # one workspace per (device, n): the ones a captured HIP graph
        # (engine.StepGraph) holds are pinned and never freed behind it
        # (release() frees them explicitly); of the others the
        # MAX_WORKSPACES most recently used stay.  The few-particle path
        # (the Gauss-Seidel refreshes) needs none.
        small = bool(N.load().dsvgd_logreg_small(n, self.N, d - 1))   # logreg.hip's own test
        key = (X.device, 0 if small else n)
        ws = self._workspace(key, n, d, X.device)
        base = ws.data_ptr()
        aligned = (base + 255) // 256 * 256
        eng = self.ENGINES[self.gemm]
        s = N.stream(X.device)
        if small:
            if prior_weight != 1.0:
                raise ValueError("prior_weight needs more than %d particles" % self.SMALL_ROWS)
            N.call("dsvgd_score_logreg_engine", N.ptr(X), N.ld(X), n, d, N.ptr(xd), N.ld(xd),
                   N.ptr(t), self.N, float(scale), N.ptr(out), N.ld(out), aligned, eng, s)
            return
        if self._prepared.get(key) != eng:
            # the data-only half of the workspace (padded data, its scales
            # and split images) once per workspace; every later step reuses it
            N.call("dsvgd_logreg_prepare", N.ptr(xd), N.ld(xd), N.ptr(t), self.N, n, d, aligned,
                   eng, s)
            self._prepared[key] = eng
            if not torch.cuda.is_current_stream_capturing():
                # later calls may come on other streams (the DistSampler side stream)
                torch.cuda.current_stream(X.device).synchronize()
        if prior_weight != 1.0:
            N.call("dsvgd_score_logreg_prior", N.ptr(X), N.ld(X), n, d, self.N, float(scale),
                   float(prior_weight), N.ptr(out), N.ld(out), aligned, eng, s)
            return
        N.call("dsvgd_score_logreg_prepared", N.ptr(X), N.ld(X), n, d, self.N, float(scale),
               N.ptr(out), N.ld(out), aligned, eng, s)

    def release(self):
        """Free the score workspaces (no graph that captured them may replay after)."""
        self._ws.clear()
        self._prepared.clear()
        self._pinned.clear()


class BayesianNN(_Windowed, BuiltinTarget):
    """Bayesian neural-network regression (Liu & Wang 2016): one hidden ReLU
    layer of `hidden` units, Gamma(a0, b0) hyper-priors on the noise precision
    gamma and the weight precision lambda (carried as logs, with the
    log-Jacobian).  Not in the reference, whose users would pass this logp.

        x = [vec(W1) (p x H row-major) | b1 (H) | w2 (H) | b2 | log gamma | log lambda]
        d = H (p + 2) + 3,   f(z) = w2 . relu(W1^T z + b1) + b2

    The score is one kernel, a workgroup per particle (csrc/bnn.hip).

    batch=B with 1 <= B < N scores a minibatch (Liu & Wang's estimate): the
    likelihood over the cyclic window of B rows that starts at a cursor kept
    on the device, weighted N / B, the priors once.  next_batch() moves the
    window by B rows (a kernel: it replays inside a captured iteration),
    reset_batch(t) puts it where iteration t finds it, (t B) mod N.  `logp`
    stays the full-data density and `full` is the full-data twin (evaluation,
    dsvgd.metrics.ksd).  batch=None or batch >= N is the full-data target."""

    MAX_WIDTH = 64    # largest p and hidden (dsvgd_score_bnn)

    def __init__(self, x_train, y_train, hidden=50, a0=1.0, b0=0.1, batch=None):
        self.x = torch.as_tensor(x_train, dtype=torch.float32)
        self.y = torch.as_tensor(y_train, dtype=torch.float32).reshape(-1)
        if self.x.dim() != 2 or self.x.shape[0] != self.y.shape[0] or self.x.shape[0] < 1:
            raise ValueError("x_train must be (N, p) and y_train (N,), N >= 1")
        self.hidden = int(hidden)
        if not 1 <= self.hidden <= self.MAX_WIDTH:
            raise ValueError("hidden must be in [1, %d], got %r" % (self.MAX_WIDTH, hidden))
        if not 1 <= self.p <= self.MAX_WIDTH:
            raise ValueError("x_train must have 1 to %d columns, got %d" % (self.MAX_WIDTH, self.p))
        self.a0, self.b0 = float(a0), float(b0)
        self._init_batch(batch)
        self._dev = {}

    @property
    def N(self):
        return self.x.shape[0]

    @property
    def p(self):
        return self.x.shape[1]

    @property
    def d(self):
        return self.hidden * (self.p + 2) + 3

    def unpack(self, x):
        """(W1 (p, H), b1, w2, b2, log gamma, log lambda) views of a particle."""
        p, H = self.p, self.hidden
        return (x[:p * H].reshape(p, H), x[p * H:p * H + H], x[p * H + H:p * H + 2 * H],
                x[p * H + 2 * H], x[-2], x[-1])

    def logp(self, x):
        if x.shape[-1] != self.d:
            raise ValueError("BayesianNN target has d = H (p + 2) + 3 = %d" % self.d)
        z, y = self.x.to(device=x.device, dtype=x.dtype), self.y.to(device=x.device, dtype=x.dtype)
        W1, b1, w2, b2, lg, ll = self.unpack(x)
        r = y - (torch.relu(z @ W1 + b1) @ w2 + b2)
        theta = x[:-2]
        return (0.5 * self.N * lg - 0.5 * torch.exp(lg) * (r * r).sum()
                + 0.5 * (self.d - 2) * ll - 0.5 * torch.exp(ll) * (theta * theta).sum()
                + self.a0 * lg - self.b0 * torch.exp(lg) + self.a0 * ll - self.b0 * torch.exp(ll))

    def _params(self, dev):
        if dev not in self._dev:
            self._dev[dev] = (self.x.to(dev).contiguous(), self.y.to(dev).contiguous())
        return self._dev[dev]

    def fingerprint(self):
        """Digest of the data and the model (hidden, a0, b0, and the batch of
        a minibatch target)."""
        import hashlib
        import struct
        h = hashlib.sha1(b"bnn")
        h.update(struct.pack("<qqqdd", self.N, self.p, self.hidden, self.a0, self.b0))
        if self.batch is not None:
            h.update(struct.pack("<q", self.batch))
        h.update(_host_bytes(self.x))
        h.update(_host_bytes(self.y))
        return h.hexdigest()

    def score(self, X, out, scale=1.0):
        n, d = X.shape
        assert d == self.d, "BayesianNN target has d = H (p + 2) + 3 = %d" % self.d
        z, y = self._params(X.device)
        if self.batch is not None:
            N.call("dsvgd_score_bnn_window", N.ptr(X), N.ld(X), n, d, N.ptr(z), N.ld(z), N.ptr(y),
                   self.N, self.p, self.hidden, self.a0, self.b0, float(scale),
                   N.ptr(self._window(X.device)), self.batch, N.ptr(out), N.ld(out),
                   N.stream(X.device))
            return
        N.call("dsvgd_score_bnn", N.ptr(X), N.ld(X), n, d, N.ptr(z), N.ld(z), N.ptr(y), self.N,
               self.p, self.hidden, self.a0, self.b0, float(scale), N.ptr(out), N.ld(out),
               N.stream(X.device))


class GaussianMixture(BuiltinTarget):
    """sum_k w~_k N(x; mu_k, diag(1 / lam_k)) in d dimensions, w~ = w / sum(w).

    means: (K, d); precisions: anything that broadcasts to (K, d), finite and
    > 0 (default 1); weights: (K,), finite and > 0 (default equal), normalised
    here: `weights` holds w~ in fp64.  d <= 1024.

    The score is one kernel (csrc/gmix.hip): one pass over the components with
    a running maximum, so any K, and finite scores however far a particle is
    from every mode.  `assign` gives every particle's log density and its most
    responsible component (dsvgd.metrics.gmix_logp / mode_shares)."""

    MAX_D = 1024    # dsvgd_score_gmix

    def __init__(self, means, precisions=1.0, weights=None):
        self.means = torch.as_tensor(means).detach().to(torch.float32)
        if self.means.dim() != 2 or self.means.shape[0] < 1 or self.means.shape[1] < 1:
            raise ValueError("means must be (K, d) with K, d >= 1, got shape %s"
                             % (tuple(self.means.shape),))
        if not bool(torch.isfinite(self.means).all()):
            raise ValueError("means must be finite")
        K, d = self.means.shape
        if d > self.MAX_D:
            raise ValueError("GaussianMixture supports d <= %d, got %d" % (self.MAX_D, d))
        lam = torch.as_tensor(precisions).detach().to(torch.float32)
        try:
            lam = torch.broadcast_to(lam, (K, d))
        except RuntimeError:
            raise ValueError("precisions must broadcast to (K, d) = %s, got shape %s"
                             % ((K, d), tuple(lam.shape))) from None
        if not bool((torch.isfinite(lam) & (lam > 0)).all()):
            raise ValueError("precisions must be finite and > 0")
        self.precisions = lam.contiguous()
        if weights is not None and not isinstance(weights, torch.Tensor):
            try:
                weights = np.asarray(weights, dtype=np.float64)   # Python floats keep their fp64
            except (TypeError, ValueError):
                raise ValueError("weights must be (K,) numbers") from None
        w = torch.ones(K, dtype=torch.float64) if weights is None else \
            torch.as_tensor(weights).detach().to(device="cpu", dtype=torch.float64)
        if tuple(w.shape) != (K,):
            raise ValueError("weights must be (K,) = (%d,), got shape %s" % (K, tuple(w.shape)))
        if not bool((torch.isfinite(w) & (w > 0)).all()):
            raise ValueError("weights must be finite and > 0")
        self.weights = w / w.sum()
        # c_k = log w~_k + 1/2 sum_c log lam_kc, in fp64 on the host
        self._c = torch.log(self.weights) + 0.5 * torch.log(self.precisions.double().cpu()).sum(1)
        self._dev = {}

    @property
    def K(self):
        return self.means.shape[0]

    @property
    def d(self):
        return self.means.shape[1]

    def logp(self, x):
        """The normalised log density of one particle x (d,), in x's dtype."""
        if x.shape[-1] != self.d:
            raise ValueError("GaussianMixture target has d = %d" % self.d)
        mu = self.means.to(device=x.device, dtype=x.dtype)
        lam = self.precisions.to(device=x.device, dtype=x.dtype)
        c = self._c.to(device=x.device, dtype=x.dtype)
        q = 0.5 * (lam * (x - mu) ** 2).sum(-1)
        return torch.logsumexp(c - q, -1) - 0.5 * self.d * math.log(2.0 * math.pi)

    def sample(self, m, seed=None, device=None):
        """m exact draws as an (m, d) fp32 tensor (on `device` if given, else
        on the host): a component k from the normalised weights, then mu_k +
        eps / sqrt(lam_k), eps ~ N(0, I).  Drawn with a torch.Generator on the
        CPU, so a seed gives the same draws on every machine and device
        (seed=None: a fresh random seed).  The reference set of
        dsvgd.metrics.mmd."""
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or m < 1:
            raise ValueError("m must be an integer >= 1, got %r" % (m,))
        g = torch.Generator(device="cpu")
        if seed is None:
            g.seed()
        else:
            g.manual_seed(int(seed))
        comp = torch.multinomial(self.weights, int(m), replacement=True, generator=g)
        eps = torch.randn(int(m), self.d, generator=g, dtype=torch.float32)
        x = self.means.cpu()[comp] + eps / torch.sqrt(self.precisions.cpu()[comp])
        return x if device is None else x.to(device)

    def _params(self, dev):
        """(means, precisions, c) on dev, made on first use (outside any
        capture: the samplers' first iteration runs eagerly)."""
        if dev not in self._dev:
            self._dev[dev] = (self.means.to(dev).contiguous(), self.precisions.to(dev).contiguous(),
                              self._c.to(device=dev, dtype=torch.float32).contiguous())
        return self._dev[dev]

    def fingerprint(self):
        """Digest of K, d, the means, the precisions and the normalised weights."""
        import hashlib
        import struct
        h = hashlib.sha1(b"gmix")
        h.update(struct.pack("<qq", self.K, self.d))
        for t in (self.means, self.precisions, self.weights):
            h.update(_host_bytes(t))
        return h.hexdigest()

    def score(self, X, out, scale=1.0):
        n, d = X.shape
        assert d == self.d, "GaussianMixture target has d = %d" % self.d
        mu, lam, c = self._params(X.device)
        N.call("dsvgd_score_gmix", N.ptr(X), N.ld(X), n, d, N.ptr(mu), N.ld(mu), N.ptr(lam),
               N.ld(lam), N.ptr(c), self.K, float(scale), N.ptr(out), N.ld(out),
               N.stream(X.device))

    def assign(self, X):
        """(logp (n,) float32, comp (n,) int32) on X's device: every particle's
        normalised log density and its most responsible component, the lowest
        index on a tie (dsvgd_gmix_assign)."""
        n, d = X.shape
        assert d == self.d, "GaussianMixture target has d = %d" % self.d
        mu, lam, c = self._params(X.device)
        logp = torch.empty(n, dtype=torch.float32, device=X.device)
        comp = torch.empty(n, dtype=torch.int32, device=X.device)
        N.call("dsvgd_gmix_assign", N.ptr(X), N.ld(X), n, d, N.ptr(mu), N.ld(mu), N.ptr(lam),
               N.ld(lam), N.ptr(c), self.K, N.ptr(logp), N.ptr(comp), N.stream(X.device))
        return logp, comp


class SoftmaxRegression(_Windowed, BuiltinTarget):
    """Bayesian softmax (multiclass logistic) regression: data rows xd_q in R^p
    with labels y_q in {0..C-1}, no bias term (append a ones column, as for
    LogisticRegression).  Not in the reference, whose users would pass this logp.

        x = [log alpha | vec(W)] with W (C, p) row-major,   d = 1 + C p
        W_ck ~ N(0, 1 / alpha),  alpha ~ Gamma(a0, b0)
        log p = sum_q log softmax(W xd_q)[y_q] + (C p / 2) x_0 - alpha |W|^2 / 2
                + a0 x_0 - b0 alpha

    alpha is carried as its log WITH the log-Jacobian (the a0 x_0 term): this
    is BayesianNN's convention, not LogisticRegression's, which follows the
    reference's logreg and has none.

    classes=None takes C = max(y) + 1.  2 <= C <= MAX_CLASSES, p >= 1 and
    d <= MAX_D.  The score is csrc/softmax.hip: both products on the f32 MFMA
    for more than a few particles, a workgroup per particle below that (the
    sequential order's per-row refresh).

    batch=B with 1 <= B < N scores a minibatch, by BayesianNN's rules: the
    data sum over the cyclic window of B rows that starts at a cursor kept on
    the device, weighted N / B, the prior terms once.  next_batch() moves the
    window by B rows, reset_batch(t) puts it at (t B) mod N; `logp` stays the
    full-data density and `full` is the full-data twin (evaluation,
    dsvgd.metrics.ksd).  batch=None or batch >= N is the full-data target."""

    MAX_CLASSES = 16    # DSVGD_SOFTMAX_MAX_CLASSES
    MAX_D = 1024        # dsvgd_score_softmax

    def __init__(self, x_train, y_train, classes=None, a0=1.0, b0=1.0, batch=None):
        self.x = torch.as_tensor(x_train).detach().to(torch.float32)
        y = torch.as_tensor(y_train).detach().reshape(-1)
        if self.x.dim() != 2 or self.x.shape[0] != y.shape[0] or self.x.shape[0] < 1 \
                or self.x.shape[1] < 1:
            raise ValueError("x_train must be (N, p) and y_train (N,), N, p >= 1")
        if y.dtype == torch.bool:
            raise ValueError("labels must be integers in [0, classes)")
        if y.is_floating_point():
            if not bool((torch.isfinite(y) & (y == torch.floor(y))).all()):
                raise ValueError("labels must be integers in [0, classes)")
        elif y.is_complex():
            raise ValueError("labels must be integers in [0, classes)")
        y = y.to(device="cpu", dtype=torch.int64)
        if classes is None:
            classes = int(y.max()) + 1
        if isinstance(classes, bool) or int(classes) != classes:
            raise ValueError("classes must be an integer, got %r" % (classes,))
        self.classes = int(classes)
        if not 2 <= self.classes <= self.MAX_CLASSES:
            raise ValueError("classes must be in [2, %d], got %d" % (self.MAX_CLASSES, self.classes))
        if int(y.min()) < 0 or int(y.max()) >= self.classes:
            raise ValueError("labels must lie in [0, %d)" % self.classes)
        if self.d > self.MAX_D:
            raise ValueError("SoftmaxRegression supports d = 1 + C p <= %d, got %d"
                             % (self.MAX_D, self.d))
        self.y = y.to(torch.int32)
        self.a0, self.b0 = float(a0), float(b0)
        self._init_batch(batch)
        self._dev = {}

    @property
    def N(self):
        return self.x.shape[0]

    @property
    def p(self):
        return self.x.shape[1]

    @property
    def C(self):
        return self.classes

    @property
    def d(self):
        return 1 + self.classes * self.x.shape[1]

    def unpack(self, x):
        """(log alpha, W (C, p)) views of a particle."""
        return x[0], x[1:].reshape(self.classes, self.p)

    def logp(self, x):
        if x.shape[-1] != self.d:
            raise ValueError("SoftmaxRegression target has d = 1 + C p = %d" % self.d)
        xd = self.x.to(device=x.device, dtype=x.dtype)
        y = self.y.to(device=x.device, dtype=torch.int64)
        la, W = self.unpack(x)
        z = xd @ W.T
        lik = (torch.gather(z, 1, y[:, None])[:, 0] - torch.logsumexp(z, 1)).sum()
        alpha = torch.exp(la)
        return (lik + 0.5 * (self.d - 1) * la - 0.5 * alpha * (W * W).sum()
                + self.a0 * la - self.b0 * alpha)

    def _params(self, dev):
        if dev not in self._dev:
            self._dev[dev] = (self.x.to(dev).contiguous(), self.y.to(dev).contiguous())
        return self._dev[dev]

    def fingerprint(self):
        """Digest of the data and the model (C, a0, b0, and the batch of a
        minibatch target)."""
        import hashlib
        import struct
        h = hashlib.sha1(b"softmax")
        h.update(struct.pack("<qqqdd", self.N, self.p, self.classes, self.a0, self.b0))
        if self.batch is not None:
            h.update(struct.pack("<q", self.batch))
        h.update(_host_bytes(self.x))
        h.update(_host_bytes(self.y))
        return h.hexdigest()

    def score(self, X, out, scale=1.0, form=None):
        """out = scale * grad log p(X).  form="rows" takes the
        workgroup-per-particle kernel whatever n is (scripts/softmax_timing.py)."""
        n, d = X.shape
        assert d == self.d, "SoftmaxRegression target has d = 1 + C p = %d" % self.d
        if form not in (None, "rows"):
            raise ValueError("form must be None or 'rows'")
        xd, y = self._params(X.device)
        head = (N.ptr(X), N.ld(X), n, d, N.ptr(xd), N.ld(xd), N.ptr(y), self.N, self.classes,
                self.p, self.a0, self.b0, float(scale))
        tail = (N.ptr(out), N.ld(out), N.stream(X.device))
        if self.batch is not None:
            cur = N.ptr(self._window(X.device))
            N.call("dsvgd_score_softmax_rows" if form else "dsvgd_score_softmax_window",
                   *head, cur, self.batch, *tail)
        elif form:
            N.call("dsvgd_score_softmax_rows", *head, None, self.N, *tail)
        else:
            N.call("dsvgd_score_softmax", *head, *tail)


class CallableTarget(Target):
    """Any reference-style `logp(x[d]) -> 0-d tensor`, batched with torch.func.

    The callable must accept tensors on the particles' device; dsvgd does not
    move user code or data to the host.
    """

    def __init__(self, logp, chunk=65536):
        self._logp = logp
        self.chunk = chunk
        self._vg = None

    def logp(self, x):
        return self._logp(x)

    def score(self, X, out, scale=1.0):
        if self._vg is None:
            self._vg = torch.func.vmap(torch.func.grad(self._logp))
        try:
            for s in range(0, X.shape[0], self.chunk):
                g = self._vg(X[s:s + self.chunk])
                out[s:s + self.chunk].copy_(g.reshape(out[s:s + self.chunk].shape)).mul_(scale)
        except RuntimeError as e:
            if "device" in str(e) or "vmap" in str(e).lower() or "batch" in str(e).lower():
                self._score_loop(X, out, scale, e)
            else:
                raise

    def _score_loop(self, X, out, scale, why):
        """Per-particle autograd on the device (callables vmap cannot batch)."""
        for j in range(X.shape[0]):
            x = X[j].detach().clone().requires_grad_(True)
            try:
                lp = self._logp(x)
            except RuntimeError as e:
                raise RuntimeError(
                    "logp could not be evaluated on %s tensors (%s); dsvgd runs scores on the "
                    "particles' device -- use a dsvgd.targets class or a device-agnostic logp"
                    % (X.device, e)) from why
            (g,) = torch.autograd.grad(lp, x)
            out[j] = scale * g


def resolve_target(logp):
    if isinstance(logp, Target):
        return logp
    if not callable(logp):
        raise ValueError("logp must be callable")
    return CallableTarget(logp)
