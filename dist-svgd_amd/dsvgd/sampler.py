"""Drop-in `dsvgd.Sampler` (reference: dsvgd/sampler.py:6-74) on MI355X.

Same constructor and `sample(n, num_iter, step_size) -> pandas.DataFrame`
(columns timestep, particle, value; n*(num_iter+1) rows ordered by
(timestep, particle); value = float32 ndarray (d,)), same particle init from
torch's global CPU generator, same "Iteration l" / mean prints.

Extensions (keyword-only, defaults keep the reference behaviour):
  order="sequential"  the reference's in-place Gauss-Seidel sweep
                      (sampler.py:64-68), one gfx950 row kernel per particle;
  order="jacobi"      all particles move together from the frozen set -- the
                      MFMA fast path (sq-distances, radix-select median, fused
                      exp, K.[X|S]) used for throughput;
  device              HIP device (default: current cuda device);
  verbose             the reference's per-iteration prints;
  graphs              capture one iteration as a HIP graph and replay it
                      (built-in targets; default on);
  ksd_every           record the kernelized Stein discrepancy every k-th
                      timestep into `sampler.diagnostics` (default off);
  adagrad             None (fixed steps), True or a dsvgd.AdaGrad: Liu &
                      Wang's AdaGrad-conditioned steps (order="jacobi");
  project             None or a dsvgd.Projection: projected SVGD, the particles
                      interact in an r-dimensional subspace (order="jacobi").
A target with minibatches (targets.BayesianNN(batch=...) or
targets.LogisticRegression(batch=...)) is scored on window t of its data at
iteration t, in both orders.
The kernel must be RBF- or IMQ-shaped (see dsvgd.kernels); RBF("median") /
IMQ("median") select the median-heuristic bandwidth h = median(D)/log(n),
recomputed every iteration.
"""
import numpy as np
import pandas as pd
import torch
from torch.distributions.normal import Normal

from . import _native as N
from .adagrad import resolve_adagrad
from .engine import AdaGradState, PhiEngine, SelectState, StepGraph, sequential_sweep
from .kernels import resolve_kernel
from .projection import Projection
from .targets import BuiltinTarget, resolve_target


class Sampler(object):
    def __init__(self, d, logp, kernel):
        """Initializes a SVGD sampler.

        Params:
            d - dimensionality of each particle
            kernel - kernel function (RBF or IMQ family; see dsvgd.kernels)
            logp - log density function, or a dsvgd.targets.Target
        """
        self._d = d
        self._logp = logp
        self._kernel = kernel
        self._target = resolve_target(logp)
        self._rbf = resolve_kernel(kernel, d)
        self.diagnostics = None   # sample(ksd_every=k) leaves its KSD records here

    def sample(self, n, num_iter, step_size, *, order="sequential", device=None, verbose=True,
               graphs=True, ksd_every=None, adagrad=None, project=None):
        """Generate samples using SVGD (sampler.py:42-74).

        adagrad=True or a dsvgd.AdaGrad moves the particles by the AdaGrad
        rule, x += step_size * p / (eps + sqrt(G)), with G the moving average
        of p^2 per entry, started afresh by every call (order="jacobi" only:
        the sequential sweeps move their rows inside the kernels).

        ksd_every=k records the kernelized Stein discrepancy of the particles
        at timesteps 0, k, 2k, .. <= num_iter, with the bandwidth the sampler
        used there, into `self.diagnostics` (a DataFrame: timestep, ksd,
        ksd2_v, ksd2_u, h; ksd = sqrt(max(ksd2_v, 0))), read back once after
        the loop.  The returned particles do not change by a bit.

        project=dsvgd.Projection(rank=r) or (basis=Psi): projected SVGD
        (dsvgd.projection; order="jacobi", fixed steps).  The SVGD direction
        is that of the particles' r coordinates in the subspace, with this
        sampler's kernel and bandwidth rule there (the median is that of the
        projected distances), lifted back; the orthogonal complement stays
        where it was drawn.  A learned basis is refreshed eagerly, between the
        (captured) iterations, from the scores of the current particles; the
        Projection carries basis, eigenvalues, captured and refreshes
        afterwards.  ksd_every still measures in the full d dimensions, on an
        engine of its own with its own bandwidth there."""
        if order not in ("sequential", "jacobi"):
            raise ValueError("order must be 'sequential' or 'jacobi'")
        if ksd_every is not None:
            if isinstance(ksd_every, bool) or int(ksd_every) != ksd_every or ksd_every <= 0:
                raise ValueError("ksd_every must be a positive integer (or None)")
            ksd_every = int(ksd_every)
        rule = resolve_adagrad(adagrad)
        if rule is not None and order != "jacobi":
            raise ValueError("adagrad needs order='jacobi': the sequential sweeps move their "
                             "rows inside the sweep kernels, which take fixed steps")
        if project is not None:
            if not isinstance(project, Projection):
                raise ValueError("project must be None or a dsvgd.Projection, got %r" % (project,))
            if order != "jacobi":
                raise ValueError("project needs order='jacobi': the subspace step moves all "
                                 "particles together")
            if rule is not None:
                raise ValueError("project refuses adagrad: a per-entry history has no meaning "
                                 "in coordinates that rotate with the basis")
            project.check(self._d)
        self.diagnostics = None
        dev = N.require_gpu(device if device is not None else "cuda")
        q = Normal(0, 1)
        make_sample = lambda: q.sample((self._d, 1))  # noqa: E731  (sampler.py:58-60)
        particles = torch.cat([make_sample() for _ in range(n)], dim=1).t()
        X = torch.empty(n, self._d, dtype=torch.float32, device=dev)
        X.copy_(particles)
        d = self._d
        hist = torch.empty(num_iter + 1, n, d, dtype=torch.float32, device=dev)
        S = torch.empty(n, d, dtype=torch.float32, device=dev)
        median = self._rbf.median
        # (ksd() reads K . Xc, which only the two-operand phi_mm leaves behind)
        form = "w" if ksd_every is None else "xs"
        # (a projected run interacts on its own r-wide engine)
        peng = project.begin(n, d, self._rbf, dev) if project is not None else None
        engine = (PhiEngine(n, d, device=dev, phi_form=form, kernel=self._rbf)
                  if ((order == "jacobi" or median) and peng is None) else None)
        state = (peng.engine.state if peng is not None
                 else engine.state if engine is not None else SelectState(dev))
        if not median:
            N.call("dsvgd_set_bandwidth", state.ptr, float(self._rbf.h), N.stream(dev))
        target = self._target
        hold = {}    # the sweep's workspace, alive while `step` replays through it
        # the AdaGrad history starts afresh with every run, and so does a
        # minibatch target's window: two runs from the same seed agree
        ada = (rule, AdaGradState(n, d, dev)) if rule is not None else None
        target.reset_batch()

        def iteration():
            target.score(X, S)
            if peng is not None:
                peng.step(X, S, step_size, h=None if median else self._rbf.h)
            elif order == "jacobi":
                if ada is not None:
                    engine.step(X, S, X_own=X, step=step_size,
                                h=None if median else self._rbf.h, adagrad=ada)
                else:
                    engine.step(X, S, X_own=X, step=step_size,
                                h=None if median else self._rbf.h, write_phi=False)
            else:
                if median:
                    engine.pack(X)
                    engine.distances(median=True)
                    engine.median_bandwidth()
                sequential_sweep(X, S, range(n), state, step_size, target=target, hold=hold,
                                 kernel=self._rbf)
            target.next_batch()     # (after the iteration's last score call)

        # built-in targets are pure kernel launches: capture the iteration
        # once and replay it (user callables run eagerly)
        step = StepGraph(iteration, dev, enabled=graphs and isinstance(target, BuiltinTarget))
        # KSD records: the Jacobi MFMA step leaves everything ksd() needs
        # (the launches follow the step, graph replay or not, on the stream);
        # otherwise a full evaluation on an engine and scores of its own, so
        # the sampler's buffers and the trajectory are untouched
        records = list(range(0, num_iter + 1, ksd_every)) if ksd_every else []
        if records:
            kout = torch.empty(len(records), 4, dtype=torch.float64, device=dev)
            kh = torch.empty(len(records), dtype=torch.float32, device=dev)
            fused = order == "jacobi" and d > PhiEngine.DIRECT_MAX_D and peng is None
            keng = engine if fused else PhiEngine(n, d, device=dev, kernel=self._rbf)
            Sk = S if fused else torch.empty_like(S)
            h_fixed = None if median else self._rbf.h

        def record(l, evaluate):
            if evaluate:   # (the fused path: the step just ran on these particles)
                target.score(X, Sk)
                keng.step(X, Sk, step=0.0, h=h_fixed, write_phi=False)
            k = l // ksd_every
            keng.ksd(out=kout[k])
            kh[k:k + 1].copy_(keng.state.bandwidth)

        for l in range(num_iter):
            if verbose:
                print('Iteration {}'.format(l))
            hist[l].copy_(X)
            rec = bool(records) and l % ksd_every == 0
            if rec and not fused:
                record(l, True)
            if peng is not None and project.due(l):
                target.score(X, S)      # (the iteration's own window; it moves after the step)
                project.refresh(peng, X, S, l)
            step()
            if rec and fused:
                record(l, False)
            if verbose:
                print(X.mean(dim=0).cpu())
        hist[num_iter].copy_(X)
        if records and num_iter % ksd_every == 0:
            record(num_iter, True)   # no step follows the last timestep: step 0
        if records:
            kv, hv = kout.cpu().numpy(), kh.cpu().numpy()
            self.diagnostics = pd.DataFrame({
                "timestep": records, "ksd": np.sqrt(np.maximum(kv[:, 2], 0.0)),
                "ksd2_v": kv[:, 2], "ksd2_u": kv[:, 3], "h": hv})
        vals = hist.cpu().numpy().reshape(-1, d)
        steps = torch.arange(num_iter + 1).repeat_interleave(n).numpy()
        ids = torch.arange(n).repeat(num_iter + 1).numpy()
        return pd.DataFrame({"timestep": steps, "particle": ids, "value": list(vals)})
