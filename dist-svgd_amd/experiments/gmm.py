"""The multimodal toy with dsvgd on MI355X: SVGD on a Gaussian mixture, the
counterpart of the reference's experiments/gmm.py on the GPU sampler and the
built-in `dsvgd.targets.GaussianMixture` target.

    python experiments/gmm.py
    python experiments/gmm.py --d 16 --modes 5 --spread 6 --nparticles 4096 --kernel imq

The defaults are the reference's run: d = 1, two unit-variance modes at -2 and
+2 with equal weights, 50 particles from N(0, 1), 500 iterations of step 1.0
with the kernel exp(-|x - y|^2), in the sequential order.  Other mixtures come
from a seed: `--modes` K unit-variance components in `--d` dimensions, their
means `--spread` times N(0, I) draws (K = 2: -spread and +spread along the
first axis), with equal weights.

Every `--every` iterations the mode shares of the particles (the fraction
whose most responsible component is k, dsvgd.metrics.mode_shares) are printed
beside the weights, with the mean log density (dsvgd.metrics.gmix_logp); at
the end the kernelized Stein discrepancy of the final particles
(dsvgd.metrics.ksd).  With `--mmd M` the particles are also compared with M
exact draws of the mixture (drawn once, GaussianMixture.sample): every printed
iteration gains the maximum mean discrepancy to them (dsvgd.metrics.mmd, the
unbiased statistic at the pooled-median bandwidth), which -- unlike the
score-based KSD -- sees wrong mode shares; the final one is printed before the
final KSD.  No plots.
"""
import os
import sys

import click
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import dsvgd  # noqa: E402


def mixture(d=1, modes=2, spread=2.0, seed=0):
    """(means (K, d), precisions (K, d), weights (K,)), fp32: the seeded
    problem."""
    if d < 1 or modes < 1:
        raise ValueError("d and modes must be >= 1")
    if modes == 2:
        means = np.zeros((2, d), np.float32)
        means[0, 0], means[1, 0] = -spread, spread
    else:
        means = (spread * np.random.RandomState(seed).randn(modes, d)).astype(np.float32)
    return means, np.ones((modes, d), np.float32), np.full(modes, 1.0 / modes, np.float32)


def make_kernel(name):
    if name == "rbf":
        return dsvgd.RBF(1.0)
    if name == "imq":
        return dsvgd.IMQ(1.0, -0.5)
    raise ValueError("kernel must be 'rbf' or 'imq'")


def _shares(v):
    return "[" + " ".join("%.3f" % s for s in v) + "]"


def run(nparticles=50, niter=500, stepsize=1.0, every=100, d=1, modes=2, spread=2.0,
        order="sequential", kernel="rbf", seed=42, device="cuda:0", out=print, mmd=0):
    """Runs the experiment; returns the recorded curve as a list of dicts
    (iteration, shares, logp -- and mmd, against `mmd` exact draws, if mmd >
    0) and the final KSD."""
    if mmd < 0:
        raise ValueError("mmd must be >= 0 (the number of exact draws; 0: off)")
    means, precisions, weights = mixture(d, modes, spread, seed)
    target = dsvgd.targets.GaussianMixture(means, precisions, weights)
    kern = make_kernel(kernel)
    torch.manual_seed(seed)
    sampler = dsvgd.Sampler(d, target, kern)
    df = sampler.sample(nparticles, niter, stepsize, order=order, device=device, verbose=False)
    hist = np.stack(df["value"].to_list()).reshape(niter + 1, nparticles, d)
    out("weights %s" % _shares(target.weights.tolist()))
    exact = target.sample(mmd, seed=seed, device=device) if mmd > 0 else None
    curve = []
    for it in sorted(set(range(0, niter + 1, every)) | {niter}):
        P = torch.as_tensor(hist[it], dtype=torch.float32, device=device)
        row = {"iteration": it,
               "shares": dsvgd.metrics.mode_shares(P, target).cpu().tolist(),
               "logp": float(dsvgd.metrics.gmix_logp(P, target).double().mean())}
        curve.append(row)
        line = "iteration %5d  shares %s  mean logp %.4f" % (it, _shares(row["shares"]), row["logp"])
        if exact is not None:
            row["mmd"] = dsvgd.metrics.mmd(P, exact, device=device)
            line += "  mmd %.6g" % row["mmd"]
        out(line)
    if exact is not None:
        out("final mmd %.6g" % curve[-1]["mmd"])
    ksd = dsvgd.metrics.ksd(hist[niter], target, kern, device=device)
    out("final ksd %.6g" % ksd)
    return curve, ksd


@click.command()
@click.option('--d', type=int, default=1, help='dimension')
@click.option('--modes', type=int, default=2, help='number of components')
@click.option('--spread', type=float, default=2.0, help='scale of the means')
@click.option('--nparticles', type=int, default=50)
@click.option('--niter', type=int, default=500)
@click.option('--stepsize', type=float, default=1.0)
@click.option('--order', type=click.Choice(['sequential', 'jacobi']), default='sequential')
@click.option('--kernel', type=click.Choice(['rbf', 'imq']), default='rbf')
@click.option('--every', type=int, default=100, help='print the diagnostics every k iterations')
@click.option('--seed', type=int, default=42)
@click.option('--mmd', type=int, default=0,
              help='compare with this many exact draws of the mixture (0: off)')
def cli(d, modes, spread, nparticles, niter, stepsize, order, kernel, every, seed, mmd):
    run(nparticles, niter, stepsize, every, d, modes, spread, order, kernel, seed, mmd=mmd)


if __name__ == "__main__":
    cli()
