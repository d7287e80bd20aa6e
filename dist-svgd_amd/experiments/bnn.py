"""Bayesian neural-network regression with dsvgd on MI355X: Liu & Wang's
second SVGD workload (one hidden ReLU layer, Gamma hyper-priors) on the
built-in `dsvgd.targets.BayesianNN` target.  Not part of the reference, whose
experiments stop at logistic regression.

    python experiments/bnn.py --nparticles 512 --niter 300 --stepsize 1e-4 --every 50

Data: a synthetic regression set made from a seed, nothing downloaded:
z ~ N(0, I_p), y = sin(sum_k z_k) + 0.1 noise (p = 8, 1000 rows by default),
split 90 / 10 into train and test.  `dsvgd.Sampler` runs in the Jacobi order
with the median bandwidth from its own N(0, 1) start: plain SVGD steps of a
fixed size over all the data by default, Liu & Wang's AdaGrad steps with
`--adagrad` and minibatches of `--batch` rows (a cyclic window) with `--batch`:

    python experiments/bnn.py --adagrad --stepsize 1e-3 --batch 100

`--project R` runs projected SVGD (dsvgd.Projection): the particles interact
in the R leading directions of the gradient of log(p / N(0, I)), relearned
every `--project-every` iterations; the share of that gradient's second moment
the subspace captures is printed for each refresh:

    python experiments/bnn.py --project 16 --project-every 25

Every `--every` iterations the test
RMSE of the particle-mean prediction and the mean test log-likelihood of the
particle mixture are printed (dsvgd.metrics.bnn_rmse / bnn_loglik, from the
sampler's history), and at the end the kernelized Stein discrepancy of the
final particles (dsvgd.metrics.ksd, on all the data whatever the batch).
"""
import os
import sys

import click
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import dsvgd  # noqa: E402


def synthetic_regression(N=1000, p=8, seed=0, test_fraction=0.1):
    """(x_train, y_train, x_test, y_test), fp32."""
    rs = np.random.RandomState(seed)
    z = rs.randn(N, p).astype(np.float32)
    y = (np.sin(z.sum(1)) + 0.1 * rs.randn(N)).astype(np.float32)
    perm = rs.permutation(N)
    nt = max(1, int(round(test_fraction * N)))
    te, tr = perm[:nt], perm[nt:]
    return z[tr], y[tr], z[te], y[te]


def run(nparticles, niter, stepsize, every, hidden=50, rows=1000, p=8, seed=0, device="cuda:0",
        out=print, adagrad=False, batch=None, project=None, project_every=10):
    """Runs the experiment; returns the recorded curve as a list of dicts
    (iteration, rmse, loglik) and the final KSD.  adagrad: True or a
    dsvgd.AdaGrad for AdaGrad steps; batch: rows per minibatch (None: all);
    project: the rank of projected SVGD (None: plain SVGD), its basis
    relearned every project_every iterations."""
    x_train, y_train, x_test, y_test = synthetic_regression(rows, p, seed)
    target = dsvgd.targets.BayesianNN(x_train, y_train, hidden=hidden, batch=batch)
    d = target.d
    torch.manual_seed(seed)
    sampler = dsvgd.Sampler(d, target, dsvgd.RBF("median"))
    proj = dsvgd.Projection(rank=project, every=project_every) if project else None
    df = sampler.sample(nparticles, niter, stepsize, order="jacobi", device=device, verbose=False,
                        adagrad=adagrad or None, project=proj)
    if proj is not None:
        for it, captured in proj.captured_history:
            out("iteration %5d  basis refresh: rank %d captured %.4f" % (it, proj.rank, captured))
    hist = np.stack(df["value"].to_list()).reshape(niter + 1, nparticles, d)
    curve = []
    for it in sorted(set(range(0, niter + 1, every)) | {niter}):
        P = torch.as_tensor(hist[it], dtype=torch.float32, device=device)
        row = {"iteration": it,
               "rmse": dsvgd.metrics.bnn_rmse(P, target, x_test, y_test),
               "loglik": dsvgd.metrics.bnn_loglik(P, target, x_test, y_test)}
        curve.append(row)
        out("iteration %5d  test rmse %.4f  test loglik %.4f" % (it, row["rmse"], row["loglik"]))
    ksd = dsvgd.metrics.ksd(hist[niter], target.full, dsvgd.RBF("median"), device=device)
    out("final ksd %.6g" % ksd)
    return curve, ksd


@click.command()
@click.option('--nparticles', type=int, default=512)
@click.option('--niter', type=int, default=300)
@click.option('--stepsize', type=float, default=1e-4)
@click.option('--every', type=int, default=50, help='print the test metrics every k iterations')
@click.option('--hidden', type=int, default=50)
@click.option('--rows', type=int, default=1000, help='rows of the synthetic set (train + test)')
@click.option('--features', type=int, default=8)
@click.option('--seed', type=int, default=0)
@click.option('--adagrad/--no-adagrad', default=False,
              help="AdaGrad-conditioned steps (Liu & Wang's rule)")
@click.option('--batch', type=int, default=None,
              help='rows per minibatch (a cyclic window; default: all the data)')
@click.option('--project', type=int, default=None,
              help='projected SVGD in a learned subspace of this rank (default: plain SVGD)')
@click.option('--project-every', type=int, default=10,
              help='relearn the subspace every k iterations')
def cli(nparticles, niter, stepsize, every, hidden, rows, features, seed, adagrad, batch, project,
        project_every):
    run(nparticles, niter, stepsize, every, hidden, rows, features, seed, adagrad=adagrad,
        batch=batch, project=project, project_every=project_every)


if __name__ == "__main__":
    cli()
