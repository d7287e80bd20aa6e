"""Bayesian softmax (multiclass logistic) regression with dsvgd on MI355X, on
the built-in `dsvgd.targets.SoftmaxRegression` target.  Not part of the
reference, whose experiments stop at two classes.

    python experiments/softmax.py --classes 7 --p 54 --nparticles 512 --niter 300 --every 50
    python experiments/softmax.py --batch 100 --adagrad --stepsize 1e-2 --kernel imq

Data: a synthetic C-class set made from a seed, nothing downloaded: class
means mu_c ~ 2 N(0, I_{p-1}), x = mu_y + N(0, I), a ones column appended (the
model has no bias of its own), 1000 rows by default, split 90 / 10 into train
and test.  `dsvgd.Sampler` runs from its own N(0, 1) start with the median
bandwidth: plain SVGD steps of a fixed size over all the data by default,
AdaGrad steps with `--adagrad`, minibatches of `--batch` rows (a cyclic
window) with `--batch`.

Every `--every` iterations the test accuracy and the mean predictive
log-likelihood of the particle mixture are printed
(dsvgd.metrics.softmax_accuracy / softmax_loglik, from the sampler's history),
and at the end the kernelized Stein discrepancy of the final particles
(dsvgd.metrics.ksd, on all the data whatever the batch).
"""
import os
import sys

import click
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import dsvgd  # noqa: E402


def synthetic_classes(N=1000, p=8, classes=4, seed=0, test_fraction=0.1):
    """(x_train, y_train, x_test, y_test): fp32 rows of p columns (the last
    one ones) and int64 labels."""
    rs = np.random.RandomState(seed)
    mu = 2.0 * rs.randn(classes, p - 1)
    y = rs.randint(0, classes, N)
    x = np.concatenate([mu[y] + rs.randn(N, p - 1), np.ones((N, 1))], 1).astype(np.float32)
    perm = rs.permutation(N)
    nt = max(1, int(round(test_fraction * N)))
    te, tr = perm[:nt], perm[nt:]
    return x[tr], y[tr].astype(np.int64), x[te], y[te].astype(np.int64)


def make_kernel(kernel):
    if kernel == "rbf":
        return dsvgd.RBF("median")
    if kernel == "imq":
        return dsvgd.IMQ("median", -0.5)
    raise ValueError("kernel must be 'rbf' or 'imq'")


def run(nparticles, niter, stepsize, every, classes=4, p=8, rows=1000, seed=0, order="jacobi",
        kernel="rbf", device="cuda:0", out=print, adagrad=False, batch=None):
    """Runs the experiment; returns the recorded curve as a list of dicts
    (iteration, accuracy, loglik) and the final KSD."""
    x_train, y_train, x_test, y_test = synthetic_classes(rows, p, classes, seed)
    target = dsvgd.targets.SoftmaxRegression(x_train, y_train, classes=classes, batch=batch)
    d = target.d
    torch.manual_seed(seed)
    sampler = dsvgd.Sampler(d, target, make_kernel(kernel))
    df = sampler.sample(nparticles, niter, stepsize, order=order, device=device, verbose=False,
                        adagrad=adagrad or None)
    hist = np.stack(df["value"].to_list()).reshape(niter + 1, nparticles, d)
    curve = []
    for it in sorted(set(range(0, niter + 1, every)) | {niter}):
        P = torch.as_tensor(hist[it], dtype=torch.float32, device=device)
        row = {"iteration": it,
               "accuracy": dsvgd.metrics.softmax_accuracy(P, target, x_test, y_test),
               "loglik": dsvgd.metrics.softmax_loglik(P, target, x_test, y_test)}
        curve.append(row)
        out("iteration %5d  test accuracy %.4f  test loglik %.4f"
            % (it, row["accuracy"], row["loglik"]))
    ksd = dsvgd.metrics.ksd(hist[niter], target.full, dsvgd.RBF("median"), device=device)
    out("final ksd %.6g" % ksd)
    return curve, ksd


@click.command()
@click.option('--classes', type=int, default=4)
@click.option('--p', type=int, default=8, help='columns of a data row, the ones column included')
@click.option('--nparticles', type=int, default=512)
@click.option('--niter', type=int, default=300)
@click.option('--stepsize', type=float, default=1e-3)
@click.option('--order', type=click.Choice(['jacobi', 'sequential']), default='jacobi')
@click.option('--kernel', type=click.Choice(['rbf', 'imq']), default='rbf')
@click.option('--batch', type=int, default=None,
              help='rows per minibatch (a cyclic window; default: all the data)')
@click.option('--adagrad/--no-adagrad', default=False,
              help="AdaGrad-conditioned steps (Liu & Wang's rule)")
@click.option('--every', type=int, default=50, help='print the test metrics every k iterations')
@click.option('--rows', type=int, default=1000, help='rows of the synthetic set (train + test)')
@click.option('--seed', type=int, default=0)
def cli(classes, p, nparticles, niter, stepsize, order, kernel, batch, adagrad, every, rows, seed):
    run(nparticles, niter, stepsize, every, classes, p, rows, seed, order, kernel,
        adagrad=adagrad, batch=batch)


if __name__ == "__main__":
    cli()
