"""Generate the inverse multiquadric (IMQ) fixtures tests/golden/imq_*.npz by
RUNNING THE REFERENCE with IMQ lambdas (the reference takes any kernel(x, y)
callable and differentiates it by autograd, dsvgd/sampler.py:19-40).

Like make_golden.py, whose targets, particle init and reference import it
reuses, this script runs in the build container only; the fixtures hold plain
numpy arrays (inputs + the reference's outputs).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_imq.py

Cases: three phi evaluations on frozen particles (Sampler._phi_hat) and one
Sampler.sample trajectory in the reference's sequential (Gauss-Seidel) order.
"""
import contextlib
import io
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as G  # noqa: E402


def imq(h=1.0, beta=-0.5):
    import torch

    def kernel(x, y):
        return (1. + torch.dist(x, y, p=2) ** 2 / h) ** beta
    return kernel


def phi_case(name, X, logp, h, beta, extra):
    dsvgd = G._ref()
    import torch
    s = dsvgd.Sampler(X.shape[1], logp, imq(h, beta))
    Xt = torch.tensor(X, dtype=torch.float32)
    phi = torch.stack([s._phi_hat(Xt[i], Xt) for i in range(Xt.shape[0])]).numpy()
    np.savez(os.path.join(OUT, name + ".npz"), X=X.astype(np.float32), phi=phi,
             h=np.float64(h), beta=np.float64(beta), **extra)
    print(name, X.shape, "max|phi|", np.abs(phi).max())


def sample_case(name, d, n, T, eps, logp, h, beta, seed, extra):
    dsvgd = G._ref()
    import torch
    torch.manual_seed(seed)
    s = dsvgd.Sampler(d, logp, imq(h, beta))
    with contextlib.redirect_stdout(io.StringIO()):
        df = s.sample(n, T, eps)
    vals = np.stack(df["value"].to_list()).reshape(T + 1, n, d)
    np.savez(os.path.join(OUT, name + ".npz"), values=vals,
             timestep=df["timestep"].to_numpy(), particle=df["particle"].to_numpy(),
             seed=np.int64(seed), n=np.int64(n), d=np.int64(d), T=np.int64(T),
             eps=np.float64(eps), h=np.float64(h), beta=np.float64(beta), **extra)
    print(name, vals.shape)


def main():
    import torch
    torch.set_num_threads(1)
    # phi on frozen particles (sampler.py:35-40)
    X = G.ref_init(48, 5, 21).numpy()
    mu = np.random.RandomState(5).randn(5).astype(np.float32)
    lam = np.random.RandomState(6).uniform(0.5, 2.0, 5).astype(np.float32)
    phi_case("imq_gauss_n48_d5_h1p7", X, G.gauss_logp(mu, lam), 1.7, -0.5,
             {"target": np.array("gaussian"), "mu": mu, "lam": lam})
    phi_case("imq_gmm_n40", G.ref_init(40, 1, 42).numpy(), G.gmm_logp(), 1.0, -0.5,
             {"target": np.array("gmm")})
    x, t = G.banana_like(N=400)
    phi_case("imq_logreg_n60", G.ref_init(60, 3, 0).numpy(), G.logreg_logp(x, t), 1.0, -0.75,
             {"target": np.array("logreg"), "x_train": x, "t_train": t})
    # Sampler.sample, the Gauss-Seidel trajectory (sampler.py:42-74)
    mu = np.array([0.5, -1.0, 0.25], np.float32)
    lam = np.array([1.0, 2.0, 0.5], np.float32)
    sample_case("imq_sample_gauss_n16_d3", 3, 16, 3, 0.1, G.gauss_logp(mu, lam), 1.0, -0.5, 42,
                {"target": np.array("gaussian"), "mu": mu, "lam": lam})


if __name__ == "__main__":
    main()
