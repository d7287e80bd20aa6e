"""Time one Jacobi step with the inverse multiquadric (IMQ) kernel at the bench
configuration (n = 65536, d = 256, median bandwidth) beside the RBF
two-operand step (phi_form="xs") in the same process: the whole step and its
phi_mm launches (IMQ: two, F = u^beta and G' = u^(beta-1); RBF: one), with HIP
events, and the IMQ phi's error against fp64 on sampled rows of that run.

    python scripts/imq_timing.py [--n N] [--d D] [--beta B] [--reps R] [--warmup W]
                                 [--rows K] [--timeout SECONDS] [--json PATH]

The measuring process is a child started under `timeout` (a hang ends there,
and nothing further is started on the device); the IMQ and the RBF steps
alternate inside one loop, so both see the same machine state.  Reported:
median and minimum over the repeats and the ratios of the medians.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dist-svgd_amd"))


def phi_rows_fp64(X, S, h, beta, rows):
    """phi of `rows` pair by pair in fp64 (the reference's own sum)."""
    import numpy as np
    n = X.shape[0]
    c1 = -2.0 * beta / h
    out = np.empty((len(rows), X.shape[1]))
    for k, i in enumerate(rows):
        diff = X[i] - X
        lg = np.log1p((diff ** 2).sum(1) / h)
        F, G = np.exp(beta * lg), np.exp((beta - 1.0) * lg)
        out[k] = (F @ S + c1 * (G @ diff)) / n
    return out


def measure(a):
    import numpy as np
    import torch

    import dsvgd
    from dsvgd import _native as N
    from dsvgd.engine import StageTimer
    dev = N.require_gpu("cuda:0")
    n, d = a.n, a.d
    g = torch.Generator(device="cpu").manual_seed(0)
    Xc = torch.randn(n, d, generator=g)
    X = Xc.to(dev)
    mu, lam = torch.randn(d, generator=g), torch.rand(d, generator=g) * 1.5 + 0.5
    S = torch.empty_like(X)
    dsvgd.targets.Gaussian(mu, lam).score(X, S)
    engines = {"imq": dsvgd.PhiEngine(n, d, device=dev, kernel=dsvgd.IMQ("median", a.beta)),
               "rbf_xs": dsvgd.PhiEngine(n, d, device=dev, phi_form="xs")}
    launches = {"imq": ("phi_mm_f", "phi_mm_g"), "rbf_xs": ("phi_mm",)}
    Xw = X.clone()

    def step(eng):       # step 0: X_own is rewritten with the same values
        eng.step(X, S, X_own=Xw, step=0.0, write_phi=True)

    ms = {k: [] for k in engines}
    for it in range(a.warmup + a.reps):
        for name, eng in engines.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(eng)
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    # the launches, in a loop of their own (every timed span is a pair of
    # stream markers the device waits on)
    lms = {}
    for name, eng in engines.items():
        eng.timer = StageTimer(only=launches[name])
    for it in range(a.reps):
        for eng in engines.values():
            step(eng)
    for name, eng in engines.items():
        for k, v in eng.timer.summary().items():
            lms[name + "." + k] = v
        eng.timer = None
    # the IMQ phi against fp64 on sampled rows of this run
    eng = engines["imq"]
    h = eng.state.read()[1]
    rows = np.random.RandomState(1).choice(n, a.rows, replace=False)
    rows.sort()
    got = eng.phi[torch.as_tensor(rows, device=dev)].cpu().numpy().astype(np.float64)
    ref = phi_rows_fp64(Xc.numpy().astype(np.float64), S.cpu().numpy().astype(np.float64), h,
                        a.beta, rows)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    med = {k: statistics.median(v) for k, v in ms.items()}
    lmed = {k: statistics.median(v) for k, v in lms.items()}
    res = {"n": n, "d": d, "beta": a.beta, "reps": a.reps, "h": h,
           "sym": int(eng.sym), "splits": int(eng.splits),
           "range_guard": {k: e.range_guard() for k, e in engines.items()},
           "step_ms_median": {k: round(v, 4) for k, v in med.items()},
           "step_ms_min": {k: round(min(v), 4) for k, v in ms.items()},
           "launch_ms_median": {k: round(v, 4) for k, v in lmed.items()},
           "launch_ms_min": {k: round(min(v), 4) for k, v in lms.items()},
           "imq_over_rbf_step": round(med["imq"] / med["rbf_xs"], 3),
           "imq_launches_over_rbf_launch": round(
               (lmed["imq.phi_mm_f"] + lmed["imq.phi_mm_g"]) / lmed["rbf_xs.phi_mm"], 3),
           "imq_phi_err_sampled_rows": err, "sampled_rows": int(a.rows),
           "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--beta", type=float, default=-0.5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        measure(a)
        return 0
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__),
           "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        print("imq_timing: the measuring process ended with status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
