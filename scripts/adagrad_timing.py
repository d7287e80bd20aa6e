"""Time one Jacobi step with and without the AdaGrad rule at the bench
configuration (n = 65536, d = 256, median bandwidth, the one-operand phi_mm
the samplers use) in the same process, and the update kernel alone, with HIP
events.

    python scripts/adagrad_timing.py [--n N] [--d D] [--reps R] [--warmup W]
                                     [--timeout SECONDS] [--json PATH]

The measuring process is a child started under `timeout` (a hang ends there,
and nothing further is started on the device); the two steps alternate inside
one loop on one engine, so both see the same machine state.  The plain step
is the samplers' (the finish kernel moves the particles and writes no phi);
the AdaGrad step's finish writes phi without moving anything and
dsvgd_adagrad_step follows (it reads x, phi and G and writes x and G: about
5 m d 4 bytes).  Both run with step size 0, so the particles stay where they
are.  Reported: median and minimum over the repeats, and the difference of
the medians in ms and as a share of the plain step.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dist-svgd_amd"))


def measure(a):
    import torch

    import dsvgd
    from dsvgd import _native as N
    from dsvgd.engine import AdaGradState, StageTimer
    dev = N.require_gpu("cuda:0")
    n, d = a.n, a.d
    g = torch.Generator(device="cpu").manual_seed(0)
    X = torch.randn(n, d, generator=g).to(dev)
    mu, lam = torch.randn(d, generator=g), torch.rand(d, generator=g) * 1.5 + 0.5
    S = torch.empty_like(X)
    dsvgd.targets.Gaussian(mu, lam).score(X, S)
    eng = dsvgd.PhiEngine(n, d, device=dev, phi_form="w")
    ada = (dsvgd.AdaGrad(), AdaGradState(n, d, dev))
    Xw = X.clone()
    steps = {"plain": lambda: eng.step(X, S, X_own=Xw, step=0.0, write_phi=False),
             "adagrad": lambda: eng.step(X, S, X_own=Xw, step=0.0, adagrad=ada)}
    ms = {k: [] for k in steps}
    for it in range(a.warmup + a.reps):
        for name, fn in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    # the update kernel, in a loop of its own (every timed span is a pair of
    # stream markers the device waits on)
    eng.timer = StageTimer(only=("adagrad",))
    for it in range(a.reps):
        steps["adagrad"]()
    kern = eng.timer.summary()["adagrad"]
    eng.timer = None
    med = {k: statistics.median(v) for k, v in ms.items()}
    diff = med["adagrad"] - med["plain"]
    res = {"n": n, "d": d, "reps": a.reps, "phi_form": eng.phi_form,
           "range_guard": eng.range_guard(),
           "step_ms_median": {k: round(v, 4) for k, v in med.items()},
           "step_ms_min": {k: round(min(v), 4) for k, v in ms.items()},
           "adagrad_minus_plain_ms": round(diff, 4),
           "adagrad_minus_plain_share": round(diff / med["plain"], 5),
           "update_kernel_ms_median": round(statistics.median(kern), 4),
           "update_kernel_ms_min": round(min(kern), 4),
           "update_kernel_bytes": 5 * n * d * 4,
           "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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
        print("adagrad_timing: the measuring process ended with status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
