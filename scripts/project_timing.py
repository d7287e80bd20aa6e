"""Time projected SVGD (dsvgd.projection) at the headline shapes, n = 65536
with (d, r) = (256, 16) and (1024, 32): the three kernels of csrc/project.hip
(Gram, apply, lift), the refresh's device-to-host copy of H plus the host
eigh, one projected step and one full-width step, all in the same process with
HIP events (the host part with a host clock around work that ends in a
synchronise), after a warm-up, the variants alternating inside one loop.  A
sample of a kernel is `--batch` back-to-back launches between one pair of
events, divided by their number, so that the events' and the launches' own
overhead does not count as kernel time; a step is timed one at a time.

    python scripts/project_timing.py [--n N] [--shapes D:R,D:R] [--reps R] [--warmup W]
                                     [--batch K] [--timeout SECONDS] [--json PATH]

The measuring process is a child started under `timeout` (a hang ends there,
and nothing further is started on the device).  Reported: median and minimum
over the repeats, the bytes each kernel has to move over its median time, and
`every` = the refresh interval at which a refresh costs a tenth of the
projected steps between two of them.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dist-svgd_amd"))


def measure_shape(n, d, r, reps, warmup, batch, dev):
    import torch

    import dsvgd
    from dsvgd.projection import ProjectedEngine, leading_basis
    g = torch.Generator(device="cpu").manual_seed(0)
    X = torch.randn(n, d, generator=g).to(dev)
    mu, lam = 2.0 * torch.randn(d, generator=g), torch.rand(d, generator=g) * 1.5 + 0.5
    S = torch.empty_like(X)
    dsvgd.targets.Gaussian(mu, lam).score(X, S)
    peng = ProjectedEngine(n, d, r, device=dev, kernel=dsvgd.RBF("median"))
    peng.refresh(X, S)
    full = dsvgd.PhiEngine(n, d, device=dev, phi_form="w")
    Xw = X.clone()
    peng.project(X, S)
    peng.engine.step(peng.Xr, peng.Sr, step=0.0, h=None, write_phi=True)

    def refresh_host():
        H = peng.H.cpu()                      # synchronises
        Psi, _ = leading_basis(H, r)
        peng.set_basis(Psi)

    device_runs = {
        "gram": lambda: peng.gram(X, S),
        "apply": lambda: peng.project(X, S),
        "lift": lambda: peng.lift(0.0, phi_out=Xw),      # writes n x d, X is not read
        "lift_step": lambda: peng.lift(1e-9, X=Xw),      # reads and writes X
        "projected_step": lambda: peng.step(Xw, S, 1e-9, h=None),
        "full_step": lambda: full.step(X, S, X_own=Xw, step=0.0, write_phi=False),
    }
    launches = {k: (1 if k.endswith("_step") and k != "lift_step" else batch)
                for k in device_runs}
    ms = {k: [] for k in device_runs}
    ms["d2h_eigh"] = []
    for it in range(warmup + reps):
        for name, fn in device_runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches[name]):
                fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                ms[name].append(e0.elapsed_time(e1) / launches[name])
        peng.gram(X, S)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        refresh_host()
        torch.cuda.synchronize(dev)
        if it >= warmup:
            ms["d2h_eigh"].append(1e3 * (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in ms.items()}
    # the bytes each kernel has to move, from the shapes
    need = {"gram": 4 * (2 * n * d + d * d), "apply": 4 * (2 * n * d + d * r + 2 * n * r),
            "lift": 4 * (n * r + d * r + n * d), "lift_step": 4 * (n * r + d * r + 2 * n * d)}
    flops = {"gram": n * d * d, "apply": 4 * n * d * r, "lift": 2 * n * d * r,
             "lift_step": 2 * n * d * r}       # (the Gram's upper half: n d^2 / 2 MACs)
    refresh = med["gram"] + med["d2h_eigh"]
    return {"n": n, "d": d, "r": r, "gram_slices": peng.slices, "launches_per_sample": launches,
            "ms_median": {k: round(v, 4) for k, v in med.items()},
            "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
            "tb_per_s": {k: round(need[k] / med[k] * 1e-9, 3) for k in need},
            "tflop_per_s": {k: round(flops[k] / med[k] * 1e-9, 2) for k in flops},
            "refresh_ms": round(refresh, 3),
            "projected_over_full_step": round(med["projected_step"] / med["full_step"], 4),
            "every_for_a_tenth": int(-(-refresh // (0.1 * med["projected_step"])))}


def measure(a):
    import torch

    from dsvgd import _native as N
    dev = N.require_gpu("cuda:0")
    res = {"reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev),
           "shapes": []}
    for item in a.shapes.split(","):
        d, r = (int(v) for v in item.split(":"))
        res["shapes"].append(measure_shape(a.n, d, r, a.reps, a.warmup, a.batch, dev))
        print(json.dumps(res["shapes"][-1]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--shapes", default="256:16,1024:32")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=20,
                    help="back-to-back launches of a kernel per timed sample")
    ap.add_argument("--timeout", type=int, default=400)
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
        print("project_timing: the measuring process ended with status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
