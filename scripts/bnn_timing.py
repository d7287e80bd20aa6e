"""Time the Bayesian neural-network score: `BayesianNN.score` (one kernel,
csrc/bnn.hip) beside `CallableTarget(target.logp).score` -- the same model as
a user logp under torch.func.vmap(grad), the path a user had before the
target existed -- on the same device and inputs, with HIP events.

    python scripts/bnn_timing.py [--n N [N ...]] [--rows N] [--p P] [--hidden H]
                                 [--reps R] [--warmup W] [--timeout SECONDS] [--json PATH]

Defaults: n = 4096 and 65536 particles, N = 1024 rows, p = 13, H = 50
(d = 753).  The measuring process is a child started under `timeout` (a hang
ends there, and nothing further is started on the device); the two paths
alternate inside one loop, so both see the same machine state.  Reported per
n: median and minimum over the repeats, the ratio of the medians, the
built-in kernel's executed flop 4 n N p H and its rate, and the largest
difference of the two scores against the fp32 scale of the entries.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dist-svgd_amd"))

# fp32 FMA peak of the vector ALUs: 256 CUs x 4 SIMDs x 32 lanes x 2 flop at 2.4 GHz
VALU_PEAK_FLOPS = 256 * 4 * 32 * 2 * 2.4e9


def measure(a):
    import numpy as np
    import torch

    import dsvgd
    from dsvgd import _native as N
    from dsvgd.targets import BayesianNN, CallableTarget
    dev = N.require_gpu("cuda:0")
    N_, p, H = a.rows, a.p, a.hidden
    rs = np.random.RandomState(0)
    Z = rs.randn(N_, p).astype(np.float32)
    y = (np.sin(Z.sum(1)) + 0.1 * rs.randn(N_)).astype(np.float32)
    target = BayesianNN(Z, y, hidden=H)
    d = target.d
    paths = {"builtin": target, "callable": CallableTarget(target.logp)}
    out = []
    for n in a.n:
        g = torch.Generator(device="cpu").manual_seed(n)
        Xc = torch.randn(n, d, generator=g) / (p + 1) ** 0.5
        Xc[:, -2:] = torch.rand(n, 2, generator=g) * 2 - 1
        X = Xc.to(dev)
        S = {k: torch.empty_like(X) for k in paths}
        ms = {k: [] for k in paths}
        failed = {}
        for it in range(a.warmup + a.reps):
            for name, tgt in paths.items():
                if name in failed:
                    continue
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                try:
                    e0.record()
                    tgt.score(X, S[name])
                    e1.record()
                    e1.synchronize()
                except torch.OutOfMemoryError as e:    # the callable path's intermediates
                    failed[name] = "out of memory: %s" % str(e).split("\n")[0]
                    torch.cuda.empty_cache()
                    continue
                if it >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
        res = {"n": n, "N": N_, "p": p, "H": H, "d": d, "reps": a.reps}
        for name in paths:
            if name in failed:
                res[name + "_failed"] = failed[name]
            else:
                res[name + "_ms_median"] = round(statistics.median(ms[name]), 4)
                res[name + "_ms_min"] = round(min(ms[name]), 4)
        flop = 4.0 * n * N_ * p * H
        rate = flop / (res["builtin_ms_median"] * 1e-3)
        res["builtin_flop"] = flop
        res["builtin_tflops"] = round(rate / 1e12, 3)
        res["builtin_share_of_fp32_valu_peak"] = round(rate / VALU_PEAK_FLOPS, 4)
        if "callable" not in failed:
            res["callable_over_builtin"] = round(
                res["callable_ms_median"] / res["builtin_ms_median"], 3)
            diff = (S["builtin"] - S["callable"]).abs().double()
            scale = S["callable"].abs().double().amax(0, keepdim=True).clamp_min(1e-30)
            res["max_diff_over_column_max"] = float((diff / scale).max())
        out.append(res)
        print(json.dumps(res), flush=True)
        del X, S
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(dev), "valu_peak_tflops": VALU_PEAK_FLOPS / 1e12,
           "results": out}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--p", type=int, default=13)
    ap.add_argument("--hidden", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=420)
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
        print("bnn_timing: the measuring process ended with status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
