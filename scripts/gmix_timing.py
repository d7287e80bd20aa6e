"""Time the Gaussian-mixture score: `GaussianMixture.score` (one kernel,
csrc/gmix.hip) beside `CallableTarget(target.logp).score` -- the same model as
a user logp under torch.func.vmap(grad), the path a user had before the target
existed -- and beside one whole Jacobi step with this target (the score plus
PhiEngine.step with the median bandwidth), on the same device and inputs, with
HIP events.

    python scripts/gmix_timing.py [--n N] [--d D] [--K K [K ...]] [--reps R] [--warmup W]
                                  [--elements E] [--timeout SECONDS] [--json PATH]

Defaults: n = 65536 particles, d = 256, K = 2, 64 and 1024 components.  The
measuring process is a child started under `timeout` (a hang ends there, and
nothing further is started on the device); the paths alternate inside one loop,
so all see the same machine state.  The callable path holds several
(chunk, K, d) intermediates: its chunk is the library's default (65536
particles) where chunk K d stays within `--elements` (2^29: 2 GiB each), else
the largest that does, and is reported.  Reported per K: median and minimum over the repeats, the ratio
of the medians, the kernel's 6 n K d flop and its rate, the score's share of
the Jacobi step, and the largest difference of the two scores against the
column maxima.
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


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(a):
    import numpy as np
    import torch

    import dsvgd
    from dsvgd import _native as N
    from dsvgd.targets import CallableTarget, GaussianMixture
    dev = N.require_gpu("cuda:0")
    n, d = a.n, a.d
    out = []
    for K in a.K:
        rs = np.random.RandomState(K)
        means = (0.2 * rs.randn(K, d)).astype(np.float32)
        lam = np.exp(rs.uniform(-1, 1, (K, d))).astype(np.float32)
        w = rs.uniform(0.2, 1, K).astype(np.float32)
        target = GaussianMixture(means, lam, w)
        g = torch.Generator(device="cpu").manual_seed(K)
        comp = torch.randint(0, K, (n,), generator=g)
        X = (torch.from_numpy(means)[comp]
             + torch.randn(n, d, generator=g) / torch.from_numpy(lam)[comp].sqrt()).to(dev)
        S = {k: torch.empty_like(X) for k in ("builtin", "callable")}
        eng = dsvgd.PhiEngine(n, d, device=dev)
        res = {"n": n, "d": d, "K": K, "reps": a.reps}
        # the callable path holds several (chunk, K, d) intermediates
        chunk = min(CallableTarget(target.logp).chunk, max(256, a.elements // (K * d)))
        call = CallableTarget(target.logp, chunk=chunk)
        res["callable_chunk"] = chunk
        try:
            _timed(lambda: call.score(X, S["callable"]))
        except torch.OutOfMemoryError as e:
            torch.cuda.empty_cache()
            res["callable_failed"] = "out of memory: %s" % str(e).split("\n")[0]
            call = None
        paths = {"builtin": lambda: target.score(X, S["builtin"]),
                 "step": lambda: (target.score(X, S["builtin"]),
                                  eng.step(X, S["builtin"], step=0.0, h=None))}
        if call is not None:
            paths["callable"] = lambda: call.score(X, S["callable"])
        ms = {k: [] for k in paths}
        for it in range(a.warmup + a.reps):
            for name, fn in paths.items():
                t = _timed(fn)
                if it >= a.warmup:
                    ms[name].append(t)
        for name in paths:
            res[name + "_ms_median"] = round(statistics.median(ms[name]), 4)
            res[name + "_ms_min"] = round(min(ms[name]), 4)
        flop = 6.0 * n * K * d
        rate = flop / (res["builtin_ms_median"] * 1e-3)
        res["builtin_flop"] = flop
        res["builtin_tflops"] = round(rate / 1e12, 3)
        res["builtin_share_of_fp32_valu_peak"] = round(rate / VALU_PEAK_FLOPS, 4)
        res["score_share_of_jacobi_step"] = round(
            res["builtin_ms_median"] / res["step_ms_median"], 4)
        if call is not None:
            res["callable_over_builtin"] = round(
                res["callable_ms_median"] / res["builtin_ms_median"], 3)
            diff = (S["builtin"] - S["callable"]).abs().double()
            scale = S["callable"].abs().double().amax(0, keepdim=True).clamp_min(1e-30)
            res["max_diff_over_column_max"] = float((diff / scale).max())
        out.append(res)
        print(json.dumps(res), flush=True)
        del X, S, eng
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(dev), "valu_peak_tflops": VALU_PEAK_FLOPS / 1e12,
           "results": out}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--K", type=int, nargs="+", default=[2, 64, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--elements", type=int, default=1 << 29,
                    help="largest chunk K d of one vmap(grad) call (2 GiB of fp32 each)")
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
        print("gmix_timing: the measuring process ended with status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
