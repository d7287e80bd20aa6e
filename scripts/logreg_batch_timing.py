"""Time the minibatch logistic-regression score (dsvgd_score_logreg_window,
csrc/logreg_window.hip) beside the full-data score of the same target, and
the Jacobi step (score + direction + update) with and without a batch, with
HIP events.

    python scripts/logreg_batch_timing.py [--n N] [--d D] [--rows N] [--batch B [B ...]]
                                          [--reps R] [--warmup W] [--timeout SECONDS]
                                          [--json PATH]

Defaults: n = 65536 particles, d = 256, N = 16384 data rows, B = 100, 1024 and
4096, 2 warm-up and 10 timed rounds.  The measuring process is a child started
under `timeout` (a hang ends there, and nothing further is started on the
device).  The window scores and the full-data score alternate inside one
loop, so all see the same machine state; so do the two steps.  Reported per
B: median and minimum, the achieved 8 n d bytes per second (X read, S
written) against the measured copy rate, the achieved 4 n B roundup(p, 32)
flop per second against the f32 MFMA rate, and which of the two bounds is
the nearer one.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dist-svgd_amd"))

COPY_BYTES_PER_S = 6.3e12     # measured device copy rate
MFMA_F32_FLOPS = 155e12       # f32-input MFMA rate


def measure(a):
    import numpy as np
    import torch

    import dsvgd
    from dsvgd import _native as N
    from dsvgd.targets import LogisticRegression
    dev = N.require_gpu("cuda:0")
    n, d, rows = a.n, a.d, a.rows
    p = d - 1
    rs = np.random.RandomState(0)
    xd = (rs.randn(rows, p) / np.sqrt(p)).astype(np.float32)
    t = np.where(rs.randn(rows) > 0, 1.0, -1.0).astype(np.float32)
    g = torch.Generator(device="cpu").manual_seed(0)
    X = (0.3 * torch.randn(n, d, generator=g)).to(dev)
    full = LogisticRegression(xd, t)
    paths = {"full": full}
    for B in a.batch:
        paths["B=%d" % B] = LogisticRegression(xd, t, batch=B)
    S = torch.empty_like(X)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    ms = {k: [] for k in paths}
    for it in range(a.warmup + a.reps):
        for name, tgt in paths.items():
            v = timed(lambda: tgt.score(X, S))
            tgt.next_batch()
            if it >= a.warmup:
                ms[name].append(v)
    res = {"n": n, "d": d, "N": rows, "reps": a.reps, "device": torch.cuda.get_device_name(dev),
           "score_ms_median": {k: round(statistics.median(v), 4) for k, v in ms.items()},
           "score_ms_min": {k: round(min(v), 4) for k, v in ms.items()}}
    pp = -(-p // 32) * 32
    res["window"] = []
    for B in a.batch:
        sec = statistics.median(ms["B=%d" % B]) * 1e-3
        bw, fl = 8.0 * n * d / sec, 4.0 * n * B * pp / sec
        res["window"].append({
            "B": B, "ms_median": round(sec * 1e3, 4), "ms_min": round(min(ms["B=%d" % B]), 4),
            "TB_per_s": round(bw / 1e12, 3), "share_of_copy_rate": round(bw / COPY_BYTES_PER_S, 4),
            "tflops": round(fl / 1e12, 2), "share_of_mfma_rate": round(fl / MFMA_F32_FLOPS, 4),
            "nearer_bound": "hbm" if bw / COPY_BYTES_PER_S > fl / MFMA_F32_FLOPS else "mfma",
            "over_full": round(sec * 1e3 / statistics.median(ms["full"]), 4)})
    # the Jacobi step: score, then the direction and the update
    eng = dsvgd.PhiEngine(n, d, device=dev)
    Xw = X.clone()
    B0 = a.batch[0]
    steps = {}
    for name, tgt in (("full", full), ("B=%d" % B0, paths["B=%d" % B0])):
        def step(tgt=tgt):
            tgt.score(X, S)
            eng.step(X, S, X_own=Xw, step=0.0, write_phi=False)
            tgt.next_batch()
        steps[name] = step
    sm = {k: [] for k in steps}
    for it in range(a.warmup + a.reps):
        for name, fn in steps.items():
            v = timed(fn)
            if it >= a.warmup:
                sm[name].append(v)
    res["step_ms_median"] = {k: round(statistics.median(v), 4) for k, v in sm.items()}
    res["step_ms_min"] = {k: round(min(v), 4) for k, v in sm.items()}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--batch", type=int, nargs="+", default=[100, 1024, 4096])
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
        print("logreg_batch_timing: the measuring process ended with status %d" % rc,
              file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
