"""Time the softmax-regression score: `SoftmaxRegression.score` (csrc/softmax.hip,
the tile form on the f32 MFMA) beside `CallableTarget(target.logp).score` --
the same model as a user logp under torch.func.vmap(grad), the path a user had
before the target existed -- beside the row form forced at the same n (up to
`--rows-up-to` particles), and beside one whole Jacobi step with this target
(the score plus PhiEngine.step with the median bandwidth), on the same device
and inputs, with HIP events.

    python scripts/softmax_timing.py [--n N [N ...]] [--classes C] [--p P] [--rows N]
                                     [--batch B] [--reps R] [--warmup W] [--json PATH]

Defaults: C = 7, p = 54, N = 1024 data rows, the full data and batch = 100,
n = 4096 and 65536 particles.  The measuring process is a child started under
`timeout` (a hang ends there, and nothing further is started on the device);
the paths alternate inside one loop, so all see the same machine state.
Reported per case: median and minimum over the repeats, the ratios of the
medians, the algorithmic flop 4 n B C p and the executed flop (the logits of a
slab's classes are computed twice, those of the others once per slab, rows and
columns are padded to the MFMA's 32 x 32 x 2, and idle waves of the last round
run on zeros) as fractions of the f32 MFMA peak, the score's share of the
Jacobi step, and the largest difference of the two scores against the column
maxima.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dist-svgd_amd"))

MFMA_F32_PEAK_FLOPS = 157.3e12
TILES, CHUNK, WAVES = 16, 32, 4       # csrc/softmax.hip: kSmxTiles, kSmxChunk, waves per workgroup


def executed_flop(n, B, C, p):
    """The flop of the tile form's MFMAs (4096 each)."""
    nkb = -(-p // 32)
    ntile = C * nkb
    per_class = 4 * -(-p // 8)
    mfma = 0
    for t0 in range(0, ntile, TILES):
        nt = min(TILES, ntile - t0)
        ncls = (t0 + nt - 1) // nkb - t0 // nkb + 1
        mfma += (C + ncls) * per_class + 16 * nt
    rounds = -(-(-(-B // CHUNK)) // WAVES)
    return 4096.0 * mfma * rounds * WAVES * -(-n // 32)


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
    from dsvgd.targets import CallableTarget, SoftmaxRegression
    dev = N.require_gpu("cuda:0")
    C, p, rows = a.classes, a.p, a.rows
    rs = np.random.RandomState(0)
    xd = rs.randn(rows, p).astype(np.float32)
    y = rs.randint(0, C, rows)
    out = []
    for batch in (None, a.batch):
        for n in a.n:
            target = SoftmaxRegression(xd, y, classes=C, batch=batch)
            B = target.batch or rows
            d = target.d
            g = torch.Generator(device="cpu").manual_seed(n)
            X = (torch.randn(n, d, generator=g) / p ** 0.5).to(dev)
            S = {k: torch.empty_like(X) for k in ("builtin", "callable", "rows")}
            eng = dsvgd.PhiEngine(n, d, device=dev)
            res = {"n": n, "N": rows, "C": C, "p": p, "batch": batch, "reps": a.reps}
            # the callable differentiates the full-data logp; with a batch its
            # equal is the logp of a window's rows, weighted N / B
            if batch is None:
                logp = target.logp
            else:
                win = SoftmaxRegression(xd[:B], y[:B], classes=C)
                wt = rows / B

                def logp(x, win=win, wt=wt):
                    la = x[0]
                    prior = (0.5 * (d - 1) * la - 0.5 * torch.exp(la) * (x[1:] * x[1:]).sum()
                             + win.a0 * la - win.b0 * torch.exp(la))
                    return wt * (win.logp(x) - prior) + prior
            chunk = min(65536, max(256, a.elements // (B * max(C, 8))))
            call = CallableTarget(logp, chunk=chunk)
            res["callable_chunk"] = chunk
            paths = {"builtin": lambda: target.score(X, S["builtin"]),
                     "callable": lambda: call.score(X, S["callable"]),
                     "step": lambda: (target.score(X, S["builtin"]),
                                      eng.step(X, S["builtin"], step=0.0, h=None))}
            if n <= a.rows_up_to:
                paths["rows"] = lambda: target.score(X, S["rows"], form="rows")
            ms = {k: [] for k in paths}
            for it in range(a.warmup + a.reps):
                for name, fn in paths.items():
                    t = _timed(fn)
                    if it >= a.warmup:
                        ms[name].append(t)
            for name in paths:
                res[name + "_ms_median"] = round(statistics.median(ms[name]), 4)
                res[name + "_ms_min"] = round(min(ms[name]), 4)
                res[name + "_ms_max"] = round(max(ms[name]), 4)
            sec = res["builtin_ms_median"] * 1e-3
            flop, done = 4.0 * n * B * C * p, executed_flop(n, B, C, p)
            res["algorithmic_flop"] = flop
            res["executed_flop"] = done
            res["algorithmic_share_of_mfma_peak"] = round(flop / sec / MFMA_F32_PEAK_FLOPS, 4)
            res["executed_share_of_mfma_peak"] = round(done / sec / MFMA_F32_PEAK_FLOPS, 4)
            res["score_share_of_jacobi_step"] = round(
                res["builtin_ms_median"] / res["step_ms_median"], 4)
            res["callable_over_builtin"] = round(
                res["callable_ms_median"] / res["builtin_ms_median"], 3)
            res["builtin_beats_callable_beyond_spread"] = (
                res["builtin_ms_max"] < res["callable_ms_min"])
            diff = (S["builtin"] - S["callable"]).abs().double()
            scale = S["callable"].abs().double().amax(0, keepdim=True).clamp_min(1e-30)
            res["max_diff_over_column_max"] = float((diff / scale).max())
            if "rows" in paths:
                res["rows_over_tile"] = round(res["rows_ms_median"] / res["builtin_ms_median"], 3)
                res["tile_beats_rows_beyond_spread"] = res["builtin_ms_max"] < res["rows_ms_min"]
            out.append(res)
            print(json.dumps(res), flush=True)
            del X, S, eng
            torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(dev),
           "mfma_f32_peak_tflops": MFMA_F32_PEAK_FLOPS / 1e12, "results": out}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--p", type=int, default=54)
    ap.add_argument("--rows", type=int, default=1024, help="data rows N")
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--rows-up-to", type=int, default=4096,
                    help="time the forced row form for n up to this")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--elements", type=int, default=1 << 29,
                    help="largest chunk B max(C, 8) of one vmap(grad) call")
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
        print("softmax_timing: the measuring process ended with status %d" % rc, file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
