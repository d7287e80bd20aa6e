"""Time the MMD two-sample diagnostic at the bench's D (n = m = 32768, d = 256:
a pooled 65536 x 65536 matrix): the sweep dsvgd_mmd_rows, the finish
dsvgd_mmd_finish and the whole dsvgd.metrics.mmd, with HIP events, against two
yardsticks over the same D -- the KSD's sweep dsvgd_ksd_rows and one
dsvgd_radix_hist pass (pass 1 over D itself: the select's fallback).

    python scripts/mmd_timing.py [--n N] [--m M] [--d D] [--reps R] [--warmup W]
                                 [--whole K] [--json PATH]

The sweeps and the yardsticks alternate inside one loop, so all see the same
machine state; reported: median, minimum and maximum over the repeats, each
pass's achieved GB/s over the bytes of D it must read (the stored tiles of the
symmetric layout, or the whole block), and the mark of the MMD sweep: its
median against the KSD sweep's median plus that sweep's own min-to-max spread.
metrics.mmd builds an engine per call (pack, distances, the exact median, the
sweep), so it is timed --whole times, on its own.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dist-svgd_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--m", type=int, default=32768)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--whole", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import dsvgd
    from dsvgd import _native as N
    from dsvgd import metrics
    from dsvgd.engine import SelectState
    dev = N.require_gpu("cuda:0")
    n, m, d = a.n, a.m, a.d
    NN = n + m
    g = torch.Generator(device="cpu").manual_seed(0)
    P = torch.randn(n, d, generator=g).to(dev)
    Q = (torch.randn(m, d, generator=g) + 0.1).to(dev)
    Z = torch.cat([P, Q], 0)
    mu, lam = torch.randn(d, generator=g), torch.rand(d, generator=g) * 1.5 + 0.5
    S = torch.empty_like(Z)
    dsvgd.targets.Gaussian(mu, lam).score(Z, S)
    eng = dsvgd.PhiEngine(NN, d, device=dev)
    eng.step(Z, S, step=0.0, write_phi=False)      # D, the median, and what ksd() reads
    eng.ksd()                                       # allocates the KSD's workspaces
    med = eng.state.read()[0]
    eng.fixed_bandwidth(med if med > 0 else 1.0)    # the MMD rule: no 1 / log N
    out = eng.mmd(n)                                # allocates the MMD's
    torch.cuda.synchronize()
    K, W, sym, s = eng._ksd, eng._mmd, int(eng.sym), N.stream(dev)
    T = eng.n_pad // 128
    d_bytes = (T * (T + 1) // 2) * 128 * 128 * 4 if sym else eng.m_pad * eng.n_pad * 4
    st2 = SelectState(dev)     # the yardstick's own state: eng.state keeps h

    def mmd_rows():
        N.call("dsvgd_mmd_rows", N.ptr(eng.D), eng.n_pad, NN, n, eng.state.ptr, eng._kern, sym,
               W["parts"], 0, N.ptr(W["P"]), s)

    def mmd_finish():
        N.call("dsvgd_mmd_finish", N.ptr(W["P"]), NN, n, sym, W["parts"], 0, N.ptr(W["rp"]),
               N.ptr(W["rq"]), N.ptr(W["witness"]), N.ptr(W["ws"]), N.ptr(W["out"]), s)

    def ksd_rows():
        N.call("dsvgd_ksd_rows", N.ptr(eng.D), eng.n_pad, N.ptr(eng.Y), eng.ldy, eng.dp, d, 0, NN,
               NN, eng.state.ptr, sym, K["parts"], N.ptr(K["P"]), N.ptr(K["a"]), s)

    def hist():
        N.call("dsvgd_radix_hist", N.ptr(eng.D), eng.m_pad * eng.n_pad, None, 1, st2.ptr,
               eng.n_pad if sym else 0, s)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    N.call("dsvgd_select_init", st2.ptr, NN, -1, s)
    fns = (("mmd_rows", mmd_rows), ("ksd_rows", ksd_rows), ("radix_hist", hist),
           ("mmd_finish", mmd_finish))
    ms = {k: [] for k, _ in fns}
    for it in range(a.warmup + a.reps):
        for name, fn in fns:           # alternating: the same machine state for all
            t = timed(fn)
            if it >= a.warmup:
                ms[name].append(t)
    del eng, K, W
    torch.cuda.empty_cache()
    res_whole = {}
    ms["metrics_mmd"] = [timed(lambda: res_whole.update(metrics.mmd(P, Q, details=True)))
                         for _ in range(a.whole + 1)][1:]
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = max(ms["ksd_rows"]) - min(ms["ksd_rows"])
    res = {"n": n, "m": m, "d": d, "sym": sym, "reps": a.reps, "d_bytes": d_bytes,
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
           "ms_max": {k: round(max(v), 4) for k, v in ms.items()},
           "GBps": {k: round(d_bytes / med[k] / 1e6, 1) for k in ("mmd_rows", "ksd_rows", "radix_hist")},
           "mmd_over_ksd_rows": round(med["mmd_rows"] / med["ksd_rows"], 3),
           "ksd_rows_spread_ms": round(spread, 4),
           "within_mark": bool(med["mmd_rows"] <= med["ksd_rows"] + spread),
           "out": [float(v) for v in out.cpu()],
           "metrics": {k: res_whole[k] for k in ("mmd", "mmd2_v", "mmd2_u", "h")},
           "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
