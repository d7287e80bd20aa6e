"""Time the KSD diagnostic at the bench configuration (n = 65536, d = 256,
median bandwidth, after one engine.step): the sweep dsvgd_ksd_rows, the finish
dsvgd_ksd_finish and the whole PhiEngine.ksd(), with HIP events, against the
yardstick -- dsvgd_radix_hist, the existing streaming pass over the same D
(pass 1 over D itself: the select's fallback).

    python scripts/ksd_timing.py [--n N] [--d D] [--reps R] [--warmup W] [--json PATH]

The sweep and the yardstick alternate inside one loop, so both see the same
machine state; reported: median and minimum over the repeats, the ratio of
the medians, and the sweep's achieved GB/s over the bytes of D it must read
(the stored tiles of the symmetric layout, or the whole m_pad x n_pad block).
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
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import dsvgd
    from dsvgd import _native as N
    from dsvgd.engine import SelectState
    dev = N.require_gpu("cuda:0")
    n, d = a.n, a.d
    g = torch.Generator(device="cpu").manual_seed(0)
    X = torch.randn(n, d, generator=g).to(dev)
    mu, lam = torch.randn(d, generator=g), torch.rand(d, generator=g) * 1.5 + 0.5
    S = torch.empty_like(X)
    dsvgd.targets.Gaussian(mu, lam).score(X, S)
    eng = dsvgd.PhiEngine(n, d, device=dev)
    eng.step(X, S, X_own=X, step=1e-3, write_phi=False)
    out = eng.ksd()            # allocates the workspaces
    torch.cuda.synchronize()
    W, sym, s = eng._ksd, int(eng.sym), N.stream(dev)
    T = eng.n_pad // 128
    d_bytes = (T * (T + 1) // 2) * 128 * 128 * 4 if sym else eng.m_pad * eng.n_pad * 4
    st2 = SelectState(dev)     # the yardstick's own state: eng.state keeps h

    def rows():
        N.call("dsvgd_ksd_rows", N.ptr(eng.D), eng.n_pad, N.ptr(eng.Y), eng.ldy, eng.dp, d, 0, n,
               n, eng.state.ptr, sym, W["parts"], N.ptr(W["P"]), N.ptr(W["a"]), s)

    def finish():
        N.call("dsvgd_ksd_finish", N.ptr(eng.KY), eng.ldy, N.ptr(eng.rowsum), eng.splits,
               N.ptr(eng.Y), eng.ldy, eng.dp, d, 0, n, n, eng.state.ptr, sym, W["parts"],
               N.ptr(W["P"]), N.ptr(W["rows"]), N.ptr(W["ws"]), N.ptr(W["out"]), s)

    def hist():
        N.call("dsvgd_radix_hist", N.ptr(eng.D), eng.m_pad * eng.n_pad, None, 1, st2.ptr,
               eng.n_pad if sym else 0, s)

    def whole():
        eng.ksd(out=out)

    N.call("dsvgd_select_init", st2.ptr, n, -1, s)
    fns = (("ksd_rows", rows), ("radix_hist", hist), ("ksd_finish", finish), ("engine_ksd", whole))
    ms = {k: [] for k, _ in fns}
    for it in range(a.warmup + a.reps):
        for name, fn in fns:           # alternating: the same machine state for all
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"n": n, "d": d, "sym": sym, "parts": W["parts"], "splits": int(eng.splits),
           "reps": a.reps, "d_bytes": d_bytes,
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
           "rows_over_hist": round(med["ksd_rows"] / med["radix_hist"], 3),
           "rows_GBps": round(d_bytes / med["ksd_rows"] / 1e6, 1),
           "hist_GBps": round(d_bytes / med["radix_hist"] / 1e6, 1),
           "ksd": [float(v) for v in out.cpu()],
           "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
