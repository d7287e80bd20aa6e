"""The strip-resident FmtH2 distance Gram (csrc/gram_sr.hpp, dsvgd_gram_set_rs
2: a block keeps its 128-row strip's image in LDS, every wave computes and
writes out its own 128 x 64 tiles) against the split-role gram_rs_kernel
(dsvgd_gram_set_rs 1) on the same inputs and against fp64.

Same fragments, products and order as gram_rs / gram_w1, so D is compared bit
for bit in both select modes; in bracket mode the median, the bandwidth, the
below total and the candidate count are equal and the candidates are the same
multiset (the slots hold them in another order).  The fp64 bound is the one of
tests/test_gpu_gram.py: 4e-6 of |x_i - c|^2 + |x_j - c|^2 (c the column
mean), the fp16-pair image's product error.

Shapes: n = 256 (one 256-column pair, two strips), 384 (a padded pair), 1000
(ragged rows and columns), 2176 (17 strips: an odd count, several tiles per
wave and waves with none), and the full layout of a row block with row0 > 0
(m = 256 of n = 1024: 256-aligned -- two rectangles beside the 8-wave
kernel's square -- and 16-aligned -- one rectangle holding the diagonal).
Depths d = 3, 17, 255, 256, 257 and 512.  The image's depth is roundup(d, 32)
(dsvgd_dp), and the one-kernel Gram units take only depths that are multiples
of 256: d = 255 and 256 are the 16 K-steps of the new kernel; d = 3 and 17
(depth 32) and d = 257 (depth 288) run on the 8-wave kernel under either
switch value, d = 512 (32 K-steps) stays on gram_rs_kernel -- all must still
match, and the dispatch is asserted through dsvgd_gram_last_kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (n, d, m, row0)
CASES = [
    (256, 256, None, 0),
    (384, 256, None, 0),
    (1000, 256, None, 0),
    (2176, 256, None, 0),
    (1000, 3, None, 0),
    (1000, 17, None, 0),
    (1000, 255, None, 0),
    (384, 257, None, 0),
    (384, 512, None, 0),
    (1024, 256, 256, 512),
    (1024, 256, 256, 400),
]
SR, RS = 2, 1   # dsvgd_gram_set_rs: strip-resident, split roles
K_NONE, K_W1, K_RS, K_SR = -1, 0, 1, 2   # dsvgd_gram_last_kernel


def _expected_kernel(d, mode):
    dp = -(-d // 32) * 32
    if dp % 256:
        return K_NONE
    return K_SR if (mode == SR and dp == 256) else K_RS


def dsvgd():
    import dsvgd as m
    return m


def _inputs(n, d):
    rs = np.random.RandomState(1000 * d + n)
    X = (rs.randn(n, d) * 1.5 + 3.0).astype(np.float32)
    return torch.as_tensor(X, device=DEV)


def _candidates(eng):
    """The bracket's candidates of every slot, sorted (include/dsvgd.h: the
    candidate buffer's layout)."""
    from dsvgd.engine import _SelectState
    raw = eng.state.buf.cpu()
    nslots = int(raw[_SelectState.nslots.offset // 8])
    cap = int(raw[_SelectState.slot_cap.offset // 8])
    c = eng.cand.cpu()
    cnt = c[:nslots].view(torch.int32).numpy().view(np.uint32) & np.uint32(0x7FFFFFFF)
    assert int(cnt.max()) <= cap
    data = c[2 * nslots:2 * nslots + nslots * cap].numpy().reshape(nslots, cap)
    vals = [data[s, :k] for s, k in enumerate(cnt) if k]
    return np.sort(np.concatenate(vals)) if vals else np.zeros(0, np.float32)


def _run(n, d, m, row0, median, mode, calls=1):
    """One engine under gram switch `mode`: D (padded, dense), the kernel the
    Gram units ran on and, with the accounting, (median, h), (below, ncand),
    the fallback flag and the sorted candidates -- of the last of `calls`
    calls, preceded by the earlier calls' D."""
    from dsvgd import _native as N
    lib = N.load()
    prev = lib.dsvgd_gram_set_rs(mode)
    try:
        eng = dsvgd().PhiEngine(n, d, m=m, row0=row0, device=DEV, gram_gemm="h2")
        assert eng.gram_gemm == "h2"
        eng.pack(_inputs(n, d))
        out = []
        for _ in range(calls):
            eng.D.fill_(float("nan"))
            if median:
                assert eng.bracketed
                eng.distances(median=True)
                kern = lib.dsvgd_gram_last_kernel()
                eng.median_bandwidth()
            else:
                eng.distances(median=False)
                kern = lib.dsvgd_gram_last_kernel()
            torch.cuda.synchronize()
            res = {"D": eng.dense_D(padded=True).clone(), "kernel": kern}
            if median:
                b = eng.state.bracket()
                res.update(med=np.asarray(eng.state.read()[:2], np.float32), counts=tuple(b[2:4]),
                           fallback=b[4], cand=_candidates(eng))
            out.append(res)
        return out
    finally:
        lib.dsvgd_gram_set_rs(prev)


_cache = {}


def _pair(n, d, m, row0, median, monkeypatch):
    """The strip-resident run (twice) and the split-role run, computed once
    per case and shared by the tests."""
    if median:
        monkeypatch.setattr(dsvgd().PhiEngine, "BRACKET_MIN_ENTRIES", 1)
    key = (n, d, m, row0, median)
    if key not in _cache:
        _cache[key] = (_run(n, d, m, row0, median, SR, calls=2), _run(n, d, m, row0, median, RS)[0])
    return _cache[key]


@pytest.mark.parametrize("median", [False, True])
@pytest.mark.parametrize("n,d,m,row0", CASES)
def test_gram_sr_matches_gram_rs(n, d, m, row0, median, monkeypatch):
    (sr, sr2), rs = _pair(n, d, m, row0, median, monkeypatch)
    # the dispatch: 16 K-steps on the new kernel, deeper images on the old one
    assert rs["kernel"] == _expected_kernel(d, RS)
    assert sr["kernel"] == _expected_kernel(d, SR)
    assert torch.equal(sr["D"].view(torch.int32), rs["D"].view(torch.int32))
    mm = n if m is None else m
    idx = torch.arange(mm, device=DEV)
    if not median:
        assert bool((sr["D"][idx, row0 + idx] == 0).all())
    else:
        assert np.array_equal(sr["med"].view(np.uint32), rs["med"].view(np.uint32))
        assert sr["counts"] == rs["counts"]
        assert sr["fallback"] == rs["fallback"]
        assert len(sr["cand"]) > 0
        assert np.array_equal(sr["cand"].view(np.uint32), rs["cand"].view(np.uint32))
    # a second call: the same bits
    assert torch.equal(sr2["D"].view(torch.int32), sr["D"].view(torch.int32))
    if median:
        assert np.array_equal(sr2["med"].view(np.uint32), sr["med"].view(np.uint32))
        assert sr2["counts"] == sr["counts"]
        assert np.array_equal(sr2["cand"].view(np.uint32), sr["cand"].view(np.uint32))


@pytest.mark.parametrize("median", [False, True])
@pytest.mark.parametrize("n,d,m,row0", CASES)
def test_gram_sr_matches_fp64(n, d, m, row0, median, monkeypatch):
    (sr, _), _ = _pair(n, d, m, row0, median, monkeypatch)
    mm = n if m is None else m
    X = _inputs(n, d).double()
    Xc = X - X.mean(0)
    nrm = (Xc ** 2).sum(1)
    ref = torch.cdist(X[row0:row0 + mm], X, compute_mode="donot_use_mm_for_euclid_dist") ** 2
    D = sr["D"]
    assert bool(torch.isposinf(D[mm:, :]).all()) and bool(torch.isposinf(D[:, n:]).all())
    got = D[:mm, :n].double()
    assert bool(torch.isfinite(got).all())
    scale = nrm[row0:row0 + mm, None] + nrm[None, :] + 1e-30
    e = float(((got - ref).abs() / scale).max())
    print("n %d d %d m %s row0 %d median %d: max |D - D64| / (|xi|^2 + |xj|^2) = %.3g"
          % (n, d, m, row0, median, e))
    assert e < 4e-6, e
    if median and m is None and not sr["fallback"]:
        # the exact lower median of the kernel's own D
        k = (n * n - 1) // 2
        exact = torch.kthvalue(D[:n, :n].flatten().cpu(), k + 1).values.item()
        assert sr["med"][:1].view(np.uint32)[0] == np.float32(exact).view(np.uint32)
