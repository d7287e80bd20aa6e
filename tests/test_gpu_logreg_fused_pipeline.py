"""The fused FmtH2 logistic-regression score (logreg_fused_kernel) at the
edges of its software pipeline.

The kernel sweeps the data in 32-row chunks through three stages that run in
different iterations (Z^T of chunk c, sigma of chunk c - 1, G . Xd of chunk
c - 2), with a peeled head and tail and LDS rings that are written one or two
iterations before they are read.  What can go wrong is a chunk dropped, done
twice or shifted against its columns at the head, the tail or a slice
boundary -- so: parity at the shortest sweeps and slice counts there are, one
live chunk at a time at every position near those edges, and the same bits
on a second call.
"""
import numpy as np
import pytest
import torch

from conftest import record_parity
from oracle import svgd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 255


def dsvgd():
    import dsvgd as m
    return m


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _score(X, xd, t, fused=1):
    from dsvgd import _native as N_
    lib = N_.load()
    prev = lib.dsvgd_logreg_set_fused(fused)
    try:
        o = torch.zeros(X.shape[0], P + 1, device=DEV)
        dsvgd().targets.LogisticRegression(xd, t, gemm="h2").score(gpu(X), o)
        torch.cuda.synchronize()
        return o.cpu().numpy()
    finally:
        lib.dsvgd_logreg_set_fused(prev)


def _inputs(n, N, labels, seed):
    rs = np.random.RandomState(seed)
    X = (rs.randn(n, P + 1) * 0.4).astype(np.float32)
    xd = (rs.randn(N, P) / np.sqrt(P)).astype(np.float32)
    t = (np.where(rs.randn(N) > 0, 1.0, -1.0) if labels == "pm1"
         else rs.uniform(-3.0, 3.0, N)).astype(np.float32)
    return X, xd, t


# (1, 1) is the shortest sweep there is (8 chunks, one slice) but n <= 32 takes
# the one-block latency kernel; (33, 1) is the same sweep on the fused kernel.
@pytest.mark.parametrize("labels", ["pm1", "general"])
@pytest.mark.parametrize("n,N", [(1, 1), (33, 1), (129, 256), (300, 257), (200, 1024),
                                 (130, 4096)])
def test_fused_pipeline_parity_at_edges(n, N, labels):
    """Against fp64 and the two-GEMM path on the same inputs, thresholds of
    test_logreg_scores_fused: 8 chunks (the shortest sweep), 16 chunks, two
    slices of 16 (200, 1024) and eight slices (130, 4096)."""
    X, xd, t = _inputs(n, N, labels, n + 3 * N)
    f, g2 = _score(X, xd, t, 1), _score(X, xd, t, 0)
    ref = O.score_logreg(X, xd, t)
    scale = np.abs(ref).max()
    e_f = float(np.abs(f - ref).max() / scale)
    e_2 = float(np.abs(g2 - ref).max() / scale)
    d = float(np.abs(f - g2).max() / np.abs(g2).max())
    print("fused %.3e two-gemm %.3e between %.3e" % (e_f, e_2, d))
    record_parity(e_f, two_gemm=e_2)
    assert e_f < 1e-5 and e_f <= 2.0 * e_2 + 1e-7, (e_f, e_2)
    assert d < 5e-6, d


@pytest.mark.parametrize("N,k", [(512, 0), (512, 1), (512, 2), (512, 13), (512, 14), (512, 15),
                                 (1024, 15), (1024, 16), (1024, 17), (1024, 31)])
def test_fused_pipeline_one_live_chunk(N, k):
    """All data rows zero but the 32 of chunk k (a zero row adds exactly 0):
    N = 512 is one slice of 16 chunks, N = 1024 two slices of 16.  Against
    fp64, normalised by the data term's own maximum -- a dropped, doubled or
    shifted chunk, or G of one chunk against another's columns, moves the
    data term by O(1) of that."""
    n = 130
    X, xd, t = _inputs(n, N, "general", N + k)
    xd[:32 * k] = 0.0
    xd[32 * (k + 1):] = 0.0
    out = _score(X, xd, t, 1)
    ref = O.score_logreg(X, xd, t)
    data = ref - O.score_logreg(X, xd[:0], t[:0])      # without the prior terms
    dmax = np.abs(data).max()
    assert dmax > 0
    tol = 1e-5 * np.abs(ref).max() / dmax
    err = float(np.abs(out - ref).max() / dmax)
    print("err %.3e tol %.3e" % (err, tol))
    record_parity(err)
    assert err < tol, (err, tol)


def test_fused_pipeline_same_bits_on_second_call():
    X, xd, t = _inputs(300, 1024, "pm1", 5)
    a, b = _score(X, xd, t, 1), _score(X, xd, t, 1)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
