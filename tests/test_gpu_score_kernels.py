"""The target score kernels called directly at their dispatch edges against
fp64: csrc/logreg.hip (every path that (n, N, p, engine, fused) selects), the
Gaussian and mixture scores of csrc/prep.hip and dsvgd_logreg_predict.  The
cases, their inputs, references, measures and preconditions are
tests/score_cases.py's (read its docstring first); each case asserts its
preconditions again here before the device result is read.

A. logreg_small_kernel, register (p <= 32) and LDS form, and the three
   shapes just across its edges, through dsvgd_score_logreg_engine.
B. The two-GEMM paths (fused switched off) on engines 0 = h2, 1 = x3, 2 = f32:
   ldb 128 | 256 | 512 | 1024, a short K into 256 columns (p = 129 .. 224),
   both forms of logreg_finish_kernel; saturated and well-fit particles.
C. The fused score at p = 225 .. 256, 1, 2, 4 and 8 data slices, next to the
   two-GEMM path on the same prepared workspace.
D. dsvgd_score_logreg_prior: pw = 1, 0.5, 8, 0.
E. The workspace contract: nothing written past dsvgd_logreg_workspace_bytes,
   nothing read that prepare / step did not write (NaN- and zero-prefilled
   workspaces give the same bits), and the data half survives the steps.
F. dsvgd_logreg_predict, dsvgd_score_gaussian, dsvgd_score_gmm.
G. dsvgd.targets.LogisticRegression.score on both sides of the small-path
   edge: the wrapper hands each path the workspace it needs.

Every logreg call here runs on a workspace of exactly the documented size
followed by a guard tail, and writes S into a buffer prefilled with a NaN
pattern: a cell of the n x d block left unwritten is not finite, a cell
outside it must keep its bits.

Not observable from outside: which Z form (16x16x32 or 32x32x16) the x3
engine ran -- it follows ldb % 256 in both prepare and step, and a wrong
choice that still computed Z would pass.  The x3 cases cover ldb = 128 (off)
and 256 | 512 | 1024 (on).  Likewise the `fits` fallback of engines 0 and 1
to the f32 engine for images over 2^31 bytes is out of reach at these sizes.
"""
import contextlib

import numpy as np
import pytest
import torch

import score_cases as SC
from conftest import record_parity
from oracle import svgd_oracle as O
from test_gpu_range import ROW_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
TAIL = 4096
FUSED_VS_GEMM = 5e-6     # test_logreg_scores_fused's figure, max-normalised
PATTERN = np.uint32(0x7fc0beef)   # a quiet NaN with a payload


def native():
    from dsvgd import _native as N
    return N


def gpu(a):
    return torch.as_tensor(np.array(a, order="C"), device=DEV)     # a copy: the cases are read-only


def stream():
    return native().stream(torch.device(DEV))


def sync():
    torch.cuda.synchronize()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def pattern(*shape):
    return np.full(shape, PATTERN, np.uint32).view(F32)


def ids(cases):
    return [SC.case_id(c) for c in cases]


@contextlib.contextmanager
def fused_switch(on):
    lib = native().load()
    prev = lib.dsvgd_logreg_set_fused(int(on))
    try:
        yield
    finally:
        lib.dsvgd_logreg_set_fused(prev)


class Workspace(object):
    """`nbytes` bytes at a 256-byte boundary, prefilled with NaN or zeros,
    followed by a guard tail of TAIL bytes of 0xA5."""

    def __init__(self, nbytes, fill="nan"):
        assert nbytes % 256 == 0 and nbytes > 0
        self.buf = torch.empty(nbytes + TAIL + 512, dtype=torch.uint8, device=DEV)
        off = (-self.buf.data_ptr()) % 256
        self.body = self.buf[off:off + nbytes]
        self.tail = self.buf[off + nbytes:off + nbytes + TAIL]
        self.body.view(torch.float32).fill_(float("nan") if fill == "nan" else 0.0)
        self.tail.fill_(0xA5)
        self.ptr = self.body.data_ptr()
        assert self.ptr % 256 == 0

    def tail_kept(self):
        return bool((self.tail == 0xA5).all())


def logreg_ws(c, fill="nan"):
    lib = native().load()
    if lib.dsvgd_logreg_small(c.n, c.N, c.p):
        return Workspace(256, fill)
    return Workspace(lib.dsvgd_logreg_workspace_bytes(c.n, c.N, c.p), fill)


class Staged(object):
    """A case's inputs on the device.  Strided cases: ldx = d + 3, lds =
    d + 1, ldxd = p + 2, the particle rows in the middle of a NaN buffer."""

    def __init__(self, c, X, xd, t):
        self.c, self.n, self.d, self.p = c, c.n, c.p + 1, c.p
        n, d, p = self.n, self.d, self.p
        self.ldx, self.lds, self.ldxd, self.r0, self.s0 = (
            (d + 3, d + 1, p + 2, 2, 1) if c.strided else (d, d, p, 0, 0))
        xb = np.full((c.N, self.ldxd), np.nan, F32)
        xb[:, :p] = xd
        self.xd, self.t = gpu(xb), gpu(np.asarray(t, F32))
        self.X = torch.empty(n + 2 * self.r0, self.ldx, dtype=torch.float32, device=DEV)
        self.S = torch.empty(n + 2 * self.s0, self.lds, dtype=torch.float32, device=DEV)
        self.particles(X)

    def particles(self, X):
        Xb = np.full(tuple(self.X.shape), np.nan, F32)
        Xb[self.r0:self.r0 + self.n, :self.d] = X
        self.X.copy_(gpu(Xb))

    def args_X(self):
        return self.X[self.r0:].data_ptr(), self.ldx, self.n, self.d

    def args_S(self):
        self.S.copy_(gpu(pattern(*self.S.shape)))
        return self.S[self.s0:].data_ptr(), self.lds

    def result(self):
        """The n x d block; every other cell of S must have kept its bits."""
        sync()
        full = self.S.cpu().numpy()
        out = full[self.s0:self.s0 + self.n, :self.d].copy()
        full[self.s0:self.s0 + self.n, :self.d] = pattern(self.n, self.d)
        assert same_bits(full, pattern(*full.shape)), "a cell outside the n x d block was written"
        return out

    # the entry points
    def one_call(self, ws):
        Sp, lds = self.args_S()
        native().call("dsvgd_score_logreg_engine", *self.args_X(), self.xd.data_ptr(), self.ldxd,
                      self.t.data_ptr(), self.c.N, float(self.c.scale), Sp, lds, ws.ptr,
                      self.c.engine, stream())
        return self.result()

    def prepare(self, ws):
        native().call("dsvgd_logreg_prepare", self.xd.data_ptr(), self.ldxd, self.t.data_ptr(),
                      self.c.N, self.n, self.d, ws.ptr, self.c.engine, stream())

    def step(self, ws, pw=None):
        Sp, lds = self.args_S()
        if pw is None:
            native().call("dsvgd_score_logreg_prepared", *self.args_X(), self.c.N,
                          float(self.c.scale), Sp, lds, ws.ptr, self.c.engine, stream())
        else:
            native().call("dsvgd_score_logreg_prior", *self.args_X(), self.c.N,
                          float(self.c.scale), float(pw), Sp, lds, ws.ptr, self.c.engine, stream())
        return self.result()


def staged(c):
    """(preconditions and reference, device inputs) of a case."""
    k = SC.checked(c, ROW_TOL)
    return k, Staged(c, k.X, k.xd, k.t)


def judge(c, k, S, **info):
    """The two measures of score_cases.py on a device result S (n x d)."""
    assert np.isfinite(S).all(), ("not finite", SC.case_id(c), np.argwhere(~np.isfinite(S))[:4])
    got = S.astype(np.float64) / c.scale
    c0 = float(SC.col0_rows(got, k.ref, k.P, c.pw).max())
    if c.variant == "wellfit":
        e = float(SC.whole_rows(got, k.ref).max())
    else:
        rows = SC.data_rows(got, k.ref, k.P.g)
        e = float(rows[k.rows].max(initial=0.0))
        if c.p == 1 and not k.rows.all():       # the ill-conditioned rows of p = 1, by rule
            x = ~k.rows
            back = np.abs(got[x, 1] - k.ref[x, 1]) / k.absg[x, 0]
            info["excused"] = int(x.sum())
            e = max(e, float(back.max()))
    print("%s: data %.3g (fp32 %.3g) col0 %.3g (fp32 %.3g)" % (SC.case_id(c), e, k.a32, c0, k.c32))
    record_parity(e, col0=c0, group=c.group, draw=k.draw, **info)
    assert e <= ROW_TOL, ("data rows", SC.case_id(c), e)
    assert c0 <= SC.COL0_TOL, ("column 0", SC.case_id(c), c0)
    return e


def nerr(got, ref):
    den = float(np.abs(ref).max())
    num = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max())
    return num / den if den > 0 else num


# ------------------------------------------------------ A. the small paths --
A_CASES = SC.cases_A()


@pytest.mark.parametrize("c", A_CASES, ids=ids(A_CASES))
def test_small_paths_and_their_edges(c):
    """logreg_small_kernel's register and LDS forms at N below a block, below
    a wave's 4 rows, general labels with zeros, p = 1, and the three shapes one
    step outside (n = 33, N = 8193 at p = 33), which take the GEMM path and
    need the real workspace."""
    lib = native().load()
    assert bool(lib.dsvgd_logreg_small(c.n, c.N, c.p)) == (c.path != "edge")
    k, st = staged(c)
    ws = logreg_ws(c)
    S = st.one_call(ws)
    assert ws.tail_kept()
    judge(c, k, S)


# ------------------------------------------------- B. the two-GEMM paths --
B_CASES = SC.cases_B()


@pytest.mark.parametrize("c", B_CASES, ids=ids(B_CASES))
def test_two_gemm_paths(c):
    """Z and G . Xd as two kernels on each engine, every ldb, the short K of
    p = 129 .. 224 and both finish forms.  Saturated: every output finite
    with |z| past 88 and 1000.  Well fit: the whole-row measure (g is far
    below a w; see score_cases.py)."""
    k, st = staged(c)
    ws = logreg_ws(c)
    with fused_switch(0):
        st.prepare(ws)
        S = st.step(ws)
    assert ws.tail_kept()
    judge(c, k, S)


# ------------------------------------------------------ C. the fused score --
C_CASES = SC.cases_C()


def test_fused_table_reaches_every_slice_count():
    assert {SC.fused_splits_rule(c.n, c.N) for c in C_CASES} == {1, 2, 4, 8}
    assert [SC.fused_splits_rule(300, N) for N in (256, 1024, 2048, 4096)] == [1, 2, 4, 8]


@pytest.mark.parametrize("c", C_CASES, ids=ids(C_CASES))
def test_fused_score(c):
    """The fused kernel at every p it is taken for (225 .. 256: p = 256 is
    16 K-steps of 16 weights, ldb = 256 and the register form of the finish,
    all within the kernel's layout), particle counts on both sides of its
    128-row block and 1, 2, 4 and 8 data slices; the two-GEMM path on the
    same prepared workspace agrees to 5e-6 max-normalised."""
    assert SC.fused_rule(c.n, c.N, c.p)
    k, st = staged(c)
    ws = logreg_ws(c)
    with fused_switch(1):
        st.prepare(ws)
        S = st.step(ws)
    with fused_switch(0):
        S2 = st.step(ws)
    assert ws.tail_kept()
    judge(c, k, S, slices=SC.fused_splits_rule(c.n, c.N))
    e = nerr(S, S2)
    assert e <= FUSED_VS_GEMM, ("fused vs two-GEMM", SC.case_id(c), e)


# ------------------------------------------------------- D. prior weight --
D_CASES = SC.cases_D()


@pytest.mark.parametrize("c", D_CASES, ids=ids(D_CASES))
def test_prior_weight(c):
    """Data term + pw x prior terms: 4 fused slices, the p > 256 loop form of
    the finish and the register form; pw = 1 gives dsvgd_score_logreg_prepared's
    bits, pw = 0 a column 0 of exact zeros."""
    assert SC.fused_rule(c.n, c.N, c.p) == (c.path == "fused")
    k, st = staged(c)
    ws = logreg_ws(c)
    st.prepare(ws)
    S = st.step(ws, pw=c.pw)
    assert ws.tail_kept()
    judge(c, k, S)
    if c.pw == 1.0:
        assert same_bits(S, st.step(ws))
    if c.pw == 0.0:
        assert not S[:, 0].any()


# ------------------------------------------------ E. the workspace contract --
E_CASES = SC.cases_E()


@pytest.mark.parametrize("c", E_CASES, ids=ids(E_CASES))
def test_workspace_contract(c):
    """No overrun (the guard tail after dsvgd_logreg_workspace_bytes keeps its
    bits), no stale read (a NaN- and a zero-prefilled workspace give the same
    finite bits: a padded K column or row read but never written would show),
    and the prepared half survives the steps (X1, X2, X1: the first and third
    results are the same bits, and those of a fresh workspace)."""
    k, st = staged(c)
    pw = None if c.pw == 1.0 else c.pw
    X2 = SC.other_particles(c)
    with fused_switch(c.fused):
        w_nan, w_zero = logreg_ws(c, "nan"), logreg_ws(c, "zero")
        st.prepare(w_nan)
        S1 = st.step(w_nan, pw)
        st.particles(X2)
        S2 = st.step(w_nan, pw)
        st.particles(k.X)
        S3 = st.step(w_nan, pw)
        st.prepare(w_zero)
        S4 = st.step(w_zero, pw)
    assert w_nan.tail_kept() and w_zero.tail_kept()
    for S in (S1, S2, S3, S4):
        assert np.isfinite(S).all()
    assert not same_bits(S1, S2)
    assert same_bits(S1, S3), "a step wrote into the prepared data"
    assert same_bits(S1, S4), "the result depends on what the workspace held"
    judge(c, k, S1)


# ------------------------------------------- F. predict, Gaussian, mixture --
def _predict(X, xt, fill="nan", ldx=None, ldxt=None):
    N, lib = native(), native().load()
    n, d = X.shape
    Nt, p = xt.shape
    ldx, ldxt = ldx or d, ldxt or p
    Xb = np.full((n, ldx), np.nan, F32)
    Xb[:, :d] = X
    xb = np.full((Nt, ldxt), np.nan, F32)
    xb[:, :p] = xt
    Xg, xg = gpu(Xb), gpu(xb)
    ws = Workspace(lib.dsvgd_logreg_predict_workspace_bytes(n, Nt, p), fill)
    prob = gpu(pattern(Nt + 2))
    N.call("dsvgd_logreg_predict", Xg.data_ptr(), ldx, n, d, xg.data_ptr(), ldxt, Nt,
           prob[1:].data_ptr(), ws.ptr, stream())
    sync()
    out = prob.cpu().numpy()
    assert ws.tail_kept()
    assert same_bits(out[[0, -1]], pattern(2)), "prob written outside its Nt entries"
    return out[1:-1].copy()


def _check_prob(prob, X, xt):
    ref = O.predictive_prob(X, xt)
    assert np.isfinite(prob).all() and (prob >= 0).all() and (prob <= 1).all()
    e = float(np.abs(prob - ref).max())
    print("predict n %d Nt %d p %d: %.3g" % (X.shape[0], xt.shape[0], xt.shape[1], e))
    record_parity(e, group="F")
    assert e <= SC.PREDICT_TOL, e


@pytest.mark.parametrize("n,Nt,p", SC.predict_cases())
def test_predict(n, Nt, p):
    """dsvgd_logreg_predict on both sides of its 128 x 128 tile in n and Nt
    and of the 32-column K padding, inside exactly its documented workspace,
    whatever that held before."""
    X, xt = SC.predict_inputs(n, Nt, p)
    prob = _predict(X, xt, "nan")
    _check_prob(prob, X, xt)
    assert same_bits(prob, _predict(X, xt, "zero")), "the result depends on the workspace"


def test_predict_strided():
    X, xt = SC.predict_inputs(129, 127, 33)
    prob = _predict(X, xt, ldx=X.shape[1] + 3, ldxt=xt.shape[1] + 2)
    _check_prob(prob, X, xt)
    assert same_bits(prob, _predict(X, xt))


def test_predict_saturated_particles():
    """Two particles x1000 (|z| in the hundreds): prob finite, in [0, 1]."""
    X, xt = SC.predict_inputs(300, 129, 255, big=True)
    assert np.abs(xt.astype(np.float64) @ X[1, 1:].astype(np.float64)).max() > 88
    _check_prob(_predict(X, xt), X, xt)


def _elementwise(name, X, scale, extra=()):
    """S (n x d) of dsvgd_score_gaussian / _gmm with padded ldx, lds."""
    n, d = X.shape
    ldx, lds = d + 3, d + 1
    Xb = np.full((n + 2, ldx), np.nan, F32)
    Xb[1:n + 1, :d] = X
    Xg, Sg = gpu(Xb), gpu(pattern(n + 2, lds))
    keep = [gpu(a) for a in extra]
    native().call(name, Xg[1:].data_ptr(), ldx, n, d, *[a.data_ptr() for a in keep], float(scale),
                  Sg[1:].data_ptr(), lds, stream())
    sync()
    full = Sg.cpu().numpy()
    out = full[1:n + 1, :d].copy()
    full[1:n + 1, :d] = pattern(n, d)
    assert same_bits(full, pattern(n + 2, lds)), "a cell outside the n x d block was written"
    return out


@pytest.mark.parametrize("scale", [1.0, -2.5])
@pytest.mark.parametrize("n,d", SC.ELEMENTWISE_SHAPES)
def test_score_gaussian(n, d, scale):
    """lam over 2^-10 .. 2^10 and x = mu (1 + 2^-20): per element within
    2^-22 |scale| |lam_c| (|x| + |mu_c|)."""
    X, mu, lam = SC.gaussian_inputs(n, d)
    S = _elementwise("dsvgd_score_gaussian", X, scale, (mu, lam))
    ref = scale * O.score_gaussian(X, mu, lam)
    bound = SC.gaussian_bound(X, mu, lam, scale)
    assert np.isfinite(S).all() and np.abs(ref).min() > 0
    worst = float((np.abs(S - ref) / bound).max())
    record_parity(worst * 2.0 ** -22, group="F")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("scale", [1.0, -2.5])
@pytest.mark.parametrize("n,d", SC.ELEMENTWISE_SHAPES)
def test_score_gmm(n, d, scale):
    """0, +-2, +-1e-3, +-10, +-50 among the inputs: per element within
    1e-5 |scale| (|x| + 2), and exactly 0 at exactly 0."""
    X = SC.gmm_inputs(n, d)
    S = _elementwise("dsvgd_score_gmm", X, scale)
    ref = scale * O.score_gmm(X)
    assert np.isfinite(S).all()
    worst = float((np.abs(S - ref) / SC.gmm_bound(X, scale)).max())
    record_parity(worst * 1e-5, group="F")
    assert worst <= 1.0, worst
    assert (X == 0).any() and (S[X == 0] == 0).all()


# ------------------------------------------------ G. through dsvgd.targets --
G_CASES = SC.cases_G()


@pytest.mark.parametrize("c", G_CASES, ids=ids(G_CASES))
def test_through_targets(c):
    """LogisticRegression.score asks dsvgd_logreg_small which path a shape
    takes and sizes the workspace by the answer: both sides of N = 8192 at
    p = 33 and of n = 32, and prior_weight = 8 at n = 33."""
    import dsvgd
    lib = native().load()
    k = SC.checked(c, ROW_TOL)
    T = dsvgd.targets.LogisticRegression(np.array(k.xd), np.array(k.t))
    Xg = gpu(k.X)
    out = gpu(pattern(c.n, c.p + 1))
    T.score(Xg, out, scale=c.scale, prior_weight=c.pw)
    sync()
    small = bool(lib.dsvgd_logreg_small(c.n, c.N, c.p))
    assert small == (c.path != "edge")
    (key, ws), = T._ws.items()
    assert key[1] == (0 if small else c.n)
    if not small:
        base = ws.data_ptr()
        room = base + ws.numel() * 4 - (base + 255) // 256 * 256
        assert room >= lib.dsvgd_logreg_workspace_bytes(c.n, c.N, c.p)
    judge(c, k, out.cpu().numpy())
