"""Case tables, input builders, fp64 references, the float32 restatement and
the preconditions of the target score kernels' suite (test_score_cases_host.py
on the CPU, test_gpu_score_kernels.py on the device).  No GPU in here.

The logistic-regression score of n particles x = [log a, w] over N data rows
(xd, t) is  S[:, 1:] = g - pw a w,  S[:, 0] = pw (-a + p/2 - a |w|^2 / 2)
with the data term  g = G Xd,  G_iq = t_q sigma(-t_q w_i . xd_q)  and the
prior weight pw (1 unless dsvgd_score_logreg_prior).  Two measures:

* data rows:  max_i |S_i[1:] / scale - ref_i[1:]|_2 / |g_i|_2   <= ROW_TOL
  -- normalised by the part the GEMMs compute, not by the prior;
* column 0:   |S_i0 / scale - ref_i0| <= COL0_TOL pw (a_i + p/2 + a_i |w_i|^2 / 2)
  (one expf and a 64-lane tree sum of at most 16 squares per lane: under
  8 ulp of the largest term).

Every case's inputs must first show, in fp64, that
(a) the same formula in numpy float32 stays below a tenth of the data-row
    bound (a tolerance that fp32 arithmetic itself cannot meet measures
    nothing) and below a QUARTER of the column-0 bound, COL0_PRE = 2.5e-7:
    column 0 in float32 is expf (1 ulp in numpy), the sum of squares, a
    product and two additions, four or five roundings of 2^-24 of the
    largest term, so float32 itself reaches 2.2e-7 on these inputs and a
    tenth of 1e-6 (0.84 ulp) is below what any float32 evaluation can
    promise.  The kernels' own bound, COL0_TOL = 1e-6, is not touched;
(b) |a_i w_i| <= 8 |g_i| for every row (the prior's rounding is not what
    the data-row measure sees);
(c) dropping data row N - 1, dropping weight column p - 1 from Z only, and
    (general labels) replacing the largest label by its sign each move the
    data-row measure by SENS = 100 x ROW_TOL.
A mutation that cannot apply is skipped by RULE (p = 1: no column to drop
from a non-empty Z; N = 1: no row to drop and leave data), never by
tolerance, and at most one case in five of a group skips one.

The recipe is seeded per case; a case takes the first of DRAWS = 64 seeds
whose inputs meet (a) - (c) (`checked`).  The preconditions see fp64 and
numpy float32 only, never the code under test.

p = 1 has a rule of its own.  There g_i is ONE number, a decreasing function
of w_i that crosses zero at the maximum-likelihood weight, which lies inside
the particle cloud: the particles next to it have |g_i| far below the sum of
the magnitudes of its N terms, and no float32 summation holds such a row to
1e-6 |g_i| (33 particles: about 1e-5; 255: up to 2e-4), whatever the seed.
So at p = 1 precondition (a) decides per row: the rows the float32
restatement holds to a tenth of ROW_TOL are measured as everywhere else;
the others are held to the same figure relative to the sum of magnitudes,
|S_i1 / scale - ref_i1| <= ROW_TOL sum_q |G_iq| |xd_q| -- the bound the
measure itself gives a row without cancellation.

Three variants have their own rules, all from their construction:
* saturated: rows 1 and 2 of W are scaled by 100 and 1000, so |z| passes 88
  (expf overflows) and 1000 (asserted).  Every output must be finite.
  Preconditions (a) and (b) decide whether the x1000 row is measured: where
  float32 itself cannot hold that row to a tenth of the bound, or its prior
  term is more than 8 |g|, the row is only required to be finite.  No other
  row may be excused.
* well fit: labels sign(xd . w*), particles 20 w* + 0.3 randn.  g is far
  below a w, so (b) fails by design and no mutation of the data registers:
  the case is judged by the whole-row measure of test_gpu_range.py
  (row_err <= ROW_TOL) -- the fp16 image of G has an absolute floor, and
  relative to the whole row is the honest bound there.  (a) is held in that
  measure; (b) and (c) do not apply and the case does not count towards the
  skip cap.
"""
import collections
import functools
import zlib

import numpy as np

from oracle import svgd_oracle as O

F32 = np.float32
COL0_TOL = 1e-6
COL0_PRE = 2.5e-7      # (a) for column 0: see the module docstring
DRAWS = 64
PREDICT_TOL = 2e-6
SENS = 100.0
PRIOR_RATIO = 8.0
SKIP_CAP = 0.2

Case = collections.namedtuple(
    "Case", "group path n N p labels engine fused variant strided scale pw")


def case(group, path, n, N, p, labels="pm1", engine=0, fused=1, variant="plain", strided=False,
         scale=1.0, pw=1.0):
    return Case(group, path, n, N, p, labels, engine, fused, variant, strided, scale, pw)


def case_id(c):
    s = "%s-%s-n%d-N%d-p%d-%s-e%d" % (c.group, c.path, c.n, c.N, c.p, c.labels, c.engine)
    if not c.fused:
        s += "-unfused"
    if c.variant != "plain":
        s += "-" + c.variant
    if c.strided:
        s += "-strided"
    if c.pw != 1.0:
        s += "-pw%g" % c.pw
    return s


def seed_of(c, draw=0):
    return (zlib.crc32(case_id(c).encode()) + 7919 * draw) & 0x7fffffff


def rup(x, m):
    return -(-x // m) * m


def small_rule(n, N, p):
    """The documented rule of the one-block path (include/dsvgd.h)."""
    return n <= 32 and (p <= 32 or N <= 8192)


def fused_splits_rule(n, N):
    """The slice count csrc/logreg.hip documents for the fused score: doubled
    while it is below 8, the launch has under 256 blocks of 128 particles and
    every slice keeps at least 16 chunks of 32 data rows."""
    n_pad, N_pad = rup(n, 256), rup(N, 256)
    z = 1
    while z < 8 and (n_pad // 128) * z < 256 and (N_pad // 32) // (2 * z) >= 16:
        z *= 2
    return z


def fused_rule(n, N, p):
    """Whether engine 0 with the fused switch on runs the fused kernel."""
    return not small_rule(n, N, p) and rup(p, 32) == 256


# ---------------------------------------------------------------- tables --
def _thin(shapes, ns, group, path, **kw):
    """Shapes on which a mutation cannot apply (p = 1 or N = 1) once each,
    n and the labels alternating; every other shape with every n and both
    label kinds.  Keeps every edge value and the skip share under the cap."""
    out, k = [], 0
    for p, N in shapes:
        if p == 1 or N == 1:
            out.append(case(group, path, ns[k % len(ns)], N, p, ("pm1", "gen")[(k // 2) % 2], **kw))
            k += 1
        else:
            out += [case(group, path, n, N, p, lab, **kw) for n in ns for lab in ("pm1", "gen")]
    return out


def cases_A():
    reg = [(p, N) for p in (1, 2, 31, 32) for N in (1, 63, 255, 256, 257, 1025)]
    lds = [(p, N) for p in (33, 64, 65, 255, 1023) for N in (1, 3, 4, 5, 8192)]
    out = _thin(reg, (1, 32), "A", "reg") + _thin(lds, (1, 32), "A", "lds")
    for n, p, N in ((33, 2, 5), (32, 33, 8193), (33, 33, 1)):      # across the edge: GEMM path
        out += [case("A", "edge", n, N, p, lab) for lab in ("pm1", "gen")]
    out.append(case("A", "reg", 32, 257, 31, "gen", strided=True, scale=3.0))
    out.append(case("A", "lds", 32, 5, 65, "pm1", strided=True, scale=3.0))
    return out


B_P = (1, 32, 33, 128, 129, 160, 224, 225, 255, 256, 257, 512, 513, 1023)
B_NN = ((33, 1), (255, 257), (256, 256), (257, 255))


def cases_B():
    out, k = [], 0
    for e in (0, 1, 2):
        for p in B_P:
            for n, N in (B_NN if e == 0 else ((255, 257), (257, 255))):
                out.append(case("B", "gemm", n, N, p, ("pm1", "gen")[k % 2], engine=e, fused=0))
                k += 1
    for e, p in ((0, 160), (1, 33), (2, 257)):
        out.append(case("B", "gemm", 255, 257, p, "gen", engine=e, fused=0, strided=True, scale=3.0))
    for e in (0, 1, 2):
        for p in (255, 40):
            out.append(case("B", "gemm", 255, 257, p, "pm1", engine=e, fused=0, variant="sat"))
            out.append(case("B", "gemm", 255, 257, p, "fit", engine=e, fused=0, variant="wellfit"))
    return out


def cases_C():
    return [case("C", "fused", n, N, p, lab)
            for p in (225, 240, 255, 256) for n in (33, 128, 129, 300)
            for N in (1, 256, 1024, 2048, 4096, 4097) for lab in ("pm1", "gen")]


D_SHAPES = ((300, 2048, 255, "fused", "gen"), (257, 255, 513, "gemm", "pm1"),
            (255, 257, 160, "gemm", "pm1"))


def cases_D():
    return [case("D", path, n, N, p, lab, pw=pw)
            for n, N, p, path, lab in D_SHAPES for pw in (1.0, 0.5, 8.0, 0.0)]


def cases_E():
    """One shape per path of B, C and D (the predict workspace is group F's)."""
    return [case("E", "gemm", 255, 257, 160, "gen", engine=0, fused=0),
            case("E", "gemm", 255, 257, 160, "gen", engine=1, fused=0),
            case("E", "gemm", 257, 255, 513, "gen", engine=1, fused=0),
            case("E", "gemm", 255, 257, 160, "gen", engine=2, fused=0),
            case("E", "fused", 300, 2048, 255, "gen"),
            case("E", "fused", 129, 1024, 256, "pm1"),
            case("E", "gemm", 257, 255, 513, "pm1", pw=8.0)]


def cases_G():
    return [case("G", "lds", 32, 8192, 33, "pm1"), case("G", "edge", 32, 8193, 33, "gen"),
            case("G", "edge", 33, 5, 2, "gen"), case("G", "edge", 33, 5, 2, "pm1", pw=8.0)]


GROUPS = {"A": cases_A, "B": cases_B, "C": cases_C, "D": cases_D, "E": cases_E, "G": cases_G}


def all_cases():
    return [c for g in sorted(GROUPS) for c in GROUPS[g]()]


# ---------------------------------------------------------------- inputs --
def inputs(c, draw=0):
    """(X (n, p + 1), xd (N, p), t (N,)) float32, seeded by the case's id."""
    rs = np.random.RandomState(seed_of(c, draw))
    n, N, p = c.n, c.N, c.p
    X = np.empty((n, p + 1), F32)
    X[:, 1:] = 0.3 * rs.randn(n, p)
    X[:, 0] = rs.uniform(-3.0, -1.0, n)
    xd = (rs.randn(N, p) / np.sqrt(p)).astype(F32)
    if c.labels == "gen":
        t = rs.uniform(-3.0, 3.0, N).astype(F32)
        t[(N + 2) % 7::7] = 0.0       # every 7th label, never the last (the row (c) drops)
    else:
        t = np.where(rs.randn(N) > 0, 1.0, -1.0).astype(F32)
    if c.variant == "sat":
        X[1, 1:] *= F32(100.0)
        X[2, 1:] *= F32(1000.0)
    elif c.variant == "wellfit":
        ws = rs.randn(p)
        t = np.where(xd.astype(np.float64) @ ws >= 0, 1.0, -1.0).astype(F32)
        X[:, 1:] = (20.0 * ws[None, :] + 0.3 * rs.randn(n, p)).astype(F32)
    return X, xd, t


def other_particles(c):
    """A second particle set of the case's shape (workspace reuse)."""
    rs = np.random.RandomState(seed_of(c) ^ 0x5a5a5a)
    X = np.empty((c.n, c.p + 1), F32)
    X[:, 1:] = 0.3 * rs.randn(c.n, c.p)
    X[:, 0] = rs.uniform(-3.0, -1.0, c.n)
    return X


# ------------------------------------------------------------ references --
Parts = collections.namedtuple("Parts", "a W Z G g")


def parts(X, xd, t, zcols=None):
    """The score's pieces in fp64; zcols: Z from the first zcols columns only."""
    X, xd, t = np.asarray(X, np.float64), np.asarray(xd, np.float64), np.asarray(t, np.float64)
    a, W = np.exp(X[:, 0]), X[:, 1:]
    k = W.shape[1] if zcols is None else zcols
    Z = W[:, :k] @ xd[:, :k].T
    G = t[None, :] * O._sigmoid(-t[None, :] * Z)
    return Parts(a, W, Z, G, G @ xd)


def compose(P, pw=1.0):
    """ref (n, 1 + p) from the pieces, the prior weighted by pw."""
    p = P.W.shape[1]
    S = np.empty((P.W.shape[0], p + 1))
    S[:, 0] = pw * (-P.a + 0.5 * p - 0.5 * P.a * (P.W * P.W).sum(1))
    S[:, 1:] = P.g - pw * P.a[:, None] * P.W
    return S


def restate32(X, xd, t, pw=1.0, block=64):
    """The same formula in numpy float32 throughout.  G Xd is summed as the
    kernels sum it, in blocks of data rows whose float32 partial sums are
    then added (numpy's unrolled pairwise sum): a column of g is a sum of N
    terms of either sign, of order sqrt(N) times one term, and ONE running
    float32 sum over N = 1025 terms already misses a tenth of ROW_TOL at
    p = 1 (3.7e-6) -- which says something about summation order, nothing
    about float32."""
    X, xd, t = np.asarray(X, F32), np.asarray(xd, F32), np.asarray(t, F32)
    a, W = np.exp(X[:, 0]), X[:, 1:]
    p = W.shape[1]
    with np.errstate(over="ignore"):
        G = t[None, :] / (F32(1.0) + np.exp(t[None, :] * (W @ xd.T)))
    S = np.empty_like(X)
    pa = F32(pw) * a
    nb = -(-xd.shape[0] // block)
    part = np.empty((X.shape[0], p, nb), F32)
    for b in range(nb):
        part[:, :, b] = G[:, b * block:(b + 1) * block] @ xd[b * block:(b + 1) * block]
    S[:, 1:] = part.sum(-1) - pa[:, None] * W
    S[:, 0] = F32(pw) * (-a + F32(0.5 * p) - F32(0.5) * a * (W * W).sum(1))
    assert S.dtype == F32
    return S


def data_rows(got, ref, g):
    """Per row |got_i[1:] - ref_i[1:]|_2 / |g_i|_2."""
    num = np.sqrt(((np.asarray(got, np.float64)[:, 1:] - ref[:, 1:]) ** 2).sum(1))
    den = np.sqrt((g * g).sum(1))
    return num / np.maximum(den, 1e-300)


def col0_rows(got, ref, P, pw=1.0):
    """Per row |got_i0 - ref_i0| / (pw (a_i + p/2 + a_i |w_i|^2 / 2)); with
    pw = 0 both sides are zero: 0 where the value is exactly 0, inf elsewhere."""
    p = P.W.shape[1]
    num = np.abs(np.asarray(got, np.float64)[:, 0] - ref[:, 0])
    den = abs(pw) * (P.a + 0.5 * p + 0.5 * P.a * (P.W * P.W).sum(1))
    out = np.where(num == 0.0, 0.0, np.inf)
    np.divide(num, den, out=out, where=den > 0)
    return out


def whole_rows(got, ref):
    """test_gpu_range.row_err: |got_i - ref_i|_2 / |ref_i|_2."""
    num = np.sqrt(((np.asarray(got, np.float64) - ref) ** 2).sum(1))
    return num / np.maximum(np.sqrt((ref ** 2).sum(1)), 1e-300)


Checked = collections.namedtuple(
    "Checked", "X xd t P ref rows absg a32 c32 ratio sens skipped draw")


def mutations(c):
    """(applicable, skipped-by-rule) mutation names of a case."""
    want = ["row", "col"] + (["label"] if c.labels == "gen" else [])
    skip = [m for m in want if (m == "row" and c.N == 1) or (m == "col" and c.p == 1)]
    return [m for m in want if m not in skip], skip


def preconditions(c, row_tol, draw=0):
    """Builds the case's inputs (its draw-th seed) and its fp64 reference and
    asserts (a) - (c).  Returns Checked: rows = the rows held to the data-row
    measure, absg = |G| |Xd| (only where a row is not), a32 / c32 the float32
    restatement's two figures, ratio (b), sens the smallest mutation change /
    row_tol."""
    X, xd, t = inputs(c, draw)
    P = parts(X, xd, t)
    ref = compose(P, c.pw)
    oracle = O.score_logreg(X, xd, t)                 # the project's fp64 oracle, pw = 1
    mine = compose(P, 1.0)
    assert np.abs(mine - oracle).max() <= 1e-12 * max(1.0, np.abs(oracle).max()), case_id(c)
    S32 = restate32(X, xd, t, c.pw).astype(np.float64)
    assert np.isfinite(S32).all(), case_id(c)
    c32 = col0_rows(S32, ref, P, c.pw)
    assert c32.max() <= COL0_PRE, ("(a) column 0", case_id(c), c32.max())
    rows = np.ones(c.n, bool)
    if c.variant == "wellfit":
        a32 = whole_rows(S32, ref)
        assert a32.max() <= row_tol / 10, ("(a) whole row", case_id(c), a32.max())
        return Checked(X, xd, t, P, ref, rows, None, float(a32.max()), float(c32.max()), None,
                       None, ["row", "col"], draw)
    a32 = data_rows(S32, ref, P.g)
    ratio = (c.pw * P.a * np.sqrt((P.W ** 2).sum(1))) / np.sqrt((P.g ** 2).sum(1))
    if c.variant == "sat":
        assert np.abs(P.Z[1]).max() > 88 and np.abs(P.Z[2]).max() > 1000, ("sat", case_id(c))
        rows[2] = a32[2] <= row_tol / 10 and ratio[2] <= PRIOR_RATIO   # the x1000 row alone
    if c.p == 1:
        rows = a32 <= row_tol / 10                    # by rule: see the module docstring
    assert a32[rows].max(initial=0.0) <= row_tol / 10, ("(a) data rows", case_id(c), a32[rows].max())
    assert ratio[rows].max(initial=0.0) <= PRIOR_RATIO, ("(b)", case_id(c), ratio[rows].max())
    absg = None if rows.all() else np.abs(P.G) @ np.abs(np.asarray(xd, np.float64))
    todo, skipped = mutations(c)
    sens = float("inf")
    live = rows if rows.any() else np.ones(c.n, bool)
    for m in todo:
        if m == "row":
            g2 = P.g - P.G[:, -1:] * np.asarray(xd[-1], np.float64)[None, :]
        elif m == "col":
            g2 = parts(X, xd, t, zcols=c.p - 1).g
        else:
            q = int(np.abs(t).argmax())
            t2 = np.array(t, np.float64)
            t2[q] = np.sign(t2[q])
            gq = t2[q] * O._sigmoid(-t2[q] * P.Z[:, q])
            g2 = P.g + (gq - P.G[:, q])[:, None] * np.asarray(xd[q], np.float64)[None, :]
        change = (np.sqrt(((g2 - P.g) ** 2).sum(1)) / np.sqrt((P.g ** 2).sum(1)))[live].max()
        assert change >= SENS * row_tol, ("(c) insensitive inputs", case_id(c), m, change)
        sens = min(sens, change / row_tol)
    return Checked(X, xd, t, P, ref, rows, absg, float(a32[rows].max(initial=0.0)),
                   float(c32.max()), float(ratio[rows].max(initial=0.0)), sens, skipped, draw)


@functools.lru_cache(maxsize=8)
def checked(c, row_tol):
    """The case's inputs: the first of its DRAWS seeds whose inputs meet the
    preconditions (which see fp64 and numpy float32 only, never the code under
    test), shared between the tests of one case, read only.  A label near 0
    on the dropped row, |z| peaking at 950 on the x1000 row, a weight near 0
    in the dropped column: the recipe leaves these to the seed."""
    first = None
    for draw in range(DRAWS):
        try:
            out = preconditions(c, row_tol, draw)
        except AssertionError as e:
            first = first or e
            continue
        for a in (out.X, out.xd, out.t, out.ref, out.P.g):
            a.setflags(write=False)
        return out
    raise first


# --------------------------------------------- predict, Gaussian, mixture --
PREDICT_N = (1, 127, 128, 129, 300)
PREDICT_P = (1, 31, 32, 33, 255, 1023)


def predict_cases():
    """(n, Nt, p) pairs: every value of each axis at least twice."""
    return [(PREDICT_N[i % 5], PREDICT_N[(2 * i + 1) % 5], PREDICT_P[i % 6]) for i in range(12)]


def predict_inputs(n, Nt, p, big=False):
    rs = np.random.RandomState(9000 + 7 * n + 3 * Nt + p)
    X = np.empty((n, p + 1), F32)
    X[:, 1:] = 0.3 * rs.randn(n, p)
    X[:, 0] = rs.uniform(-3.0, -1.0, n)
    if big:
        X[1, 1:] *= F32(1000.0)
        X[n // 2, 1:] *= F32(1000.0)
    xt = (rs.randn(Nt, p) / np.sqrt(p)).astype(F32)
    return X, xt


ELEMENTWISE_SHAPES = ((1, 1), (3, 5), (17, 15), (256, 1), (257, 3))
GMM_SPECIALS = (0.0, 2.0, -2.0, 1e-3, -1e-3, 10.0, -10.0, 50.0, -50.0)


def gaussian_inputs(n, d):
    """lam spans 2^-10 .. 2^10; every other entry x = mu (1 + 2^-20), so that
    x - mu cancels 20 bits."""
    rs = np.random.RandomState(100 * n + d)
    lam = (2.0 ** (-10.0 + 20.0 * np.arange(d) / max(d - 1, 1))).astype(F32)
    if d == 1:
        lam[0] = F32(2.0 ** (10 if n > 1 else -10))
    mu = (3.0 * rs.randn(d) + 0.1).astype(F32)
    X = (5.0 * rs.randn(n, d)).astype(F32)
    near = (mu.astype(np.float64) * (1.0 + 2.0 ** -20)).astype(F32)
    jj, cc = np.meshgrid(np.arange(n), np.arange(d), indexing="ij")
    X = np.where((jj + cc) % 2 == 0, near[None, :], X).astype(F32)
    return X, mu, lam


def gaussian_bound(X, mu, lam, scale):
    return 2.0 ** -22 * abs(scale) * np.abs(lam.astype(np.float64))[None, :] * (
        np.abs(X.astype(np.float64)) + np.abs(mu.astype(np.float64))[None, :])


def gmm_inputs(n, d):
    rs = np.random.RandomState(200 * n + d)
    X = (3.0 * rs.randn(n * d)).astype(F32)
    k = min(len(GMM_SPECIALS), n * d)
    X[:k] = np.asarray(GMM_SPECIALS[:k], F32)
    return X.reshape(n, d)


def gmm_bound(X, scale):
    return 1e-5 * abs(scale) * (np.abs(X.astype(np.float64)) + 2.0)
