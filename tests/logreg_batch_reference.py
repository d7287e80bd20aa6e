"""fp64 references of the minibatch logistic-regression score (numpy), shared
by tests/test_logreg_batch_host.py and tests/test_gpu_logreg_batch.py.

Over the cyclic window rows (c + q) mod N, q < B, with w = N / B, in the
pieces of tests/score_cases.py (parts / compose) on the window's rows:

    S[:, 1:] = w g - a W,    g = G Xd_b,  G_iq = t_q sigma(-t_q w_i . xd_q)
    S[:, 0]  = -a + p/2 - a |w|^2 / 2

The data-row measure is taken against the weighted data term, w |g_i|.

The kernel cases are score_cases cases whose "N" is the window length B: the
window's rows pass score_cases.checked, the other 2B + 7 rows of the data hold
1e3 randn with labels +-1 -- any of them read by mistake moves a row of S far
past the bound (asserted, `extra_row_change`).  |z| is in the hundreds on such
a row, so sigma(-t z) is 0 or 1 to the last bit: with a random label half of
the rows would add exactly nothing to a particle, and a one-particle case
could not see them.  The label is therefore the one the FIRST particle gets
wrong, t = -sign(xd . w_0): sigma is 1 there and the row's term is t xd.
"""
import functools

import numpy as np

import score_cases as SC

F32 = np.float32
SHAPES = [(1, 1, 33), (1, 100, 255), (33, 32, 32), (33, 33, 33), (64, 100, 255), (65, 31, 256),
          (65, 64, 128), (257, 257, 255), (129, 100, 1023), (64, 100, 1), (300, 1000, 255)]
# the dispatch edges of csrc/logreg_window.hip beyond the table above: the
# last n of the one-particle form and the first of the tile form, its 256-row
# chunk edge, and a second column slab that is not full
EXTRA_SHAPES = [(16, 33, 33), (17, 33, 33), (3, 257, 40), (40, 33, 257)]
LABELS = ("pm1", "gen")


def window_case(n, B, p, labels, **kw):
    return SC.case("W", "window", n, B, p, labels, **kw)


def table(shapes=None):
    return [window_case(n, B, p, lab) for n, B, p in (shapes or SHAPES + EXTRA_SHAPES)
            for lab in LABELS]


def data_rows_total(B):
    return 3 * B + 7


def origins(B):
    """0, the window that ends on the last row, the one that wraps by one row
    and the one with all but one row wrapped."""
    N = data_rows_total(B)
    return [0, N - B, N - B + 1, N - 1]


def window(N, B, c):
    return (int(c) + np.arange(B)) % N


# ------------------------------------------------------------ the score --
def window_score64(X, xd, t, B, c):
    """(S, P, w): the fp64 estimate over the window (c, B) of the data
    (xd, t), the pieces of its rows and the weight N / B."""
    xd, t = np.asarray(xd), np.asarray(t)
    N = xd.shape[0]
    rows = window(N, B, c)
    w = N / B
    P = SC.parts(X, xd[rows], t[rows])
    return compose_weighted(P, w), P, w


def compose_weighted(P, w):
    S = SC.compose(P)
    S[:, 1:] = w * P.g - P.a[:, None] * P.W
    return S


def window_score_fn(xd, t, B):
    """score_fn(X, it): iteration it's estimate, window origin (it B) mod N."""
    N = np.asarray(xd).shape[0]
    return lambda X, it: window_score64(X, xd, t, B, (it * B) % N)[0]


class RankScores(object):
    """Per-rank score functions for oracle.DistOracle, which calls score_fn(X)
    without an iteration: the test sets `.it` before each step."""

    def __init__(self, shards, B):
        self.it = 0
        self.fns = [self._fn(window_score_fn(xd, t, B)) for xd, t in shards]

    def _fn(self, fn):
        return lambda X: fn(X, self.it)


def restate32_window(X, xd, t, w, block=32):
    """score_cases.restate32 with the data term weighted w, float32 throughout
    (the window summed in chunks of 32 rows whose partial sums are added)."""
    X, xd, t = np.asarray(X, F32), np.asarray(xd, F32), np.asarray(t, F32)
    a, W = np.exp(X[:, 0]), X[:, 1:]
    p = W.shape[1]
    with np.errstate(over="ignore"):
        G = t[None, :] / (F32(1.0) + np.exp(t[None, :] * (W @ xd.T)))
    nb = -(-xd.shape[0] // block)
    part = np.empty((X.shape[0], p, nb), F32)
    for b in range(nb):
        part[:, :, b] = G[:, b * block:(b + 1) * block] @ xd[b * block:(b + 1) * block]
    S = np.empty_like(X)
    S[:, 1:] = F32(w) * part.sum(-1) - a[:, None] * W
    S[:, 0] = -a + F32(0.5 * p) - F32(0.5) * a * (W * W).sum(1)
    assert S.dtype == F32
    return S


def weighted_rows(got, ref, g, w):
    """Per row |got_i[1:] - ref_i[1:]|_2 / (w |g_i|_2)."""
    return SC.data_rows(got, ref, g) / w


# ------------------------------------------------------------ the cases --
def filler(c, k, rows):
    """The data rows outside the window: 1e3 randn, labels +-1 (the label
    particle 0 gets wrong: see the module docstring)."""
    rs = np.random.RandomState(SC.seed_of(c) ^ 0x33cc33)
    xd = (1e3 * rs.randn(rows, c.p)).astype(F32)
    z0 = xd.astype(np.float64) @ k.P.W[0]
    t = np.where(z0 > 0, -1.0, 1.0).astype(F32)
    return xd, t


def place(c, k, origin):
    """The N = 3B + 7 data rows with the checked rows in the window at `origin`."""
    B = c.N
    N = data_rows_total(B)
    xd, t = filler(c, k, N)
    rows = window(N, B, origin)
    xd[rows], t[rows] = k.xd, k.t
    return xd, t


def extra_row_change(c, k):
    """The smallest, over the filler rows (each lies outside the window at
    some origin), of the largest change of the data-row measure when that row
    joins the sum (its term weighted like the others, so the weight cancels)."""
    xd, t = filler(c, k, data_rows_total(c.N))
    xd, t = xd.astype(np.float64), t.astype(np.float64)
    from oracle import svgd_oracle as O
    G = t[None, :] * O._sigmoid(-t[None, :] * (k.P.W @ xd.T))        # (n, rows)
    gn = np.sqrt((k.P.g ** 2).sum(1))
    live = k.rows if k.rows.any() else np.ones(c.n, bool)
    change = np.abs(G) * np.sqrt((xd * xd).sum(1))[None, :] / np.maximum(gn, 1e-300)[:, None]
    return float(change[live].max(0).min())


@functools.lru_cache(maxsize=4)
def checked(c, row_tol):
    """(k, ref, w, rows, absg, a32): the case through score_cases.checked (its
    preconditions (a) - (c) on the window's rows), the weighted reference, and
    the two preconditions asserted anew with the weight: the float32
    restatement under row_tol / 10 on the weighted measure (p = 1: per row,
    by score_cases' rule), and every row outside the window moving the
    measure by SENS row_tol if it joined the sum."""
    k = SC.checked(c, row_tol)
    w = data_rows_total(c.N) / c.N
    ref = compose_weighted(k.P, w)
    S32 = restate32_window(k.X, k.xd, k.t, w).astype(np.float64)
    assert np.isfinite(S32).all(), SC.case_id(c)
    a32 = weighted_rows(S32, ref, k.P.g, w)
    rows = np.array(k.rows)
    if c.p == 1:
        rows &= a32 <= row_tol / 10
    assert a32[rows].max(initial=0.0) <= row_tol / 10, ("(a) weighted", SC.case_id(c), a32[rows].max())
    absg = None if rows.all() else np.abs(k.P.G) @ np.abs(np.asarray(k.xd, np.float64))
    change = extra_row_change(c, k)
    assert change >= SC.SENS * row_tol, ("extra row", SC.case_id(c), change)
    ref.setflags(write=False)
    return k, ref, w, rows, absg, float(a32[rows].max(initial=0.0)), change


# ------------------------------------------------------- trajectories --
def sorted_problem(N, p, seed, spread=3.0):
    """(xd, t) float32 for the sampler tests: rows spread randn / sqrt(p),
    labels from a true direction with logistic noise, the rows SORTED along
    the noisy margin -- a window then holds one end of the data, and a run
    whose window stands still, or that scores all of the data, leaves the
    minibatch trajectory far behind."""
    rs = np.random.RandomState(seed)
    ws = rs.randn(p)
    x = spread * rs.randn(N, p) / np.sqrt(p)
    m = x @ ws + 0.3 * rs.logistic(size=N)
    o = np.argsort(m)
    return x[o].astype(F32), np.where(m[o] > 0, 1.0, -1.0).astype(F32)
