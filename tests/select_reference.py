"""The plain side of the exact median select (csrc/select.hip, select.hpp):
numpy, integers and fp64 only.  Keys are the uint32 bit patterns of fp32
values (monotone for values >= 0); a radix pass histograms one digit of the
keys below +inf whose higher digits equal the prefix; the k-th order statistic
is a sort and a cumulative sum.  Also the builders of the hand-made buffers
the GPU tests feed the kernels (candidate slots, panel-layout tiles) and the
seeded case tables shared by test_select_host.py and
test_gpu_select_kernels.py.
"""
import math

import numpy as np

NBINS = 2048
INF_KEY = 0x7F800000            # +inf; NaNs and negative values have larger keys
WEIGHT2 = 0x80000000            # DSVGD_SLOT_WEIGHT2
SHIFT = {1: 21, 2: 10, 3: 0}
MASK = {1: 0x7FF, 2: 0x7FF, 3: 0x3FF}
HISHIFT = {1: 32, 2: 21, 3: 10}
PANEL = 2048                    # floats of one 128 x 16 panel
FLT_MAX = np.float32(3.4028234663852886e38)
DENORM_MIN = np.float32(1.401298464324817e-45)


def keys(x):
    """fp32 values viewed as uint32 (flattened)."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).ravel()


def bits(v):
    return int(np.float32(v).view(np.uint32))


def from_bits(k):
    return np.uint32(k).view(np.float32)


def digit_hist(ks, pas, prefix=0, weights=None):
    """int64[2048] histogram of digit `pas` (1, 2, 3) of the keys < +inf whose
    higher digits equal those of `prefix`; weights: non-negative integers."""
    ks = np.asarray(ks, dtype=np.uint32).astype(np.int64)
    ok = ks < INF_KEY
    if pas > 1:
        ok &= (ks >> HISHIFT[pas]) == (int(prefix) >> HISHIFT[pas])
    dig = (ks >> SHIFT[pas]) & MASK[pas]
    out = np.zeros(NBINS, dtype=np.int64)
    if weights is None:
        out += np.bincount(dig[ok], minlength=NBINS)
        return out
    w = np.broadcast_to(np.asarray(weights, dtype=np.int64), ks.shape)
    for u in np.unique(w):
        if u:
            out += int(u) * np.bincount(dig[ok & (w == u)], minlength=NBINS)
    return out


def pick(hist, k):
    """(digit, remaining rank) of rank k in a histogram (Python integers)."""
    run = 0
    for b, c in enumerate(int(x) for x in hist):
        if k < run + c:
            return b, k - run
        run += c
    raise ValueError("rank %d past the histogram's %d entries" % (k, run))


def weighted_kth(values, weights, k):
    """The k-th (0-based) order statistic of the multiset holding values[i]
    weights[i] times, over the finite non-negative entries (keys < +inf)."""
    v = np.ascontiguousarray(values, dtype=np.float32).ravel()
    w = np.broadcast_to(np.asarray(weights, dtype=np.int64), v.shape)
    ks = v.view(np.uint32)
    ok = (ks < INF_KEY) & (w > 0)
    ks, w = ks[ok], w[ok]
    order = np.argsort(ks, kind="stable")
    cum = np.cumsum(w[order])
    assert 0 <= k < int(cum[-1]), (k, int(cum[-1]))
    return from_bits(ks[order][int(np.searchsorted(cum, k, side="right"))])


def h_of(med, n_total):
    """The bandwidth rule in fp64: 1 if med <= 0 or n_total <= 1."""
    med = float(med)
    if not med > 0.0 or n_total <= 1:
        return 1.0
    return med / math.log(float(n_total))


def ulps(got32, want64):
    """|got - want| in units of the fp32 spacing at want."""
    want64 = float(want64)
    return abs(float(got32) - want64) / float(np.spacing(np.float32(abs(want64))))


# ---- buffers ----------------------------------------------------------------
def build_cand(slots, cap, poison=0.0):
    """The candidate buffer of include/dsvgd.h as uint32 words: nslots counts
    (bit 31 = weight 2), nslots belows, then cap floats per slot.  A slot is
    (values, weight2, declared_count[, below]): values[:cap] are stored (the
    kernels never read past cap; the rest of the slot holds `poison`),
    declared_count (None: len(values)) goes to the count word.
    Returns (words, (below_total, ncand_total, overflow))."""
    ns = len(slots)
    buf = np.empty(2 * ns + ns * cap, dtype=np.uint32)
    data = buf[2 * ns:].view(np.float32).reshape(ns, cap) if cap else None
    if cap:
        data[:] = np.float32(poison)
    below_t = ncand_t = over = 0
    for s, slot in enumerate(slots):
        vals, w2, decl = slot[0], bool(slot[1]), slot[2]
        below = int(slot[3]) if len(slot) > 3 else 0
        vals = np.asarray(vals, dtype=np.float32).ravel()
        decl = len(vals) if decl is None else int(decl)
        assert 0 <= decl < WEIGHT2 and 0 <= below < (1 << 32)
        buf[s] = decl | (WEIGHT2 if w2 else 0)
        buf[ns + s] = below
        st = min(len(vals), cap)
        if st:
            data[s, :st] = vals[:st]
        w = 2 if w2 else 1
        below_t += w * below
        ncand_t += w * decl
        over += 1 if decl > cap else 0
    return buf, (below_t, ncand_t, over)


def parse_cand(buf, ns, cap):
    """Inverse of build_cand: [(stored values, weight2, declared, below)]."""
    buf = np.asarray(buf, dtype=np.uint32)
    data = buf[2 * ns:2 * ns + ns * cap].view(np.float32).reshape(ns, cap) if cap else None
    out = []
    for s in range(ns):
        decl = int(buf[s] & (WEIGHT2 - 1))
        st = min(decl, cap)
        vals = data[s, :st].copy() if cap else np.zeros(0, np.float32)
        out.append((vals, bool(buf[s] & WEIGHT2), decl, int(buf[ns + s])))
    return out


def cand_multiset(slots, cap):
    """(values, weights) the select passes must see: the first min(declared,
    len, cap) values of every slot, weight 1 or 2."""
    vs, ws = [], []
    for slot in slots:
        vals = np.asarray(slot[0], dtype=np.float32).ravel()
        decl = len(vals) if slot[2] is None else int(slot[2])
        st = min(decl, cap, len(vals))
        vs.append(vals[:st])
        ws.append(np.full(st, 2 if slot[1] else 1, dtype=np.int64))
    if not vs:
        return np.zeros(0, np.float32), np.zeros(0, np.int64)
    return np.concatenate(vs), np.concatenate(ws)


def panel_fill(m_pad, n_pad, tile_value):
    """A panel-layout m_pad x n_pad buffer (128 x 16 panels, row-major inside)
    holding tile_value[I][J] in every entry of the 128 x 128 tile (I, J)."""
    tv = np.asarray(tile_value, dtype=np.float32)
    assert m_pad % 128 == 0 and n_pad % 128 == 0 and tv.shape == (m_pad // 128, n_pad // 128)
    buf = np.empty((m_pad // 128, n_pad // 16, PANEL), dtype=np.float32)
    buf[:] = np.repeat(tv, 8, axis=1)[:, :, None]
    return buf.ravel()


def panel_weights(m_pad, n_pad, tile_weight):
    """Per-entry integer weights in panel_fill's order."""
    tw = np.asarray(tile_weight, dtype=np.int64)
    buf = np.empty((m_pad // 128, n_pad // 16, PANEL), dtype=np.int64)
    buf[:] = np.repeat(tw, 8, axis=1)[:, :, None]
    return buf.ravel()


def sym_tile_weights(T):
    """The symmetric layout's rule: 0 below the diagonal, 1 on it, 2 above."""
    I, J = np.indices((T, T))
    return np.where(J < I, 0, np.where(J == I, 1, 2)).astype(np.int64)


# ---- case tables --------------------------------------------------------------
FLAT_COUNTS = (1, 3, 4, 5, 1023, 1027, 4 * 256 * 4096 + 7)


def _octaves(count, rs):
    # one value per octave from the smallest denormal to FLT_MAX: 2^-149 .. 2^127
    # (and FLT_MAX itself), cycled
    e = np.arange(-149, 128)
    v = np.concatenate([np.ldexp(1.0, e), [float(FLT_MAX)]]).astype(np.float32)
    return v[rs.randint(0, len(v), size=count)]


def _digit3(count, rs):
    # one digit-1 / digit-2 prefix, the low 10 bits vary
    return (np.uint32(bits(3.0)) | rs.randint(0, 1 << 10, size=count).astype(np.uint32)).view(np.float32)


def _digit2(count, rs):
    # one digit 1 and one digit 3, bits 20..10 vary
    k = np.uint32(bits(0.75) | 0x155) | (rs.randint(0, 1 << 11, size=count).astype(np.uint32) << 10)
    return k.astype(np.uint32).view(np.float32)


def _zeros_denormals(count, rs):
    k = rs.randint(0, 1 << 23, size=count).astype(np.uint32)   # denormal keys (0 = zero)
    k[rs.rand(count) < 0.5] = 0
    return k.view(np.float32)


FLAT_FAMILIES = {
    "all_equal": lambda count, rs: np.full(count, 2.205, dtype=np.float32),
    "two_values": lambda count, rs: np.where(rs.rand(count) < 0.5, np.float32(0.3),
                                             np.float32(17.0)).astype(np.float32),
    "digit3_only": _digit3,
    "digit2_only": _digit2,
    "octaves": _octaves,
    "zeros_denormals": _zeros_denormals,
}


def flat_case(family, count):
    """(values with +inf / NaN sprinkled in, finite mask).  At least one entry
    stays finite; counts below 4 get no specials beyond that rule."""
    rs = np.random.RandomState(1000 * sorted(FLAT_FAMILIES).index(family) + count % 9973)
    v = np.array(FLAT_FAMILIES[family](count, rs), dtype=np.float32)
    if count >= 3:
        nsp = max(2, count // 50)
        idx = rs.choice(count - 1, size=min(nsp, count - 1), replace=False) + 1   # entry 0 stays
        v[idx[0::2]] = np.inf
        v[idx[1::2]] = np.nan
    fin = keys(v) < INF_KEY
    return v, fin


def flat_ranks(c):
    return sorted({0, min(1, c - 1), (c - 1) // 2, c - 1})


# radix_pick on a hand-written histogram: bins either side of a thread boundary
# (8 bins per thread in passes 1 and 2, 4 in pass 3), of a wave boundary
# (thread 63 | 64) and the last bin
BIG = 3 * (1 << 32) + 5
PICK_BINS = {1: (7, 8, 511, 512, 2047), 2: (7, 8, 511, 512, 2047), 3: (3, 4, 255, 256, 1023)}
PICK_PREFIX = {1: 0, 2: bits(2.0) & 0xFFE00000, 3: (bits(2.0) & 0xFFE00000) | (0x2AB << 10)}


def pick_hist(pas):
    """A histogram with u64-sized counts in PICK_BINS[pas] and small counts in
    a few bins between them."""
    h = np.zeros(NBINS, dtype=np.int64)
    for b in PICK_BINS[pas]:
        h[b] = BIG
    for b in (0, 5, 9, 300, 600, 1000):
        if b <= MASK[pas] and h[b] == 0:
            h[b] = 3 + b
    return h


def pick_cases():
    """(pass, bin, k) with k the first and the last rank of the bin."""
    out = []
    for pas in (1, 2, 3):
        h = pick_hist(pas)
        for b in PICK_BINS[pas]:
            lo = int(h[:b].sum())
            out.append((pas, b, lo))
            out.append((pas, b, lo + int(h[b]) - 1))
    return out


# brackets: "shared" has bits(lo) >> 21 == bits(hi) >> 21, "straddle" does not
BRACKETS = {
    "shared": (np.float32(2.19), np.float32(2.23)),      # both in [2, 2.5)
    "straddle": (np.float32(1.98), np.float32(2.03)),    # across the octave boundary at 2
    "point": (np.float32(2.205), np.float32(2.205)),     # lo == hi
}


def bracket_values(name, count, rs):
    """count fp32 values in [lo, hi] of the bracket, both ends included."""
    lo, hi = BRACKETS[name]
    a, b = bits(lo), bits(hi)
    k = rs.randint(a, b + 1, size=count).astype(np.uint32)
    if count > 0:
        k[0] = a
    if count > 1:
        k[-1] = b
    return k.view(np.float32)


def _slots_for(counts, cap, seed, below=7):
    rs = np.random.RandomState(seed)
    return [(bracket_values("shared", min(c, cap), rs), bool(s % 3 == 1), c, below + s)
            for s, c in enumerate(counts)]


def decision_cases():
    """name -> (kind, slots, cap, rank offset): k = below_total + offset for
    offset >= 0, k = below_total + ncand_total + (offset + 1) for 'end'
    offsets, spelled out as a function of the totals."""
    cap = 16
    base = _slots_for([3, 0, 16, 5, 1], cap, seed=11)
    at_cap = _slots_for([16], cap, seed=12)
    over = _slots_for([3, 17, 2], cap, seed=13)
    return {
        "holds_first": ("holds", base, cap, lambda b, c: b),
        "holds_last": ("holds", base, cap, lambda b, c: b + c - 1),
        "miss_low": ("miss-low", base, cap, lambda b, c: b - 1),
        "miss_high": ("miss-high", base, cap, lambda b, c: b + c),
        "holds_at_cap": ("holds", at_cap, cap, lambda b, c: b + c // 2),
        "overflow": ("overflow", over, cap, lambda b, c: b + 1),
    }


def decision_case(name):
    """(kind, slots, cap, k, (below, ncand, overflow))."""
    kind, slots, cap, rank = decision_cases()[name]
    _, tot = build_cand(slots, cap)
    return kind, slots, cap, rank(tot[0], tot[1]), tot


def bracket_holds(k, totals):
    below, ncand, over = totals
    return over == 0 and below <= k < below + ncand


TOTALS_NSLOTS = (1, 5, 255, 256, 257, 65537)


def totals_slots(ns):
    """ns slots without data (cap 4): counts and belows only."""
    rs = np.random.RandomState(ns)
    cnt = rs.randint(0, 7, size=ns)
    bel = rs.randint(0, 100000, size=ns)
    w2 = rs.rand(ns) < 0.4
    empty = np.zeros(0, np.float32)
    return [(empty, bool(w2[s]), int(cnt[s]), int(bel[s])) for s in range(ns)], 4


# the walk over the candidate slots: 4096 waves, two slots per wave per trip
WALK_NSLOTS = (1, 2, 5, 4095, 4096, 4097, 8191, 8193, 12289)
WALK_CAPS = (4, 300)


def walk_slots(ns, cap, bracket):
    """ns slots with the per-slot counts 0, 1, 63, 64, 255, 256, 257, cap and
    a declared count above cap in turn (stored entries stop at cap), every
    third slot of weight 2."""
    rs = np.random.RandomState(7 * ns + cap)
    cyc = (257, 0, 1, 63, 64, 255, 256, cap, cap + 3)
    slots = []
    for s in range(ns):
        c = cyc[(s + s // len(cyc)) % len(cyc)]
        slots.append((bracket_values(bracket, min(c, cap), rs), s % 3 == 2, c))
    return slots


# sample selects
SAMPLE_SIZES = (4, 8, 1028, 4096, 1 << 16)


def sample_case(kind, s):
    """(sample, [(k_lo, k_hi), ...])."""
    rs = np.random.RandomState(s)
    mid = (s - 1) // 2
    ranks = [(mid, mid), (0, s - 1), (s // 4, (3 * s) // 4)]
    if kind == "all_equal":
        return np.full(s, 2.205, dtype=np.float32), ranks
    if kind == "two_values":
        # two values in different octaves, k_lo on the one and k_hi on the other:
        # the two selects want different digits in passes 2 and 3
        v = np.where(np.arange(s) % 2 == 0, np.float32(0.75), np.float32(12.0)).astype(np.float32)
        return v, [(s // 2 - 1, s // 2), (0, s - 1), (s // 4, (3 * s) // 4)]
    if kind == "two_octaves":
        # half in [0.5, 1), half in [8, 16): k_lo in the one, k_hi in the other
        lo = (np.uint32(bits(0.5)) + rs.randint(0, 1 << 23, size=s // 2).astype(np.uint32))
        hi = (np.uint32(bits(8.0)) + rs.randint(0, 1 << 23, size=s - s // 2).astype(np.uint32))
        v = np.concatenate([lo, hi]).astype(np.uint32).view(np.float32)
        v = v[rs.permutation(s)]
        return v, [(s // 2 - 1, s // 2), (0, s - 1), (s // 4, (3 * s) // 4)]
    assert kind == "wave_mix"
    # a wave reads 256 consecutive floats, lane l the four at 4 l: blocks of
    # 256 in turn all equal / 64 distinct digits 1 / one digit 1 and 64
    # distinct digits 2 / one digit 1 and 2 and 64 distinct digits 3
    a = bits(2.205)
    lane = np.repeat(np.arange(64, dtype=np.uint32), 4)
    blocks = [np.full(256, a, dtype=np.uint32),
              ((np.uint32(60) + lane) << 23).astype(np.uint32) | np.uint32(0x12345),
              (np.uint32(a & 0xFFE00000) | (lane * np.uint32(29) << 10) | np.uint32(a & 0x3FF)),
              (np.uint32(a & 0xFFFFFC00) | (lane * np.uint32(13)))]
    k = np.concatenate([blocks[(i // 256) % 4][:min(256, s - i)] for i in range(0, s, 256)])
    return k.astype(np.uint32).view(np.float32), ranks


SAMPLE_KINDS = ("all_equal", "two_values", "two_octaves", "wave_mix")


# degenerate particle sets for the fused accounting of the Gram kernels
def equidistant(n, d):
    assert d >= n
    X = np.zeros((n, d), dtype=np.float32)
    X[np.arange(n), np.arange(n)] = np.float32(1.05)
    return X


def particle_set(kind, n, d):
    rs = np.random.RandomState(n + 3 * d)
    if kind == "identical":
        return np.ones((n, d), dtype=np.float32)
    if kind == "equidistant":
        return equidistant(n, d)
    if kind == "clusters":
        # two tight clusters of n / 2: the n^2 / 2 within-cluster distances are
        # tiny, the rest about |c|^2, so the lower median sits at the gap
        X = (1e-3 * rs.randn(n, d)).astype(np.float32)
        X[n // 2:] += np.float32(2.0)
        return X
    assert kind == "lattice"
    return rs.randint(0, 3, size=(n, d)).astype(np.float32)


GRAM_NS = (200, 256, 384)


def gram_cases():
    """(kind, n, d): d in {3, 65, 256, n}; the equidistant set needs d >= n."""
    out = []
    for n in GRAM_NS:
        for d in sorted({3, 65, 256, n}):
            for kind in ("identical", "equidistant", "clusters", "lattice"):
                if kind == "equidistant" and d < n:
                    continue
                out.append((kind, n, d))
    return out
