"""CPU checks of tests/select_reference.py: the plain select is right on small
multisets, the buffer builders round-trip, and every table case has the
property it is named for (so a GPU test that uses it tests what it says)."""
import numpy as np
import pytest

import select_reference as R


def test_keys_are_monotone_for_non_negative_values():
    v = np.array([0.0, 1e-45, 1e-38, 0.5, 1.0, 2.205, 3e38, np.inf], dtype=np.float32)
    k = R.keys(v)
    assert k.dtype == np.uint32 and np.all(np.diff(k.astype(np.int64)) > 0)
    assert k[-1] == R.INF_KEY and R.keys(np.float32(np.nan))[0] > R.INF_KEY
    assert R.bits(R.from_bits(0x40123456)) == 0x40123456


@pytest.mark.parametrize("seed", range(6))
def test_weighted_kth_equals_partition_of_repeated_array(seed):
    rs = np.random.RandomState(seed)
    n = int(rs.randint(1, 40))
    v = rs.choice(np.array([0.0, 1e-40, 0.3, 0.3, 2.0, 2.205, 17.0, 3e38], np.float32), size=n)
    w = rs.randint(0, 4, size=n)
    w[int(rs.randint(n))] = 2
    rep = np.repeat(v, w)
    for k in range(len(rep)):
        want = np.partition(rep, k)[k]
        assert R.bits(R.weighted_kth(v, w, k)) == R.bits(want), k
    with pytest.raises(AssertionError):
        R.weighted_kth(v, w, len(rep))


def test_weighted_kth_skips_inf_and_nan():
    v = np.array([np.inf, 3.0, np.nan, 1.0, 2.0], np.float32)
    assert [float(R.weighted_kth(v, 1, k)) for k in range(3)] == [1.0, 2.0, 3.0]


@pytest.mark.parametrize("seed", range(4))
def test_digit_hist_three_passes_find_the_kth(seed):
    """digit_hist + pick, chained, is a radix select: the same answer as the
    sort (the reference is consistent with itself)."""
    rs = np.random.RandomState(seed)
    v = np.abs(rs.randn(500)).astype(np.float32) * np.float32(10.0 ** rs.randint(-3, 3))
    v[::37] = np.inf
    w = rs.randint(0, 3, size=v.size)
    ks = R.keys(v)
    total = int(w[ks < R.INF_KEY].sum())
    for k in (0, total // 2, total - 1):
        prefix, kk = 0, k
        for pas in (1, 2, 3):
            h = R.digit_hist(ks, pas, prefix, w)
            assert h.sum() <= total and (pas > 1 or h.sum() == total)
            dig, kk = R.pick(h, kk)
            prefix |= dig << R.SHIFT[pas]
        assert prefix == R.bits(R.weighted_kth(v, w, k))


def test_digit_hist_counts_by_hand():
    ks = np.array([R.bits(2.0), R.bits(2.0) + 1, R.bits(2.0) + (1 << 10), R.bits(4.0), R.INF_KEY,
                   R.INF_KEY + 1, 0x80000000], np.uint32)
    h1 = R.digit_hist(ks, 1)
    assert h1.sum() == 4 and h1[R.bits(2.0) >> 21] == 3 and h1[R.bits(4.0) >> 21] == 1
    h2 = R.digit_hist(ks, 2, R.bits(2.0))
    assert h2.sum() == 3 and h2[0] == 2 and h2[1] == 1
    h3 = R.digit_hist(ks, 3, R.bits(2.0), weights=[2, 1, 5, 1, 1, 1, 1])
    assert h3.sum() == 3 and h3[0] == 2 and h3[1] == 1


def test_h_of():
    assert R.h_of(0.0, 100) == 1.0 and R.h_of(3.0, 1) == 1.0 and R.h_of(-1.0, 5) == 1.0
    assert R.h_of(2.0, 10) == 2.0 / np.log(10.0)
    assert R.ulps(np.float32(1.0), 1.0) == 0.0
    assert R.ulps(np.nextafter(np.float32(1.0), np.float32(2.0)), 1.0) == 1.0


@pytest.mark.parametrize("cap", [0, 4, 16])
def test_build_cand_round_trips(cap):
    rs = np.random.RandomState(cap)
    slots = [(rs.rand(c).astype(np.float32), bool(i % 2), None if i % 3 else c + i, 10 * i)
             for i, c in enumerate([0, 1, 3, 4, 5, 16, 17, 40])]
    buf, (below, ncand, over) = R.build_cand(slots, cap, poison=-5.0)
    ns = len(slots)
    assert buf.dtype == np.uint32 and buf.size == 2 * ns + ns * cap
    back = R.parse_cand(buf, ns, cap)
    b2 = c2 = o2 = 0
    for (vals, w2, decl, *rest), (bv, bw2, bdecl, bbelow) in zip(slots, back):
        want_decl = len(vals) if decl is None else decl
        assert (bw2, bdecl, bbelow) == (w2, want_decl, rest[0])
        st = min(len(vals), cap)
        assert np.array_equal(bv[:st], vals[:st])
        assert np.all(bv[st:] == np.float32(-5.0))       # declared beyond the data: poison
        b2 += (2 if w2 else 1) * bbelow
        c2 += (2 if w2 else 1) * bdecl
        o2 += bdecl > cap
    assert (below, ncand, over) == (b2, c2, o2)
    rebuilt, tot = R.build_cand(back, cap, poison=-5.0)
    assert np.array_equal(rebuilt, buf) and tot == (below, ncand, over)


def test_panel_fill_matches_the_engine_layout():
    """Entry (i, j) of the dense matrix sits at panel (i // 128, j // 16),
    row i % 128, column j % 16 (PhiEngine.dense_D's view)."""
    mp, npad = 256, 384
    tv = np.arange(6, dtype=np.float32).reshape(2, 3) + 1
    buf = R.panel_fill(mp, npad, tv)
    dense = buf.reshape(mp // 128, npad // 16, 128, 16).transpose(0, 2, 1, 3).reshape(mp, npad)
    assert np.array_equal(dense, np.kron(tv, np.ones((128, 128), np.float32)))
    w = R.panel_weights(mp, npad, [[0, 1, 2], [2, 0, 1]])
    assert w.shape == buf.shape and [int(w[buf == t].max()) for t in (1, 2, 3, 4, 5, 6)] == [0, 1, 2, 2, 0, 1]
    assert R.sym_tile_weights(3).tolist() == [[1, 2, 2], [0, 1, 2], [0, 0, 1]]


# ---- the tables ---------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(R.FLAT_FAMILIES))
@pytest.mark.parametrize("count", R.FLAT_COUNTS)
def test_flat_cases(family, count):
    v, fin = R.flat_case(family, count)
    assert v.dtype == np.float32 and v.size == count and fin[0]
    assert np.all(v[fin] >= 0)
    if count >= 4:
        assert np.isposinf(v).any() and np.isnan(v).any()
    ks = R.keys(v)[fin]
    d1, d2, d3 = ks >> 21, (ks >> 10) & 0x7FF, ks & 0x3FF
    if family == "all_equal":
        assert len(np.unique(ks)) == 1
    elif family == "digit3_only":
        assert len(np.unique(d1)) == 1 and len(np.unique(d2)) == 1
        assert count < 1000 or len(np.unique(d3)) > 500
    elif family == "digit2_only":
        assert len(np.unique(d1)) == 1 and len(np.unique(d3)) == 1
        assert count < 1000 or len(np.unique(d2)) > 300
    elif family == "octaves" and count > 100000:
        assert ks.min() == 1 and ks.max() == R.bits(R.FLT_MAX) and len(np.unique(ks >> 23)) == 255
    elif family == "zeros_denormals" and count > 1000:
        assert ks.max() < (1 << 23) and (ks == 0).sum() > count // 4
    ranks = R.flat_ranks(int(fin.sum()))
    assert ranks[0] == 0 and ranks[-1] == int(fin.sum()) - 1


def test_pick_cases_sit_at_the_ends_of_their_bins():
    cases = R.pick_cases()
    assert len(cases) == 30
    for pas, b, k in cases:
        h = R.pick_hist(pas)
        assert h[b] == R.BIG > (1 << 32) and np.all(h[R.MASK[pas] + 1:] == 0)
        dig, rem = R.pick(h, k)
        assert dig == b and rem in (0, R.BIG - 1)
    # bins either side of a thread boundary and of a wave boundary, and the last
    for pas, per in ((1, 8), (2, 8), (3, 4)):
        bins = R.PICK_BINS[pas]
        assert bins[0] // per != bins[1] // per and bins[1] - bins[0] == 1
        assert bins[2] // per == 63 and bins[3] // per == 64 and bins[4] == R.MASK[pas]


def test_brackets():
    lo, hi = R.BRACKETS["shared"]
    assert lo < hi and R.bits(lo) >> 21 == R.bits(hi) >> 21
    lo, hi = R.BRACKETS["straddle"]
    assert lo < hi and R.bits(lo) >> 21 != R.bits(hi) >> 21
    lo, hi = R.BRACKETS["point"]
    assert lo == hi
    for name, (lo, hi) in R.BRACKETS.items():
        v = R.bracket_values(name, 100, np.random.RandomState(0))
        assert np.all((v >= lo) & (v <= hi)) and v[0] == lo and v[-1] == hi


@pytest.mark.parametrize("name", sorted(R.decision_cases()))
def test_decision_cases(name):
    kind, slots, cap, k, tot = R.decision_case(name)
    below, ncand, over = tot
    if kind == "holds":
        assert over == 0 and below <= k < below + ncand
    else:
        assert not R.bracket_holds(k, tot)
    if kind == "miss-low":
        assert k == below - 1 and over == 0
    if kind == "miss-high":
        assert k == below + ncand and over == 0
    if kind == "overflow":
        assert over == 1 and below <= k < below + ncand      # only the overflow refuses it
        assert max(s[2] for s in slots) == cap + 1
    if name == "holds_at_cap":
        assert [s[2] for s in slots] == [cap]
    if name == "holds_first":
        assert k == below
    if name == "holds_last":
        assert k == below + ncand - 1
    assert any(s[1] for s in slots) or len(slots) == 1       # weight-2 slots are mixed in


def test_totals_and_walk_tables():
    for ns in R.TOTALS_NSLOTS:
        slots, cap = R.totals_slots(ns)
        assert len(slots) == ns
    slots, cap = R.totals_slots(65537)
    assert any(s[1] for s in slots) and any(not s[1] for s in slots)
    for cap in R.WALK_CAPS:
        for br in ("shared", "straddle"):
            slots = R.walk_slots(37, cap, br)
            decl = {s[2] for s in slots}
            assert {0, 1, 63, 64, 255, 256, 257, cap, cap + 3} <= decl
            assert all(len(s[0]) == min(s[2], cap) for s in slots)
            assert any(s[1] for s in slots)
            v, w = R.cand_multiset(slots, cap)
            lo, hi = R.BRACKETS[br]
            assert np.all((v >= lo) & (v <= hi)) and set(w.tolist()) == {1, 2}
    assert R.walk_slots(1, 4, "shared")[0][2] > 0            # a single slot is not empty


@pytest.mark.parametrize("kind", R.SAMPLE_KINDS)
@pytest.mark.parametrize("s", R.SAMPLE_SIZES)
def test_sample_cases(kind, s):
    v, ranks = R.sample_case(kind, s)
    assert v.dtype == np.float32 and v.size == s and s % 4 == 0
    assert np.all(np.isfinite(v)) and np.all(v >= 0)
    for klo, khi in ranks:
        assert 0 <= klo <= khi < s
    assert (0, s - 1) in ranks
    assert any(a == b for a, b in ranks) or kind in ("two_values", "two_octaves")
    srt = np.sort(v)
    if kind == "two_values":
        assert len(np.unique(v)) == 2
    if kind in ("two_values", "two_octaves"):
        klo, khi = ranks[0]
        assert R.bits(srt[klo]) >> 23 != R.bits(srt[khi]) >> 23     # different octaves
        assert khi == klo + 1
    if kind == "wave_mix" and s >= 1024:
        k = R.keys(v)
        assert len(np.unique(k[:256])) == 1
        assert len(np.unique(k[256:512:4] >> 21)) == 64             # 64 lanes, 64 digit-1 bins
        assert len(np.unique(k[512:768] >> 21)) == 1 and len(np.unique((k[512:768:4] >> 10) & 0x7FF)) == 64
        assert len(np.unique(k[768:1024] >> 10)) == 1 and len(np.unique(k[768:1024:4] & 0x3FF)) == 64


def test_equidistant_set_sits_inside_one_digit1_bin():
    """Every off-diagonal fp64 distance of x_i = 1.05 e_i lies at least 5 % of
    the bin's width inside one digit-1 bin (four bins per octave), so fp32
    rounding of the Gram cannot move an entry to a neighbour bin."""
    X = R.equidistant(40, 64).astype(np.float64)
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    off = D[~np.eye(40, dtype=bool)]
    b = R.bits(off[0]) >> 21
    lo, hi = float(R.from_bits(b << 21)), float(R.from_bits((b + 1) << 21))
    assert np.all(off >= lo + 0.05 * (hi - lo)) and np.all(off <= hi - 0.05 * (hi - lo))
    assert abs(off[0] - 2.205) < 1e-6 and np.all(np.diag(D) == 0)


def test_particle_sets():
    cases = R.gram_cases()
    assert {(n, d) for _, n, d in cases} == {(n, d) for n in R.GRAM_NS for d in {3, 65, 256, n}}
    for kind in ("identical", "equidistant", "clusters", "lattice"):
        assert {n for k, n, d in cases if k == kind} == set(R.GRAM_NS)
    n, d = 200, 65
    X = R.particle_set("clusters", n, d).astype(np.float64)
    D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1).ravel()
    srt = np.sort(D)
    k = (n * n - 1) // 2
    assert srt[k] < 1e-2 and srt[k + 1] > 100.0          # the lower median is the last small one
    L = R.particle_set("lattice", n, 3)
    assert len(np.unique(L, axis=0)) <= 27                # massive ties
    assert np.all(R.particle_set("identical", n, d) == 1)
