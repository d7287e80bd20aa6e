"""The exact median select (csrc/select.hip, select.hpp and the accounting fused
into the distance epilogues of csrc/sqdist.hip) through the C ABI on
hand-built buffers, against the plain numpy select of select_reference.py.

What is held to what:
  * every histogram (st.hist after a dsvgd_radix_hist, the fused digit-1
    histogram of a distance launch) equals the integer recount, bin by bin;
  * every order statistic is bit-equal to the sort's;
  * h is within 1 fp32 ulp of fp64 median / log(n_total) (the device's fp64
    log may differ from numpy's in its last bits; the one rounding to fp32 can
    then land on the neighbour) and inv_h within 3 fp32 ulp of fp64 1 / h (the
    bound of a non-IEEE fp32 divide, 2.5 ulp, plus the rounding of the
    reference).  Both are checked where the median is a normal number in
    [1e-30, 1e30], so neither h nor 1 / h leaves the normal range.

Parts 1-6 use no engine and no distance kernel: state fields are written
through SelectState.buf with the offsets of engine._SelectState.  Part 7 runs
PhiEngine on degenerate particle sets; its reference is a recount of the
engine's own dense_D().

Gram variants part 7 reaches (dsvgd_gram_last_kernel, recorded per case):
HIST mode always runs sqdist_x3w_kernel (-1: no one-kernel Gram unit) -- the
32x32 form on the h2 engine, the 16x16 form on gemm="x3", and, for the row
block, the symmetric launch of its diagonal square with mirror stores;
BRACKET mode runs the same two kernels except on the h2 engine at d = 256,
where the symmetric layout takes the one-kernel Gram units: gram_sr_kernel
(2) as built, gram_w1_kernel (0) and gram_rs_kernel (1) under
dsvgd_gram_set_rs in test_bracket_gram_unit_variants.  So: x3w 32x32, x3w
16x16, w1, rs and sr are all reached.
"""
import numpy as np
import pytest
import torch

import select_reference as R
from conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {"h": 0.0, "inv_h": 0.0}
NOTES = {}


def note(err=0.0, **info):
    """record_parity with the running test's counters merged, not replaced."""
    import os
    mine = NOTES.setdefault(os.environ.get("PYTEST_CURRENT_TEST", "?"), {})
    mine.update(info)
    record_parity(err, **mine)


def native():
    from dsvgd import _native as N
    return N


def new_state():
    from dsvgd.engine import SelectState
    return SelectState(DEV)


def st_read(st):
    """The whole device state as a host copy of the C struct (synchronises)."""
    from dsvgd.engine import _SelectState
    return _SelectState.from_buffer_copy(st.buf.cpu().numpy().tobytes())


def st_put(st, hist=None, **fields):
    """Overwrite fields of the device state (read, modify, write back)."""
    s = st_read(st)
    for name, val in fields.items():
        setattr(s, name, val)
    st.buf.copy_(torch.from_numpy(np.frombuffer(bytes(s), dtype=np.int64).copy()))
    if hist is not None:
        st.hist.copy_(torch.from_numpy(np.asarray(hist, dtype=np.int64)))


def f32bits(x):
    return R.bits(x)


def dev_f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def dev_words(a):
    """uint32 words as a device float buffer (same bits)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(DEV).view(torch.float32)


def hist_of(st):
    return st.hist.cpu().numpy()


def diff_bins(got, want):
    bad = np.nonzero(got != want)[0]
    return {int(b): (int(got[b]), int(want[b])) for b in bad[:12]}


def check_bandwidth(s, n_total):
    """median -> h, inv_h of a finished select (the two ulp bounds)."""
    med = float(s.median)
    if med == 0.0 or n_total == 1:
        assert s.h == 1.0 and s.inv_h == 1.0
        return
    if not 1e-30 <= med <= 1e30:
        return
    eh = R.ulps(s.h, R.h_of(med, n_total))
    ei = R.ulps(s.inv_h, 1.0 / float(s.h))
    WORST["h"], WORST["inv_h"] = max(WORST["h"], eh), max(WORST["inv_h"], ei)
    print("median %.9g n_total %d: h %.9g (%.3f ulp), inv_h %.9g (%.3f ulp)"
          % (med, n_total, s.h, eh, s.inv_h, ei))
    note(max(eh, ei / 3.0), worst_h_ulps=WORST["h"], worst_inv_h_ulps=WORST["inv_h"])
    assert eh <= 1.0, (med, n_total, s.h, eh)
    assert ei <= 3.0, (s.h, s.inv_h, ei)


def run_passes(st, launch_hist, ks, w, k, prefix=0, first=1):
    """Passes first..3 of a select armed in st: after each histogram launch the
    bins equal the recount; after each pick the bins are zero and passes_done,
    k and prefix are the recount's; a second histogram launch of the pass just
    fixed leaves the bins zero.  Returns the final state."""
    N = native()
    strm = N.stream(DEV)
    kk = k
    for p in range(first, 4):
        launch_hist(p)
        got = hist_of(st)
        want = R.digit_hist(ks, p, prefix, w)
        assert np.array_equal(got, want), (p, diff_bins(got, want))
        N.call("dsvgd_radix_pick", st.ptr, p, strm)
        dig, kk = R.pick(want, kk)
        prefix |= dig << R.SHIFT[p]
        launch_hist(p)                      # the pass is fixed: nothing is added
        s = st_read(st)
        assert not np.any(np.ctypeslib.as_array(s.hist)), p
        assert (s.passes_done, s.k, s.prefix) == (p, kk, prefix), p
    assert f32bits(s.median) == prefix
    return s


# ---- 1. radix passes over a flat D ------------------------------------------------
@pytest.mark.parametrize("count", R.FLAT_COUNTS)
@pytest.mark.parametrize("family", sorted(R.FLAT_FAMILIES))
def test_radix_passes_over_flat_d(family, count):
    """float4 body, scalar tail and the grid stride (the last count is 7 past
    4 x 256 threads x 4096 blocks); +inf and NaN entries are never counted."""
    N = native()
    strm = N.stream(DEV)
    v, fin = R.flat_case(family, count)
    D = dev_f32(v)
    assert torch.equal(D.view(torch.int32).cpu(), torch.from_numpy(v.view(np.int32)))
    ks, finite = R.keys(v), v[fin]
    c = int(fin.sum())
    n_total = max(2, count)
    st = new_state()

    def launch(p):
        N.call("dsvgd_radix_hist", N.ptr(D), count, None, p, st.ptr, 0, strm)

    for k in R.flat_ranks(c):
        N.call("dsvgd_select_init", st.ptr, n_total, k, strm)
        s0 = st_read(st)
        assert (s0.k, s0.n_total, s0.prefix, s0.passes_done, s0.fallback) == (k, n_total, 0, 0, 1)
        assert np.isnan(s0.median) and np.isnan(s0.h) and np.isnan(s0.inv_h)
        s = run_passes(st, launch, ks, None, k)
        want = np.partition(finite, k)[k]
        assert f32bits(s.median) == f32bits(want), (k, s.median, want)
        check_bandwidth(s, n_total)


# ---- 2. radix_pick on a hand-written histogram --------------------------------------
@pytest.mark.parametrize("pas,b,k", R.pick_cases())
def test_radix_pick_on_a_written_histogram(pas, b, k):
    """u64 bin counts (3 * 2^32 + 5) either side of a thread and of a wave
    boundary of the block scan and in the last bin; k at the first and the
    last rank of the chosen bin."""
    N = native()
    strm = N.stream(DEV)
    st = new_state()
    n_total = 1000
    N.call("dsvgd_select_init", st.ptr, n_total, k, strm)
    h = R.pick_hist(pas)
    st_put(st, hist=h, prefix=R.PICK_PREFIX[pas], passes_done=pas - 1)
    N.call("dsvgd_radix_pick", st.ptr, pas, strm)
    s = st_read(st)
    dig, rem = R.pick(h, k)
    assert dig == b
    want_prefix = R.PICK_PREFIX[pas] | (b << R.SHIFT[pas])
    assert (s.prefix, s.k, s.passes_done) == (want_prefix, rem, pas)
    assert not np.any(np.ctypeslib.as_array(s.hist))
    if pas == 3:
        assert f32bits(s.median) == want_prefix
        check_bandwidth(s, n_total)
    else:
        assert np.isnan(s.median) and np.isnan(s.h)


@pytest.mark.parametrize("n_total", [1, 2, 3, 1000, 65536, 1 << 40])
def test_radix_pick_bandwidth_rules(n_total):
    """h = median / log(n_total) in fp64, rounded once; median == 0 or
    n_total == 1 give h = 1.  Medians: zero, and one key per 16th octave
    between 1e-30 and 1e30."""
    N = native()
    strm = N.stream(DEV)
    st = new_state()
    rs = np.random.RandomState(5)
    e = np.arange(28, 226, 16)
    med_keys = [0] + [int(x) << 23 | int(rs.randint(1 << 23)) for x in e]
    for key in med_keys:
        N.call("dsvgd_select_init", st.ptr, n_total, 2, strm)
        h = np.zeros(R.NBINS, dtype=np.int64)
        h[key & 0x3FF] = 5
        st_put(st, hist=h, prefix=key & ~0x3FF, passes_done=2)
        N.call("dsvgd_radix_pick", st.ptr, 3, strm)
        s = st_read(st)
        assert f32bits(s.median) == key and s.k == 2 and s.passes_done == 3
        if key == 0 or n_total == 1:
            assert s.h == 1.0 and s.inv_h == 1.0
        else:
            assert 1e-30 <= s.median <= 1e30
        check_bandwidth(s, n_total)


# ---- 3. symmetric and weighted layouts ------------------------------------------------
def tile_values(Tm, Tn):
    """Distinct finite values per tile that differ in digit 3, digit 2 and --
    every eighth -- digit 1."""
    idx = np.arange(Tm * Tn, dtype=np.uint32).reshape(Tm, Tn)
    return (np.uint32(R.bits(1.7)) + np.uint32(0x40801) * idx).view(np.float32)


def weighted_ranks(total):
    return sorted({0, (total - 1) // 2, total // 2, total - 1})


@pytest.mark.parametrize("npad", [256, 384])
def test_radix_passes_symmetric_layout(npad):
    """Lower-triangle tiles hold a finite poison of weight 0; the diagonal
    counts once, the upper triangle twice."""
    N = native()
    strm = N.stream(DEV)
    T = npad // 128
    tv = tile_values(T, T)
    tw = R.sym_tile_weights(T)
    tv[tw == 0] = R.from_bits(R.bits(1.7) + 0x40801 * 2 + 3)      # poison among the values
    buf, w = R.panel_fill(npad, npad, tv), R.panel_weights(npad, npad, tw)
    D = dev_f32(buf)
    ks = R.keys(buf)
    total = int(w.sum())
    assert total == 128 * 128 * T * T
    st = new_state()

    def launch(p):
        N.call("dsvgd_radix_hist", N.ptr(D), npad * npad, None, p, st.ptr, npad, strm)

    for k in weighted_ranks(total):
        N.call("dsvgd_select_init", st.ptr, npad, k, strm)
        s = run_passes(st, launch, ks, w, k)
        assert f32bits(s.median) == f32bits(R.weighted_kth(buf, w, k)), k
        check_bandwidth(s, npad)


@pytest.mark.parametrize("mpad,tw", [(128, [[2, 0, 1]]), (256, [[1, 2, 0], [0, 2, 1]])])
def test_radix_passes_weight_map(mpad, tw):
    """dsvgd_radix_hist_wmap: a rectangle of tiles with weights from {0, 1, 2}."""
    N = native()
    strm = N.stream(DEV)
    npad = 384
    tw = np.asarray(tw, dtype=np.int64)
    tv = tile_values(mpad // 128, npad // 128)
    buf, w = R.panel_fill(mpad, npad, tv), R.panel_weights(mpad, npad, tw)
    D = dev_f32(buf)
    wmap = torch.from_numpy(tw.astype(np.uint8)).to(DEV).contiguous()
    ks = R.keys(buf)
    total = int(w.sum())
    st = new_state()

    def launch(p):
        N.call("dsvgd_radix_hist_wmap", N.ptr(D), mpad, npad, None, p, st.ptr, N.ptr(wmap), strm)

    for k in weighted_ranks(total):
        N.call("dsvgd_select_init", st.ptr, npad, k, strm)
        s = run_passes(st, launch, ks, w, k)
        assert f32bits(s.median) == f32bits(R.weighted_kth(buf, w, k)), k


# ---- 4. bracket bookkeeping ---------------------------------------------------------------
def arm_bracket(st, lo, hi, n_total, cand_cap):
    """dsvgd_bracket_init from two states whose median the test wrote."""
    N = native()
    lo_st, hi_st = new_state(), new_state()
    st_put(lo_st, median=float(np.float32(lo)))
    st_put(hi_st, median=float(np.float32(hi)))
    st_put(st, hist=np.arange(R.NBINS), k=77, prefix=123, passes_done=3, fallback=1, below_total=5,
           ncand_total=6, overflow=7, nslots=8, slot_cap=9)          # stale values to be reset
    N.call("dsvgd_bracket_init", st.ptr, n_total, lo_st.ptr, hi_st.ptr, cand_cap, N.stream(DEV))
    s = st_read(st)
    assert not np.any(np.ctypeslib.as_array(s.hist))
    assert (s.k, s.n_total, s.prefix, s.passes_done, s.fallback) == \
        ((n_total * n_total - 1) // 2, n_total, 0, 0, 0)
    assert (s.below_total, s.ncand_total, s.overflow, s.cand_cap, s.nslots, s.slot_cap) == \
        (0, 0, 0, cand_cap, 0, 0)
    assert np.isnan(s.median) and np.isnan(s.h) and np.isnan(s.inv_h)
    if np.isnan(lo):
        assert np.isnan(s.lo)
    else:
        assert f32bits(s.lo) == f32bits(lo)
    assert f32bits(s.hi) == f32bits(hi)
    return s


@pytest.mark.parametrize("ns", R.TOTALS_NSLOTS)
def test_bracket_totals(ns):
    """256 x 256 threads sum the slots (65537: one past a whole grid), weight-2
    slots twice; a second call adds again -- the caller zeroes (bracket_init)
    before each use, which is what a distributed caller relies on."""
    N = native()
    strm = N.stream(DEV)
    slots, cap = R.totals_slots(ns)
    buf, tot = R.build_cand(slots, cap)
    cand = dev_words(buf)
    st = new_state()
    lo, hi = R.BRACKETS["shared"]
    arm_bracket(st, lo, hi, 4096, buf.size)
    st_put(st, nslots=ns, slot_cap=cap)
    N.call("dsvgd_bracket_totals", st.ptr, N.ptr(cand), strm)
    s = st_read(st)
    assert (s.below_total, s.ncand_total, s.overflow) == tot
    N.call("dsvgd_bracket_totals", st.ptr, N.ptr(cand), strm)
    s = st_read(st)
    assert (s.below_total, s.ncand_total, s.overflow) == tuple(2 * t for t in tot)


@pytest.mark.parametrize("bracket", sorted(R.BRACKETS))
@pytest.mark.parametrize("name", sorted(R.decision_cases()))
def test_bracket_check_decision_edges(name, bracket):
    N = native()
    strm = N.stream(DEV)
    kind, slots, cap, k, tot = R.decision_case(name)
    buf, _ = R.build_cand(slots, cap)
    cand = dev_words(buf)
    st = new_state()
    lo, hi = R.BRACKETS[bracket]
    arm_bracket(st, lo, hi, 4096, buf.size)
    st_put(st, nslots=len(slots), slot_cap=cap, k=k)
    N.call("dsvgd_bracket_totals", st.ptr, N.ptr(cand), strm)
    N.call("dsvgd_bracket_check", st.ptr, strm)
    s = st_read(st)
    assert (s.below_total, s.ncand_total, s.overflow) == tot
    if kind == "holds":
        assert (s.fallback, s.k) == (0, k - tot[0])
        if f32bits(lo) >> 21 == f32bits(hi) >> 21:      # digit 1 fixed by the bracket
            assert (s.passes_done, s.prefix) == (1, f32bits(lo) & 0xFFE00000)
        else:
            assert (s.passes_done, s.prefix) == (0, 0)
    else:
        assert (s.fallback, s.k, s.passes_done, s.prefix) == (1, k, 0, 0)


def test_bracket_check_nan_bracket_falls_back():
    """A NaN lo: the slot writers count everything below and nothing in range
    (SlotWriter::begin), so the check must end in the passes over D."""
    N = native()
    strm = N.stream(DEV)
    n = 300
    empty = np.zeros(0, np.float32)
    slots = [(empty, False, 0, 128 * 128)] * 3 + [(empty, True, 0, (n * n - 3 * 128 * 128) // 2)]
    buf, tot = R.build_cand(slots, 4)
    assert tot == (n * n, 0, 0)
    st = new_state()
    arm_bracket(st, np.float32(np.nan), np.float32(2.0), n, buf.size)
    st_put(st, nslots=len(slots), slot_cap=4)
    N.call("dsvgd_bracket_totals", st.ptr, N.ptr(dev_words(buf)), strm)
    N.call("dsvgd_bracket_check", st.ptr, strm)
    s = st_read(st)
    assert (s.below_total, s.ncand_total, s.overflow) == tot
    assert (s.fallback, s.k, s.passes_done, s.prefix) == (1, (n * n - 1) // 2, 0, 0)


# ---- 5. radix passes over the candidate slots ------------------------------------------
def arm_candidates(st, bracket, k, ns, cap, n_total, fallback=0):
    """The state bracket_check leaves for a bracket that holds rank k."""
    N = native()
    lo, hi = R.BRACKETS[bracket]
    N.call("dsvgd_select_init", st.ptr, n_total, k, N.stream(DEV))
    shared = f32bits(lo) >> 21 == f32bits(hi) >> 21 and not fallback
    prefix = f32bits(lo) & 0xFFE00000 if shared else 0
    st_put(st, fallback=fallback, nslots=ns, slot_cap=cap, lo=float(lo), hi=float(hi),
           prefix=prefix, passes_done=1 if shared else 0)
    return prefix, (2 if shared else 1)


@pytest.mark.parametrize("bracket", ["shared", "straddle"])
@pytest.mark.parametrize("cap", R.WALK_CAPS)
@pytest.mark.parametrize("ns", R.WALK_NSLOTS)
def test_radix_passes_over_candidate_slots(ns, cap, bracket):
    """4096 waves walk the slots two at a time with a stride of 8192: an odd
    count, a second slot past the end, a second trip.  D and the slot entries
    past min(count, cap) hold a poison inside the bracket: a read of either
    shows in the histogram."""
    N = native()
    strm = N.stream(DEV)
    lo, hi = R.BRACKETS[bracket]
    poison = R.from_bits(R.bits(lo) + 1)
    slots = R.walk_slots(ns, cap, bracket)
    buf, _ = R.build_cand(slots, cap, poison=poison)
    cand = dev_words(buf)
    D = torch.full((1024,), float(poison), dtype=torch.float32, device=DEV)
    v, w = R.cand_multiset(slots, cap)
    ks = R.keys(v)
    total = int(w.sum())
    st = new_state()

    def launch(p):
        N.call("dsvgd_radix_hist", N.ptr(D), D.numel(), N.ptr(cand), p, st.ptr, 0, strm)

    for k in sorted({0, total // 2, total - 1}):
        prefix, first = arm_candidates(st, bracket, k, ns, cap, 4096)
        if first == 2:      # digit 1 fixed by the bracket: both pass-1 launches return at once
            launch(1)
            N.call("dsvgd_radix_pick", st.ptr, 1, strm)
            s = st_read(st)
            assert not np.any(np.ctypeslib.as_array(s.hist))
            assert (s.passes_done, s.k, s.prefix) == (1, k, prefix)
        s = run_passes(st, launch, ks, w, k, prefix, first)
        assert f32bits(s.median) == f32bits(R.weighted_kth(v, w, k)), k
        assert lo <= s.median <= hi


@pytest.mark.parametrize("bracket", ["shared", "straddle"])
def test_radix_passes_fallback_reads_d_not_the_slots(bracket):
    """fallback == 1 with a candidate buffer given: the passes read D; the
    slots (valid counts, poisoned data) must not be touched."""
    N = native()
    strm = N.stream(DEV)
    ns, cap = 5, 300
    lo, hi = R.BRACKETS[bracket]
    slots = R.walk_slots(ns, cap, bracket)
    v, _ = R.cand_multiset(slots, cap)
    poisoned = [(np.full(len(s[0]), lo, np.float32), s[1], s[2]) for s in slots]
    buf, _ = R.build_cand(poisoned, cap, poison=lo)
    cand = dev_words(buf)
    D = dev_f32(v)
    ks = R.keys(v)
    st = new_state()

    def launch(p):
        N.call("dsvgd_radix_hist", N.ptr(D), D.numel(), N.ptr(cand), p, st.ptr, 0, strm)

    for k in (0, v.size // 2, v.size - 1):
        prefix, first = arm_candidates(st, bracket, k, ns, cap, 4096, fallback=1)
        assert (prefix, first) == (0, 1)
        s = run_passes(st, launch, ks, None, k)
        assert f32bits(s.median) == f32bits(np.partition(v, k)[k])


# ---- 6. sample selects on hand-built samples ------------------------------------------------
@pytest.mark.parametrize("s", R.SAMPLE_SIZES)
@pytest.mark.parametrize("kind", R.SAMPLE_KINDS)
def test_sample_bracket_select_on_built_samples(kind, s):
    N = native()
    strm = N.stream(DEV)
    v, ranks = R.sample_case(kind, s)
    srt = np.sort(v)
    sample = dev_f32(v)
    lo_st, hi_st, st = new_state(), new_state(), new_state()
    n_total, cand_cap = 12345, (1 << 20) + 3
    for klo, khi in ranks:
        for rep in range(2):                        # a second call gives the same
            st_put(st, hist=np.arange(R.NBINS), k=1, fallback=1, below_total=5, ncand_total=6,
                   overflow=7, nslots=8, slot_cap=9, passes_done=3, prefix=99)
            N.call("dsvgd_sample_bracket_select", N.ptr(sample), s, klo, khi, lo_st.ptr,
                   hi_st.ptr, st.ptr, n_total, cand_cap, strm)
            a, b, c = st_read(lo_st), st_read(hi_st), st_read(st)
            assert f32bits(a.median) == f32bits(srt[klo]), (klo, rep, a.median, srt[klo])
            assert f32bits(b.median) == f32bits(srt[khi]), (khi, rep, b.median, srt[khi])
            for x in (a, b, c):
                assert not np.any(np.ctypeslib.as_array(x.hist))
            assert (a.passes_done, a.k, a.n_total) == (3, klo - int((srt < srt[klo]).sum()), s)
            assert (b.passes_done, b.k, b.n_total) == (3, khi - int((srt < srt[khi]).sum()), s)
            assert (f32bits(c.lo), f32bits(c.hi)) == (f32bits(srt[klo]), f32bits(srt[khi]))
            assert (c.k, c.n_total, c.fallback, c.prefix, c.passes_done) == \
                ((n_total * n_total - 1) // 2, n_total, 0, 0, 0)
            assert (c.below_total, c.ncand_total, c.overflow, c.cand_cap, c.nslots, c.slot_cap) == \
                (0, 0, 0, cand_cap, 0, 0)
            check_bandwidth(a, s)
            check_bandwidth(b, s)


# ---- 7. the fused accounting of the Gram kernels on degenerate particle sets ------------
def engine_cls(bracket):
    import dsvgd
    if not bracket:
        return dsvgd.PhiEngine

    class BracketEngine(dsvgd.PhiEngine):
        BRACKET_MIN_ENTRIES = 1
        SAMPLE = 4096
    return BracketEngine


def check_hist_mode(eng, X, k, entries):
    """Fused digit-1 histogram == recount of dense D == a standalone pass 1;
    the median bit-equal to np.partition."""
    N = native()
    strm = N.stream(DEV)
    eng.pack(dev_f32(X))
    eng.distances(median=True)
    kernel = int(N.load().dsvgd_gram_last_kernel())
    fused = hist_of(eng.state)
    D = eng.dense_D().cpu().numpy()
    assert D.size == entries
    want = R.digit_hist(R.keys(D), 1)
    assert int(want.sum()) == entries
    st2 = new_state()
    N.call("dsvgd_select_init", st2.ptr, eng.n, eng.k_rank, strm)
    N.call("dsvgd_radix_hist", N.ptr(eng.D), eng.m_pad * eng.n_pad, None, 1, st2.ptr,
           eng.n_pad if eng.sym else 0, strm)
    alone = hist_of(st2)
    assert np.array_equal(alone, want), ("standalone pass 1", diff_bins(alone, want))
    print("kernel %d, fused bins (got, recount) that differ: %s"
          % (kernel, diff_bins(fused, want)))
    note(gram_kernel=kernel, fused_sum=int(fused.sum()))
    assert int(fused.sum()) == entries, ("fused histogram sum", int(fused.sum()), entries,
                                         diff_bins(fused, want))
    assert np.array_equal(fused, want), diff_bins(fused, want)
    eng.median_bandwidth()
    s = st_read(eng.state)
    exact = np.partition(D.ravel(), k)[k]
    assert f32bits(s.median) == f32bits(exact), (s.median, exact)
    check_bandwidth(s, eng.n)


@pytest.mark.parametrize("gemm", ["h2", "x3"])
@pytest.mark.parametrize("kind,n,d", R.gram_cases())
def test_fused_histogram_on_degenerate_sets(kind, n, d, gemm):
    """HIST mode (every engine below BRACKET_MIN_ENTRIES).  At n >= 256 the
    128-tile (0, 1) of the symmetric square is interior and mirrored: a lane
    adds 128 values of weight 2, on these sets all to one digit-1 bin."""
    eng = engine_cls(False)(n, d, device=DEV, gemm=gemm)
    assert not eng.bracketed
    check_hist_mode(eng, R.particle_set(kind, n, d), (n * n - 1) // 2, n * n)


@pytest.mark.parametrize("gemm", ["h2", "x3"])
@pytest.mark.parametrize("kind,d", [("identical", 3), ("lattice", 65), ("clusters", 256),
                                    ("equidistant", 768)])
def test_fused_histogram_row_block_diagonal_square(kind, d, gemm):
    """A 256-aligned row block (local median): its diagonal square runs the
    symmetric kernel with mirror stores, tile (0, 1) of it at weight 2."""
    n, m, row0 = 768, 256, 256
    eng = engine_cls(False)(n, d, m=m, row0=row0, device=DEV, local_median=True, gemm=gemm)
    assert not eng.bracketed and eng.k_rank == (m * n - 1) // 2
    check_hist_mode(eng, R.particle_set(kind, n, d), (m * n - 1) // 2, m * n)


def run_bracketed(eng, X):
    N = native()
    eng.pack(dev_f32(X))
    eng.distances(median=True)
    kernel = int(N.load().dsvgd_gram_last_kernel())
    eng.median_bandwidth()
    s = st_read(eng.state)
    D = eng.dense_D().cpu().numpy()
    n = eng.n
    k = (n * n - 1) // 2
    exact = np.partition(D.ravel(), k)[k]
    lo, hi = np.float32(s.lo), np.float32(s.hi)
    below, ncand = int((D < lo).sum()), int(((D >= lo) & (D <= hi)).sum())
    print("kernel %d lo %.9g hi %.9g below %d (%d) ncand %d (%d) overflow %d fallback %d nslots %d "
          "slot_cap %d" % (kernel, lo, hi, s.below_total, below, s.ncand_total, ncand, s.overflow,
                           s.fallback, s.nslots, s.slot_cap))
    assert s.fallback in (0, 1)
    # the totals are the recount whether or not the bracket is then used,
    # unless a slot overflowed (its count saturates nothing: counts stay exact)
    assert (s.below_total, s.ncand_total) == (below, ncand)
    if s.fallback == 0:
        assert s.overflow == 0 and below <= k < below + ncand
    else:
        assert s.overflow > 0 or not below <= k < below + ncand
    assert f32bits(s.median) == f32bits(exact), (s.median, exact, s.fallback)
    check_bandwidth(s, n)
    return s, kernel


@pytest.mark.parametrize("gemm", ["h2", "x3"])
@pytest.mark.parametrize("kind,n,d", R.gram_cases())
def test_bracketed_select_on_degenerate_sets(kind, n, d, gemm):
    """BRACKET mode at the same shapes: as built, then with the candidate
    buffer shrunk to 16 floats per slot, which overflows on these sets."""
    eng = engine_cls(True)(n, d, device=DEV, gemm=gemm)
    assert eng.bracketed
    X = R.particle_set(kind, n, d)
    s, kernel = run_bracketed(eng, X)
    eng.cand_cap = 18 * int(s.nslots)
    s2, _ = run_bracketed(eng, X)
    assert s2.slot_cap == 16 and s2.nslots == s.nslots
    note(gram_kernel=kernel, fallback=(int(s.fallback), int(s2.fallback)))


@pytest.mark.parametrize("rs,want", [(0, 0), (1, 1)])
@pytest.mark.parametrize("kind,n", [("identical", 256), ("lattice", 384), ("clusters", 384)])
def test_bracket_gram_unit_variants(kind, n, rs, want):
    """The one-kernel Gram units of the h2 engine at d = 256 under
    dsvgd_gram_set_rs: gram_w1_kernel (0) and gram_rs_kernel (1)."""
    lib = native().load()
    prev = lib.dsvgd_gram_set_rs(rs)
    try:
        eng = engine_cls(True)(n, 256, device=DEV, gemm="h2")
        s, kernel = run_bracketed(eng, R.particle_set(kind, n, 256))
        note(gram_kernel=kernel)
        assert kernel == want
    finally:
        lib.dsvgd_gram_set_rs(prev)
