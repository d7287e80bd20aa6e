"""The W2 auction of csrc/w2.hip called directly through the C ABI
(dsvgd_w2_assign / _warm / _stat, dsvgd_w2_grad) at its smallest shapes and at
every edge of w2_assign's dispatch, on hand-built cost matrices uploaded as
they are (tests/w2_reference.py; tests/test_w2_host.py shows that the fp64
side and these inputs can tell a wrong answer from a right one).

Every solve is held to include/dsvgd.h's promise, "within one fp32 ulp of
max C of the optimum", and to nothing looser:

1. the plan is an int32 permutation of 0 .. n - 1;
2. C64[rows, plan].sum() - opt <= n eps_final (= cmax 2^-24 here), opt from
   scipy's exact assignment, once per case;
3. the row sets are scipy's (every case compared is decisive: the cheapest
   exchange of two slots' columns costs >= 16 x the bound);
4. R = 1: the dual certificate on the solve's own fp64 prices (workspace
   byte 256): every row's column is within eps_final + slack of its best
   value -C64 - p, slack = min(2^-40 (cmax + max p), eps_final / 16).  The
   cases marked certificate-only need no scipy run;
5. dsvgd_w2_grad entry by entry within (R + 3) 2^-24 A.

The edges: n = 64 / 65 (w2_tail_kernel alone / the bid kernels), the K = 2, 3,
5, 9, 17, 33 templates and the price cache (R = 2 .. 8) at the R where each
begins, block_topk's batched path at 1793 / 2049 columns (256 threads) and
3585 / 4097 (the tail's 512), the tail's c & 4095 and i & 511 tables at
n = 4097 and m = 513, the three warm entry passes (w2_scan_first_kernel,
w2_violation_rows_kernel, w2_violation_kernel) with ldc > n, an unaligned C
and n % 4 != 0, the keep rule, theta at its limits, a forced tail stall, cost
families that tie, and every return code.

The parity dump gets, per test, the worst of (cost - opt) / (n eps_final),
the certificate's worst / (eps_final + slack) and the gradient ratio -- each
must be <= 1 -- and the auction's round counters.
"""
import ctypes

import numpy as np
import pytest
import torch

import w2_reference as W
from conftest import record_parity

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
IDS = W.case_id


def native():
    from dsvgd import _native as N
    return N


def stream():
    return native().stream(torch.device(DEV))


class Solved(object):
    def __init__(self, plan, rounds, price, stats, trace):
        self.plan, self.rounds, self.price, self.stats, self.trace = plan, rounds, price, stats, trace

    @property
    def stalled(self):
        return self.stats[5] != 0


class Problem(object):
    """One m x n cost matrix on the device in a given layout, its workspace
    and plan.  Layouts: "plain" (ldc = n, 16-byte aligned), "ldc5" (ldc = n + 5,
    the pad columns NaN: a pad read trips done = 3 or spoils the plan), "off1"
    (C starts one float past a 16-byte boundary)."""

    def __init__(self, C, layout="plain"):
        self.m, self.n = C.shape
        self.R = self.n // self.m
        self.ldc = self.n + 5 if layout == "ldc5" else self.n
        self.off = 1 if layout == "off1" else 0
        self.buf = torch.full((self.off + self.m * self.ldc + 3,), NAN, dtype=torch.float32,
                              device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.Cd = self.buf[self.off:self.off + self.m * self.ldc].view(self.m, self.ldc)
        self.set_cost(C)
        nb = int(native().load().dsvgd_w2_workspace_bytes(self.m, self.n))
        self.ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
        self.assign = torch.full((self.n,), -7, dtype=torch.int32, device=DEV)

    def set_cost(self, C):
        assert C.shape == (self.m, self.n) and C.dtype == np.float32
        self.C = C
        self.Cd[:, :self.n] = torch.from_numpy(np.array(C)).to(DEV)

    def pads_untouched(self):
        """Nothing but the live entries of C ever changes (and they do not either)."""
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        live = host[self.off:self.off + self.m * self.ldc].reshape(self.m, self.ldc)
        return bool(np.isnan(host[:self.off]).all() and np.isnan(host[-3:]).all()
                    and np.isnan(live[:, self.n:]).all()
                    and np.array_equal(live[:, :self.n].view(np.uint32),
                                       np.asarray(self.C).view(np.uint32)))

    def solve(self, entry="assign", warm_phases=0, prev=None, cstat=False,
              max_rounds=W.MAX_ROUNDS, m=None, n=None, ldc=None):
        N = native()
        m, n, ldc = m or self.m, n or self.n, ldc or self.ldc
        rounds = ctypes.c_int64(-1)
        rp = ctypes.addressof(rounds)
        prev_d = None if prev is None else torch.as_tensor(np.asarray(prev, np.int32), device=DEV)
        stat_d = None
        if cstat:   # filled here, not by dsvgd_w2_cost_h2: the bits of C.max() and "all finite"
            bits = np.array([np.float32(self.C.max()).view(np.int32), 0], np.int32)
            stat_d = torch.as_tensor(bits, device=DEV)
        Cp, wp, ap = N.ptr(self.Cd), N.ptr(self.ws), N.ptr(self.assign)
        if entry == "assign":
            N.call("dsvgd_w2_assign", Cp, ldc, m, n, wp, max_rounds, warm_phases, ap, rp, stream())
        elif entry == "warm":
            N.call("dsvgd_w2_assign_warm", Cp, ldc, m, n, wp, max_rounds, N.ptr(prev_d), ap, rp,
                   stream())
        elif entry == "stat":
            N.call("dsvgd_w2_assign_stat", Cp, ldc, m, n, wp, max_rounds, warm_phases,
                   N.ptr(prev_d), ap, rp, N.ptr(stat_d), stream())
        else:
            raise KeyError(entry)
        torch.cuda.synchronize()
        lib = N.load()
        st = (ctypes.c_int64 * 6)()
        lib.dsvgd_w2_tail_stats(st)
        k = int(lib.dsvgd_w2_trace(None, 0))
        tr = (ctypes.c_int64 * (3 * max(k, 1)))()
        lib.dsvgd_w2_trace(tr, k)
        price = self.ws[256:256 + 8 * self.n].cpu().numpy().view(np.float64).copy()
        plan = self.assign.cpu().numpy()
        return Solved(plan, int(rounds.value), price, tuple(int(v) for v in st),
                      np.array(tr[:3 * k], np.int64).reshape(k, 3))


def check(res, case, C, scipy=True, what=""):
    """Checks 1 - 4 of one solve of `case`; returns the worst ratio to its bound."""
    m, n = C.shape
    R = n // m
    plan = res.plan
    assert plan.dtype == np.int32 and plan.min() >= 0 and plan.max() < n, what
    assert W.is_permutation(plan, n), what                                           # 1
    assert res.rounds >= 0, what
    worst = 0.0
    if scipy:
        ref, opt = W.optimum(*case)
        worst = W.cost_gap_ratio(C, plan, opt)                                       # 2
        assert worst <= 1.0, (what, worst, W.plan_cost(C, plan), opt)
        if case in W.ROWSET_CASES:                                                   # 3
            np.testing.assert_array_equal(W.row_sets(plan, m), W.row_sets(ref, m), err_msg=what)
    if R == 1:                                                                       # 4
        cert = W.certificate_ratio(C, plan, res.price)
        assert cert <= 1.0, (what, cert)
        worst = max(worst, cert)
    return max(worst, 0.0)


def switch(name, value):
    """Set a process-wide switch; returns the value to restore in a finally."""
    return getattr(native().load(), name)(value)


# ------------------------------------------------------------ cold solves --
@pytest.mark.parametrize("case", W.COLD, ids=IDS)
def test_cold(case):
    C = W.cost(*case)
    p = Problem(C)
    res = p.solve()
    worst = check(res, case, C)
    if (case[1], case[2]) in W.TAIL_ONLY:
        # the whole solve is the one-workgroup tail's: no readback saw more than 64 free
        assert res.stats[0] > 0, res.stats
        assert len(res.trace) >= 1 and res.trace[:, 2].max() <= 64, res.trace
    assert p.pads_untouched()
    record_parity(worst, rounds=res.rounds, tail_bids=res.stats[0], stalls=res.stats[5])


@pytest.mark.parametrize("case", W.CERT_ONLY, ids=IDS)
def test_cold_certificate_only(case):
    """The tail's 512-thread scan edge (3585), the first shared entry of its
    column table (4097) and every entry shared (8192): by weak duality the
    certificate alone implies the cost bound."""
    C = W.cost(*case)
    res = Problem(C).solve()
    worst = check(res, case, C, scipy=False)
    record_parity(worst, rounds=res.rounds, tail_bids=res.stats[0], stalls=res.stats[5])


@pytest.mark.parametrize("shape", W.TIE_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("family", W.TIE_FAMILIES)
def test_cold_ties(family, shape):
    """Integer costs (the bound is below 1: exactly optimal), identical rows,
    a constant matrix, all zeros (done == 2: the identity plan)."""
    case = (family,) + shape
    C = W.cost(*case)
    res = Problem(C).solve()
    worst = check(res, case, C)
    if family in ("int01", "int03"):
        assert W.plan_cost(C, res.plan) == W.optimum(*case)[1]
    if family == "zeros":
        np.testing.assert_array_equal(res.plan, np.arange(C.shape[1]))
    record_parity(worst, rounds=res.rounds, stalls=res.stats[5])


@pytest.mark.parametrize("shape", W.TIE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_cold_power_of_two_scaling(shape):
    """Costs scaled by 2^40 and 2^-40: every step of the solve scales exactly,
    so unless a tail stalled the plan and the round count are the unscaled run's."""
    out, worst = {}, 0.0
    for family in ["uniform"] + W.SCALED_FAMILIES:
        case = (family,) + shape
        C = W.cost(*case)
        out[family] = Problem(C).solve()
        worst = max(worst, check(out[family], case, C, what=family))
    base = out["uniform"]
    for family in W.SCALED_FAMILIES:
        if not (base.stalled or out[family].stalled):
            np.testing.assert_array_equal(out[family].plan, base.plan, err_msg=family)
            assert out[family].rounds == base.rounds, (family, out[family].rounds, base.rounds)
    record_parity(worst, rounds=base.rounds, stalls=sum(r.stats[5] for r in out.values()))


# ----------------------------------------------------------------- layout --
@pytest.mark.parametrize("shape", W.LAYOUT_SHAPES + W.LAYOUT_ROWS4_SHAPES,
                         ids=lambda s: "%dx%d" % s)
def test_layouts_same_solve(shape):
    """ldc = n + 5 with NaN pads, C one float past a 16-byte boundary and the
    plain ldc = n copy: cold, then warm from the solve's own plan.  At
    n % 4 != 0 every copy's warm entry pass is w2_violation_kernel; at
    n % 4 == 0 the plain copy's is w2_scan_first_kernel (R = 1, fuse on) or
    w2_violation_rows_kernel (R = 1 fuse off, R = 4) and the other two copies'
    w2_violation_kernel -- "the same bits" for viol, so the same plan and round
    count wherever no tail stalled."""
    case = ("svgd",) + shape
    C = W.cost(*case)
    R = shape[1]
    out, worst = {}, 0.0
    for layout in ["plain", "ldc5", "off1"]:
        p = Problem(C, layout)
        runs = {"cold": p.solve()}
        own = runs["cold"].plan
        saved = p.ws.clone()
        runs["warm"] = p.solve("warm", prev=own)
        if R == 1:    # w2_violation_rows_kernel (plain, n % 4 == 0) / w2_violation_kernel
            old = switch("dsvgd_w2_set_fuse_first", 0)
            try:
                p.ws.copy_(saved)
                runs["warm_unfused"] = p.solve("warm", prev=own)
            finally:
                switch("dsvgd_w2_set_fuse_first", old)
        for name, res in runs.items():
            worst = max(worst, check(res, case, C, what="%s %s" % (layout, name)))
        assert p.pads_untouched(), layout
        out[layout] = runs
    for layout in ["ldc5", "off1"]:
        for name, res in out[layout].items():
            ref = out["plain"][name]
            if not (res.stalled or ref.stalled):
                np.testing.assert_array_equal(res.plan, ref.plan, err_msg="%s %s" % (layout, name))
                np.testing.assert_array_equal(res.price, ref.price,
                                              err_msg="%s %s" % (layout, name))
                assert res.rounds == ref.rounds, (layout, name, res.rounds, ref.rounds)
    if R == 1 and not (out["plain"]["warm"].stalled or out["plain"]["warm_unfused"].stalled):
        np.testing.assert_array_equal(out["plain"]["warm"].plan, out["plain"]["warm_unfused"].plan)
        assert out["plain"]["warm"].rounds == out["plain"]["warm_unfused"].rounds
    record_parity(worst, rounds_cold=out["plain"]["cold"].rounds,
                  rounds_warm=out["plain"]["warm"].rounds)


# ------------------------------------------------------------ warm solves --
# Two fixed phases above eps_final (warm_phases = 2) are meant for a nearby
# problem.  After the step of 0.3 the kept prices are far off, and 64 eps_final
# is a price war fought in the tail one scan per bid: measured 2747 rounds and
# ~200 s per solve at 2048 x 2048 (R = 1), 506 rounds and ~140 s at 65 x 2080
# (R = 32), 1060 rounds and ~15 s at 683 x 2049 (R = 3) -- correct plans, but no
# test for every later run of the suite.  That variant therefore runs at the
# step of 0.3 only up to this n (65 x 65: 6 rounds; 13 x 65); at 1e-4 everywhere.
FIXED_PHASES_FAR_MAX_N = 96


@pytest.mark.parametrize("case", W.WARM, ids=IDS)
def test_warm(case):
    """Problem 1 cold, then the moved problem on the same workspace (its prices
    put back before every variant) through every warm entry point."""
    family, m, R = case
    n = m * R
    C1, C2 = W.cost("first" + family[5:], m, R), W.cost(*case)
    p = Problem(C1)
    first = p.solve()
    check(first, None, C1, scipy=False, what="first")
    saved = p.ws.clone()
    p.set_cost(C2)
    rs = np.random.RandomState(n)
    holes = first.plan.copy()
    holes[rs.permutation(n)[:max(1, n // 8)]] = -1
    holes[rs.permutation(n)[:max(1, n // 8)]] = n
    variants = [("warm", dict(entry="warm", prev=first.plan)),
                ("stat_prev", dict(entry="stat", prev=first.plan, cstat=True)),
                ("stat_cold", dict(entry="stat", warm_phases=0, cstat=True)),
                ("reversed", dict(entry="warm", prev=np.arange(n)[::-1])),
                ("holes", dict(entry="warm", prev=holes))]
    if family != "moved0.3" or n <= FIXED_PHASES_FAR_MAX_N:
        variants += [("phases2", dict(entry="assign", warm_phases=2)),
                     ("stat_phases2", dict(entry="stat", warm_phases=2, cstat=True))]
    out, worst = {}, 0.0
    for name, kw in variants:
        p.ws.copy_(saved)
        out[name] = p.solve(**kw)
        worst = max(worst, check(out[name], case, C2, what=name))
    if R == 1:
        old = switch("dsvgd_w2_set_fuse_first", 0)
        try:
            for name in ("warm", "reversed", "holes"):
                p.ws.copy_(saved)
                res = p.solve(**dict(variants)[name])
                worst = max(worst, check(res, case, C2, what=name + " unfused"))
                if not (res.stalled or out[name].stalled):   # "same bids, same plan"
                    np.testing.assert_array_equal(res.plan, out[name].plan, err_msg=name)
                    assert res.rounds == out[name].rounds, (name, res.rounds, out[name].rounds)
        finally:
            switch("dsvgd_w2_set_fuse_first", old)
    # cstat in place of the pass over C: "the same plan"
    for a, b in (("stat_prev", "warm"), ("stat_phases2", "phases2")):
        if a not in out:
            continue
        if not (out[a].stalled or out[b].stalled):
            np.testing.assert_array_equal(out[a].plan, out[b].plan, err_msg=a)
            assert out[a].rounds == out[b].rounds, (a, out[a].rounds, out[b].rounds)
    assert p.pads_untouched()
    record_parity(worst, rounds_first=first.rounds,
                  **{"rounds_" + k: v.rounds for k, v in out.items()})


# --------------------------------------------------------- keep and theta --
@pytest.mark.parametrize("case", [(f, m, R) for (m, R) in W.KEEP_SHAPES
                                  for f in ("uniform", "svgd")], ids=IDS)
def test_keep_rule(case):
    """dsvgd_w2_set_keep(1): phases keep their eps-CS slots, and the warm start
    loads the previous plan as epoch 0's (w2_load_prev_kernel)."""
    C = W.cost(*case)
    p = Problem(C)
    old = switch("dsvgd_w2_set_keep", 1)
    try:
        cold = p.solve()
        warm = p.solve("warm", prev=cold.plan)
    finally:
        switch("dsvgd_w2_set_keep", old)
    worst = max(check(cold, case, C, what="cold"), check(warm, case, C, what="warm"))
    record_parity(worst, rounds_cold=cold.rounds, rounds_warm=warm.rounds)


@pytest.mark.parametrize("theta", [2.0, 1024.0])
@pytest.mark.parametrize("case", [(f, m, R) for (m, R) in W.THETA_SHAPES
                                  for f in ("uniform", "svgd")], ids=IDS)
def test_theta_limits(case, theta):
    C = W.cost(*case)
    lib = native().load()
    old = lib.dsvgd_w2_set_theta(theta)
    try:
        assert lib.dsvgd_w2_set_theta(theta) == theta    # accepted at the limit
        res = Problem(C).solve()
    finally:
        lib.dsvgd_w2_set_theta(old)
    assert lib.dsvgd_w2_set_theta(old) == old
    record_parity(check(res, case, C), rounds=res.rounds, phases=int(res.trace[-1, 1]))


def test_theta_out_of_range_is_ignored():
    lib = native().load()
    old = lib.dsvgd_w2_set_theta(1.999)
    try:
        assert lib.dsvgd_w2_set_theta(1024.5) == old
        assert lib.dsvgd_w2_set_theta(float("nan")) == old
    finally:
        assert lib.dsvgd_w2_set_theta(old) == old


# ----------------------------------------------------------- forced stall --
@pytest.mark.parametrize("case", [("uniform", m, R) for (m, R) in W.STALL_SHAPES], ids=IDS)
def test_forced_stall(case):
    """The helpers exit at once: the tail gives up, turns itself off and the
    bid rounds finish the solve within the same bounds.  (Uniform costs: the
    svgd family's 65 x 65 solve ends in the bid rounds before any tail runs,
    so it has nothing to stall.)"""
    C = W.cost(*case)
    old = switch("dsvgd_w2_set_tail_debug", 1)
    try:
        res = Problem(C).solve()
    finally:
        switch("dsvgd_w2_set_tail_debug", old)
    assert res.stats[5] >= 1, res.stats
    record_parity(check(res, case, C), rounds=res.rounds, stalls=res.stats[5])


# ----------------------------------------------------------------- errors --
def _good_after(p, case, C):
    """The workspace still solves after a refused or failed call."""
    p.set_cost(C)
    return check(p.solve(), case, C, what="after the error")


def test_refused_before_any_launch():
    N = native()
    case = ("uniform", 13, 5)
    C = W.cost(*case)
    p = Problem(C)
    p.assign.fill_(-7)
    for kw, msg in [(dict(m=12), "multiple of m"), (dict(ldc=64), "sizes"),
                    (dict(max_rounds=0), "max_rounds"),
                    (dict(entry="warm", prev=None), "null prev_assign"),
                    (dict(warm_phases=-1), "warm_phases"),
                    (dict(entry="stat", warm_phases=-1, cstat=True), "warm_phases")]:
        with pytest.raises(N.NativeError, match=msg):
            p.solve(**kw)
    # n / m = 33 slots per row
    q = Problem(np.ones((1, 33), np.float32))
    with pytest.raises(N.NativeError, match="<= 32"):
        q.solve()
    assert np.all(p.assign.cpu().numpy() == -7) and np.all(q.assign.cpu().numpy() == -7)
    record_parity(_good_after(p, case, C))


@pytest.mark.parametrize("bad", [-1.0, float("inf"), NAN], ids=["negative", "inf", "nan"])
@pytest.mark.parametrize("case", [("uniform", 13, 5), ("uniform", 65, 1)], ids=IDS)
def test_bad_cost_is_a_return_code(case, bad):
    N = native()
    C = W.cost(*case)
    Cb = np.array(C)
    Cb[C.shape[0] - 1, C.shape[1] - 1] = bad
    p = Problem(Cb)
    with pytest.raises(N.NativeError, match="non-finite or negative cost"):
        p.solve()
    record_parity(_good_after(p, case, C))


def test_no_convergence_is_a_return_code():
    N = native()
    case = ("uniform", 2049, 1)
    C = W.cost(*case)
    p = Problem(C)
    with pytest.raises(N.NativeError, match="no convergence"):
        p.solve(max_rounds=1)
    record_parity(_good_after(p, case, C))


# ---------------------------------------------------------- dsvgd_w2_grad --
SENTINEL = np.float32(-1234.5)


def _wide(A, extra):
    """A as the leading columns of a wider device buffer full of SENTINEL."""
    buf = torch.full((A.shape[0], A.shape[1] + extra), float(SENTINEL), dtype=torch.float32,
                     device=DEV)
    buf[:, :A.shape[1]] = torch.from_numpy(A).to(DEV)
    return buf


@pytest.mark.parametrize("h", [1.0, -2.5])
@pytest.mark.parametrize("m,R,d", W.GRAD_SHAPES)
def test_grad(m, R, d, h):
    """Plans made here (none optimal), X, Y and G as views of wider buffers
    whose pads keep their bits; the contiguous call gives the same bits.
    m d = 255 and 65 x 257 sit on either side of a 256-thread block."""
    N = native()
    n = m * R
    X, Y = W.grad_inputs(m, R, d)
    worst = 0.0
    for kind in W.GRAD_PLANS:
        plan = W.grad_plan(kind, n)
        pd = torch.as_tensor(plan, device=DEV)
        Xw, Yw = _wide(X, 3), _wide(Y, 2)
        Gw = _wide(np.full((m, d), SENTINEL, np.float32), 5)
        N.call("dsvgd_w2_grad", N.ptr(Xw), d + 3, m, N.ptr(Yw), d + 2, n, d, N.ptr(pd), h,
               N.ptr(Gw), d + 5, stream())
        Xc, Yc = torch.from_numpy(X).to(DEV), torch.from_numpy(Y).to(DEV)
        Gc = torch.full((m, d), float(SENTINEL), dtype=torch.float32, device=DEV)
        N.call("dsvgd_w2_grad", N.ptr(Xc), d, m, N.ptr(Yc), d, n, d, N.ptr(pd), h, N.ptr(Gc), d,
               stream())
        torch.cuda.synchronize()
        G = Gw.cpu().numpy()
        ratio = W.grad_ratio(G[:, :d], X, Y, plan, h)
        assert ratio <= 1.0, (kind, ratio)
        worst = max(worst, ratio)
        assert np.all(G[:, d:] == SENTINEL)
        assert np.all(Xw.cpu().numpy()[:, d:] == SENTINEL) and np.all(Yw.cpu().numpy()[:, d:] == SENTINEL)
        np.testing.assert_array_equal(Xw.cpu().numpy()[:, :d], X)
        np.testing.assert_array_equal(Gc.cpu().numpy().view(np.uint32),
                                      np.ascontiguousarray(G[:, :d]).view(np.uint32))
        np.testing.assert_array_equal(pd.cpu().numpy(), plan)
    record_parity(worst)
