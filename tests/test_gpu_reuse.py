"""A step depends only on its inputs, not on what the engine ran before.

A Sampler, a DistSampler rank or the benchmark builds one PhiEngine (or one
cached sweep workspace) and calls it thousands of times, mostly through a
captured HIP graph; the other tests build a fresh engine per input.  Here:

  1. one PhiEngine runs a sequence of very different inputs (ordinary; every
     power-of-two scale shifted; an outlier that trips the range guard; all
     particles identical, which overflows the bracket's slots; a NaN row), every
     float buffer it owns filled with NaN patterns between the steps, and each
     step is bit for bit the step of a fresh engine that saw only that input;
     the last step also against the fp64 oracle and the exact median, so that
     two identically wrong engines cannot pass;
  2. a DistSampler replays its captured graph across the same changes of input
     (the guard and the select's fallback flip on the device, in both
     directions) beside a twin that launches every step eagerly: same bits;
  3. a captured sequential sweep keeps its workspace alive when a sweep of
     another shape goes through the module's cache.

Comparisons between engines are bit for bit (fixed summation orders, integer
atomics only); the oracle comparison uses test_gpu_split.py's PHI_TOL.
"""
import math
import weakref

import numpy as np
import pytest
import torch

from conftest import record_parity
from oracle import svgd_oracle as O
from test_gpu_range import _outlier_case, row_err
from test_gpu_split import PHI_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dsvgd():
    import dsvgd as m
    return m


def gpu(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


# ------------------------------------------------------------- 1. engine --
# the smallest shapes that reach each set of kernels; `want`: the path the
# engine must have resolved to (phi_form, sym, bracketed, fused_scales,
# phi_gemm, gram_gemm)
H_ROWS = 60.0     # w-rows' fixed bandwidth (test_gpu_phi_wform.py's at d = 256)
CONFIGS = {
    # sqdist_direct, phi_direct, hist select
    "direct": dict(n=300, d=2, kw={}, want=("xs", False, False, False, "h2", "h2")),
    # exact MFMA, partial tiles
    "f32": dict(n=300, d=37, kw=dict(gemm="f32"), want=("xs", False, False, False, "f32", "f32")),
    # FmtX3 Gram and phi_mm
    "x3": dict(n=300, d=64, kw=dict(gemm="x3"), want=("xs", False, False, False, "x3", "x3")),
    # FmtH2 "xs", fused scales (ldy = 128: the full layout -- the symmetric one
    # needs ldy % 256 == 0, which h2-bracket and unfused have on "xs")
    "h2": dict(n=300, d=64, kw={}, want=("xs", False, False, True, "h2", "h2")),
    # one-operand form, symmetric
    "w": dict(n=300, d=256, kw=dict(phi_form="w"), want=("w", True, False, True, "h2", "h2")),
    # row block off the 256 grid, fixed h
    "w-rows": dict(n=512, d=256, m=128, row0=256, h=H_ROWS, kw=dict(phi_form="w"),
                   want=("w", False, False, True, "h2", "h2")),
    # a row block's own median
    "w-local": dict(n=512, d=256, m=128, row0=256, kw=dict(phi_form="w", local_median=True),
                    want=("w", False, False, True, "h2", "h2")),
    # bracketed select (m n = 2^24), symmetric
    "w-bracket": dict(n=4096, d=256, kw=dict(phi_form="w"),
                      want=("w", True, True, True, "h2", "h2")),
    "h2-bracket": dict(n=4096, d=256, kw={}, want=("xs", True, True, True, "h2", "h2")),
    # d > 1024: colscale_guarded, pack_wide (test_unfused_scales_path_has_the_guard's d)
    "unfused": dict(n=160, d=1100, kw={}, want=("xs", True, False, False, "h2", "h2")),
}
IDS = list(CONFIGS)
NAN_ROW = 5

# buffers poisoned between steps: everything float-valued the engine owns.  Not
# the SelectStates, `cand` (its head holds the slots' counts), the pair-split
# plan arrays and _ksd: counts, ranks and indices -- a stale value there is
# caught by the sequence itself, a poisoned one could send a kernel out of bounds
FLOAT_BUFS = ("Y", "norms", "D", "KY", "rowsum", "phi", "mean", "yscale", "wscale", "rsc",
              "sample", "scale_ws")
STAT_BUFS = ("colmax", "gmax")            # int32 images of float magnitudes
IMAGES = ("Yx", "Wh", "Yg", "Yx3")        # int16 images: fp16 (FmtH2) or bf16 (FmtX3)
NAN_F32, NAN_F16, NAN_BF16 = 0x7FC00000, 0x7E00, 0x7FC0


def _poison(eng):
    fmt = {"Yx": eng.phi_gemm, "Wh": "h2", "Yg": eng.gram_gemm, "Yx3": "x3"}
    done = []
    for name in FLOAT_BUFS:
        t = getattr(eng, name, None)
        if t is not None:
            assert t.dtype == torch.float32
            t.fill_(float("nan"))
            done.append(name)
    for name in STAT_BUFS:
        t = getattr(eng, name, None)
        if t is not None:
            assert t.dtype == torch.int32
            t.fill_(NAN_F32)
            done.append(name)
    for name in IMAGES:
        t = getattr(eng, name, None)
        if t is not None:
            assert t.dtype == torch.int16
            t.fill_(NAN_F16 if fmt[name] == "h2" else NAN_BF16)
            done.append(name)
    return done


_inputs_cache, _fresh_cache, _oracle_cache = {}, {}, {}


def _inputs(cfg, kind):
    """A: ordinary.  B1: A with X 2^10, S 2^-10 (every power-of-two scale, norm
    and bandwidth differs).  B2: one particle 2^24 away with scores 2^24 larger
    (the range guard).  B3: all particles identical (median 0, h = 1; the
    bracket's slots overflow).  B4: A with one particle row NaN."""
    c = CONFIGS[cfg]
    n, d = c["n"], c["d"]
    key = (n, d, kind)
    if key not in _inputs_cache:
        rs = np.random.RandomState(n + d)
        X = rs.randn(n, d).astype(np.float32)
        S = (-X + 0.3 * rs.randn(n, d)).astype(np.float32)
        if kind == "B1":
            X, S = X * np.float32(2.0 ** 10), S * np.float32(2.0 ** -10)
        elif kind == "B2":
            X, S = _outlier_case(n, d, "far_score", 24)
        elif kind == "B3":
            X = np.ones((n, d), np.float32)
            S = np.random.RandomState(n + d + 1).randn(n, d).astype(np.float32)
        elif kind == "B4":
            X[NAN_ROW] = np.nan
        else:
            assert kind == "A"
        _inputs_cache[key] = (X, S)
    return _inputs_cache[key]


def _engine(cfg):
    c = CONFIGS[cfg]
    eng = dsvgd().PhiEngine(c["n"], c["d"], m=c.get("m"), row0=c.get("row0", 0), device=DEV,
                            **c["kw"])
    got = (eng.phi_form, eng.sym, eng.bracketed, eng.fused_scales, eng.phi_gemm, eng.gram_gemm)
    assert got == c["want"], (cfg, got)
    assert (eng.d <= eng.DIRECT_MAX_D) == (cfg == "direct")
    assert (eng.k_rank >= 0) == (cfg == "w-local")
    if cfg == "w-local":
        assert eng.k_rank == (eng.m * eng.n - 1) // 2
    return eng


def _fbits(*vals):
    """fp32 bit patterns (a NaN equals itself; the tests that may see one
    compare with _same_floats instead)."""
    return tuple(int(np.float32(v).view(np.uint32)) for v in vals)


def _run(eng, cfg, kind):
    """One step of `kind` on `eng`; what a step leaves behind, cloned."""
    X, S = _inputs(cfg, kind)
    Xo = torch.zeros(eng.m, eng.d, device=DEV)
    eng.step(gpu(X), gpu(S), X_own=Xo, step=0.5, h=CONFIGS[cfg].get("h"))
    torch.cuda.synchronize()
    out = dict(state=eng.state.read(), D=eng.dense_D().clone(), phi=eng.phi.clone(), X_own=Xo,
               guard=eng.range_guard())
    if eng.bracketed:
        out["bracket"] = eng.state.bracket()
    return out


def _fresh(cfg, kind):
    """The step of a fresh engine that ran only this input (computed once)."""
    if (cfg, kind) not in _fresh_cache:
        _fresh_cache[cfg, kind] = _run(_engine(cfg), cfg, kind)
    return _fresh_cache[cfg, kind]


def _same_floats(a, b, nan):
    """Element for element; the select state's words may be NaN on both sides
    (a fixed bandwidth leaves the median NaN), tensors only where `nan`."""
    return all(x == y or (nan and math.isnan(x) and math.isnan(y)) for x, y in zip(a, b))


def _same_tensor(a, b, nan):
    if not nan:
        return torch.equal(a, b)
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _assert_same(got, ref, where, nan=False):
    assert _same_floats(got["state"], ref["state"], True), (where, got["state"], ref["state"])
    if "bracket" in ref:
        g, r = got["bracket"], ref["bracket"]
        assert _same_floats(g[:2], r[:2], nan) and g[2:] == r[2:], (where, g, r)
    assert got["guard"] == ref["guard"], (where, got["guard"], ref["guard"])
    for name in ("D", "phi", "X_own"):
        assert _same_tensor(got[name], ref[name], nan), (where, name)


def _oracle(cfg, h, kind="A"):
    """The fp64 phi of an input at bandwidth h (computed once per configuration)."""
    if (cfg, h, kind) not in _oracle_cache:
        c = CONFIGS[cfg]
        X, S = _inputs(cfg, kind)
        rows = np.arange(c["row0"], c["row0"] + c["m"]) if "m" in c else None
        _oracle_cache[cfg, h, kind] = (O.phi(X, S, h) if rows is None
                                       else O.phi(X, S, h, rows=rows))
    return _oracle_cache[cfg, h, kind]


def _check_against_oracle(cfg, eng, got):
    """The last A of a sequence: phi within PHI_TOL of the fp64 oracle
    (max-normalised, as test_gpu_phi_wform.py's test_phi_matches_oracle), and
    the bandwidth the exact lower median of the engine's own D over log n."""
    med, h, inv_h = got["state"]
    if "h" in CONFIGS[cfg]:
        assert h == CONFIGS[cfg]["h"]
    else:
        D = got["D"].cpu().numpy().ravel()
        k = (D.size - 1) // 2
        assert _fbits(med) == _fbits(np.partition(D, k)[k])
        # h = (float)(med / log n) and inv_h = 1 / h on the device: one fp32
        # rounding each (and the device's double log within an ulp of the host's)
        assert abs(h - med / math.log(eng.n)) <= 2.0 ** -23 * h
    assert abs(inv_h - 1.0 / h) <= 2.0 ** -23 * inv_h
    ref = _oracle(cfg, h)
    e = float(np.abs(got["phi"].cpu().numpy() - ref).max() / np.abs(ref).max())
    record_parity(e, cfg=cfg)
    assert e < PHI_TOL, (cfg, e)
    assert torch.equal(got["X_own"], 0.5 * got["phi"])     # X_own started at zero


@pytest.mark.parametrize("cfg", IDS)
def test_reused_engine_equals_fresh(cfg):
    """A, B1, B2, B3, A on one engine, every float buffer NaN between the
    steps: each step's select state, D, phi, moved rows and guard are the bits
    of a fresh engine that ran only that input.  B2 trips the range guard on
    the FmtH2 engines, B3 the select's fallback on the bracketed ones, and the
    A after them runs with both off again."""
    eng = _engine(cfg)
    h2 = eng.phi_gemm == "h2" and eng.d > eng.DIRECT_MAX_D
    got = None
    for k, kind in enumerate(("A", "B1", "B2", "B3", "A")):
        if k:
            poisoned = _poison(eng)
            assert {"Y", "norms", "D", "KY", "rowsum", "phi", "mean"} <= set(poisoned)
        got = _run(eng, cfg, kind)
        _assert_same(got, _fresh(cfg, kind), (cfg, k, kind))
        assert bool(torch.isfinite(got["phi"]).all()), (cfg, k, kind)
        if not h2:
            assert got["guard"] is None
        elif kind == "B2":
            # the step ran on the guard's fallback: right, not only repeatable
            # -- every row of the fp64 oracle's in test_gpu_range.py's
            # row-normalised form (the max-normalised one sees only the outlier)
            assert got["guard"] is True, cfg
            e = float(row_err(got["phi"].cpu().numpy(), _oracle(cfg, got["state"][1], "B2")).max())
            record_parity(e, cfg=cfg, kind=kind)
            assert e < PHI_TOL, (cfg, kind, e)
        elif kind == "A":          # (B1 and B3: whatever the fresh engine decided)
            assert got["guard"] is False, (cfg, k)
        if kind == "B3" and "h" not in CONFIGS[cfg]:
            assert got["state"][:2] == (0.0, 1.0)
        if eng.bracketed and kind in ("A", "B3"):
            # all identical: every entry in [0, 0], the slots overflow
            assert got["bracket"][4] == (1 if kind == "B3" else 0), (cfg, kind, got["bracket"])
    _check_against_oracle(cfg, eng, got)


@pytest.mark.parametrize("cfg", IDS)
def test_step_after_a_nan_row_is_clean(cfg):
    """A, B4, A: one particle row NaN (no loop bound of the select, bracket,
    centre or Gram kernels comes from a value a NaN can reach -- launch
    geometry, nslots and the slots' capacity bound them).  The NaN step equals
    the fresh engine's with NaN == NaN; the point is the A after it: the fresh
    engine's bits, and the oracle's phi."""
    eng = _engine(cfg)
    got = None
    for k, kind in enumerate(("A", "B4", "A")):
        if k:
            _poison(eng)
        got = _run(eng, cfg, kind)
        _assert_same(got, _fresh(cfg, kind), (cfg, k, kind), nan=kind == "B4")
        if kind == "B4":     # the input did reach phi
            assert bool(torch.isnan(got["phi"]).any())
        else:
            assert bool(torch.isfinite(got["phi"]).all())
    _check_against_oracle(cfg, eng, got)


# ------------------------------------------------------- 2. graph replay --
STEP = 1e-2
_targets = {}


def _target(d):
    if d not in _targets:
        rs = np.random.RandomState(1000 + d)
        _targets[d] = dsvgd().targets.Gaussian(rs.randn(d).astype(np.float32),
                                               rs.uniform(0.5, 2.0, d).astype(np.float32))
    return _targets[d]


def _sampler(n, d, order, graphs, X0, target=None):
    smp = dsvgd().DistSampler(0, 1, target or _target(d), dsvgd().RBF("median"),
                              gpu(X0).clone(), 1, 1,
                              exchange_particles=True, exchange_scores=False,
                              include_wasserstein=False, order=order)
    smp.graphs = graphs
    return smp


def _sequence(n, d):
    """The seven inputs of a replay test: (kind, particles)."""
    rs = np.random.RandomState(7 * n + d)
    ordinary = [rs.randn(n, d).astype(np.float32) for _ in range(5)]
    outlier = _outlier_case(n, d, "far_score", 24)[0]
    ident = np.ones((n, d), np.float32)
    return [("ordinary", ordinary[0]),     # eager
            ("ordinary", ordinary[1]),     # captured
            ("ordinary", ordinary[2]),     # first replay
            ("outlier", outlier), ("ordinary", ordinary[3]),
            ("identical", ident), ("ordinary", ordinary[4])]


def _engine_of(smp):
    return smp._engines[next(iter(smp._engines))]


def _replay_pair(n, d, order, seq=None, target=None):
    """(captured sampler, eager twin, per-step records) after the sequence:
    before each step both samplers' particles are set to the same tensor; after
    it their particles must be the same bits."""
    seq = seq or _sequence(n, d)
    cap = _sampler(n, d, order, True, seq[0][1], target)
    twin = _sampler(n, d, order, False, seq[0][1], target)
    records = []
    for k, (kind, P) in enumerate(seq):
        Pg = gpu(P)
        cap.particles = Pg
        twin.particles = Pg
        cap.make_step(STEP)
        twin.make_step(STEP)
        torch.cuda.synchronize()
        assert torch.equal(cap.particles, twin.particles), (n, d, order, k, kind)
        assert bool(torch.isfinite(cap.particles).all()) and not torch.equal(cap.particles, Pg)
        assert cap._graph is not None and (cap._graph.graph is not None) == (k >= 1), k
        assert twin._graph is None
        eg, et = _engine_of(cap), _engine_of(twin)
        assert eg is not et
        # (the sequential order takes only the bandwidth from its engine)
        guard = eg.range_guard() if order == "jacobi" else None
        rec = dict(kind=kind, state=eg.state.read(), guard=guard,
                   bracket=eg.state.bracket() if eg.bracketed else None)
        assert rec["state"] == et.state.read()
        assert order != "jacobi" or guard == et.range_guard()
        if eg.bracketed:
            assert rec["bracket"] == et.state.bracket()
        records.append(rec)
    return cap, twin, records


@pytest.mark.parametrize("n,d", [(4096, 256), (300, 256), (300, 64)])
def test_graph_replay_across_gated_branches(n, d):
    """Jacobi steps replayed from the captured graph while the device-gated
    branches flip: the range guard on for the outlier step and off again for
    the next, (n = 4096) the select's fallback on for identical particles and
    off again -- the bits of the eager twin after every step."""
    cap, twin, rec = _replay_pair(n, d, "jacobi")
    eng = _engine_of(cap)
    assert eng.phi_form == ("w" if d == 256 else "xs") and eng.phi_gemm == "h2"
    if n == 4096:
        assert eng.sym and eng.bracketed
    for k, r in enumerate(rec):
        assert r["guard"] is (r["kind"] == "outlier"), (k, r)
        if r["kind"] == "identical":
            assert r["state"][:2] == (0.0, 1.0), r
        if eng.bracketed and r["kind"] != "outlier":
            assert r["bracket"][4] == (1 if r["kind"] == "identical" else 0), (k, r)
    assert rec[3]["guard"] is True and rec[4]["guard"] is False


def test_graph_replay_guard_from_the_scores_alone():
    """The sampler packs X, then the scores (dsvgd_pack_h2 with X == NULL
    rewrites only the S half's statistics).  A step whose particles are
    ordinary but whose SCORES span more than 2^16 between rows must trip the
    guard from those words alone, and the next step must clear it -- under
    replay, with the bits of the eager twin.  N(mu, 1/lam) with lam_0 = 2^10:
    every particle at mu_0 in column 0 but one, 2^12 away, whose score there is
    2^22 against the others' largest of a few units; its X row is 2^12 against
    a few units, inside the 2^16 window."""
    n, d, j = 300, 64, 17
    rs = np.random.RandomState(41)
    mu = rs.randn(d).astype(np.float32)
    lam = rs.uniform(0.5, 2.0, d).astype(np.float32)
    lam[0] = 2.0 ** 10
    target = dsvgd().targets.Gaussian(mu, lam)
    ordinary = [rs.randn(n, d).astype(np.float32) for _ in range(4)]
    P = rs.randn(n, d).astype(np.float32)
    P[:, 0] = mu[0]
    P[j, 0] = mu[0] + np.float32(2.0 ** 12)
    # the construction, on the host: row maxima of the two halves of [Xc | S]
    for k, Q in enumerate(ordinary + [P]):
        rx = np.abs(Q - np.median(Q, axis=0)).max(1)
        rsc = np.abs(lam * (Q - mu)).max(1)
        assert rx.max() < 2.0 ** 14 * rx[rx > 0].min()
        assert (rsc.max() > 2.0 ** 18 * rsc.min()) == (k == 4)
        assert k == 4 or rsc.max() < 2.0 ** 14 * rsc.min()
    seq = [("ordinary", ordinary[0]), ("ordinary", ordinary[1]), ("ordinary", ordinary[2]),
           ("scores", P), ("ordinary", ordinary[3])]
    cap, twin, rec = _replay_pair(n, d, "jacobi", seq, target)
    eng = _engine_of(cap)
    assert eng.phi_form == "xs" and eng.phi_gemm == "h2" and eng.fused_scales
    assert [r["guard"] for r in rec] == [False, False, False, True, False]


@pytest.mark.parametrize("n,d", [(256, 96), (256, 8)])
def test_graph_replay_sequential_shares_scratch(n, d):
    """The same pair in the sequential order: d = 96 on the wide blocked sweep,
    d = 8 on the VALU one.  The captured sampler and the eager twin share the
    module's cached workspace and their steps alternate: those caches are
    pure scratch."""
    from dsvgd import engine as E
    cap, twin, rec = _replay_pair(n, d, "sequential")
    if d > 64:
        assert cap._sweep_hold["wide"] is twin._sweep_hold["wide"]
        assert (cap._sweep_hold["wide"].n, cap._sweep_hold["wide"].d) == (n, d)
    else:
        assert not cap._sweep_hold
        assert any(k[2] == d for k in E._GS_PARTIALS)
    assert rec[5]["state"][:2] == (0.0, 1.0)


# ------------------------------------------- 3. the workspace's lifetime --
def test_captured_sweep_keeps_its_workspace():
    """A sequential DistSampler's captured graph holds raw pointers into the
    wide sweep's workspace.  A sweep of another shape (a second DistSampler,
    then Sampler.sample) goes through the same module cache in between: the
    workspace must outlive it.  Checked on a weak reference BEFORE the graph is
    replayed again, so that a failing tree never replays through freed memory;
    then the next replay gives the bits of an eager twin that ran all its steps
    before the other shape arrived."""
    from dsvgd import engine as E
    n, d, n2, d2 = 256, 96, 384, 160
    X0 = np.random.RandomState(11).randn(n, d).astype(np.float32)
    twin = _sampler(n, d, "sequential", False, X0)
    for _ in range(4):
        twin.make_step(STEP)
    torch.cuda.synchronize()
    expected = twin.particles.detach().clone()
    del twin          # (it shares the cached workspace: only A may keep it alive)

    A = _sampler(n, d, "sequential", True, X0)
    for _ in range(3):
        A.make_step(STEP)
    torch.cuda.synchronize()
    assert A._graph is not None and A._graph.graph is not None
    mine = [W for W in E._WIDE.values() if (W.n, W.d) == (n, d)]
    assert len(mine) == 1
    ref = weakref.ref(mine[0])
    del mine

    X2 = np.random.RandomState(12).randn(n2, d2).astype(np.float32)
    B = _sampler(n2, d2, "sequential", True, X2)
    B.make_step(STEP)
    smp = dsvgd().Sampler(d2, _target(d2), dsvgd().RBF("median"))
    smp.sample(n2, 2, STEP, order="sequential", verbose=False)
    torch.cuda.synchronize()
    assert any((W.n, W.d) == (n2, d2) for W in E._WIDE.values())

    assert ref() is not None, "the captured graph's workspace was freed under it"
    A.make_step(STEP)
    torch.cuda.synchronize()
    assert torch.equal(A.particles, expected)


# ------------------------------------------------ 4. capture and the GC --
def test_capture_holds_the_cyclic_collector_off():
    """A dead reference cycle may hold device resources (a sampler's graph,
    streams, D); were it collected in the middle of another capture, its
    destructors would make calls a capturing stream does not permit.
    StepGraph collects before it captures and holds the collector off until
    the capture has ended; a DistSampler is no cycle, so it goes with its
    last reference.  (The cycle here holds plain Python objects only.)"""
    import gc
    from dsvgd.engine import StepGraph

    class Node(object):
        pass

    x = torch.zeros(64, device=DEV)
    seen, dead = [], []

    def fn():
        x.add_(1.0)
        seen.append((gc.isenabled(), dead[-1]() is None if dead else None))

    step = StepGraph(fn, torch.device(DEV))
    assert gc.isenabled()
    step()                                        # eager
    a, b = Node(), Node()
    a.other, b.other = b, a                       # a dead cycle by the time of the capture
    dead.append(weakref.ref(a))
    del a, b
    step()                                        # captured, then replayed
    step()                                        # replayed (fn does not run)
    torch.cuda.synchronize()
    assert step.graph is not None and gc.isenabled()
    assert seen == [(True, None), (False, True)]
    assert bool((x == 3.0).all())

    smp = _sampler(256, 8, "jacobi", True, np.zeros((256, 8), np.float32))
    smp.make_step(STEP)
    smp.make_step(STEP)
    torch.cuda.synchronize()
    assert smp._graph.graph is not None
    ref = weakref.ref(smp)
    del smp
    assert ref() is None
