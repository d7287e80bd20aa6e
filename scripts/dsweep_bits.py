"""Bit-for-bit record of the D-sweep diagnostics (csrc/dsweep.hpp, ksd.hip,
mmd.hip) for comparing two builds of the library on one GPU.

    python scripts/dsweep_bits.py dump OUT.npz [--lib LIBRARY]
    python scripts/dsweep_bits.py compare A.npz B.npz

dump runs every parametrisation of test_ksd_matches_fp64_median_bandwidth,
test_ksd_row_block, test_mmd_matches_fp64 and test_mmd_forced_slice_counts
through the tests' own helpers and keeps `out`, the rows and the raw slot
workspace P.  P is filled with a constant before the recorded evaluation, so
the slots that a sweep leaves alone compare too.  compare prints, per case, the
byte count and whether the two files agree byte for byte.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "dist-svgd_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

FILL = -123.0


def _params(fn, name):
    """The argument tuples of one pytest.mark.parametrize of a test."""
    return next(m.args[1] for m in fn.pytestmark if m.args[0] == name)


def dump(path, lib):
    import dsvgd
    if lib:
        dsvgd._native.LIB_PATH = os.path.abspath(lib)
    import mmd_reference as R
    import test_gpu_ksd as K
    import test_gpu_mmd as M
    rec = {}

    def keep(case, eng, W, rerun, names):
        W["P"].fill_(FILL)
        res = rerun()
        for name, v in zip(names, res):
            rec["%s/%s" % (case, name)] = v.cpu().numpy()
        rec["%s/P" % case] = W["P"].cpu().numpy()

    for n, d in _params(K.test_ksd_matches_fp64_median_bandwidth, "n,d"):
        for off in (False, True):
            eng = K._run(*K._scores(*K._problem(n, d, off)))[0]
            keep("ksd n=%d d=%d offcentre=%d" % (n, d, off), eng, eng._ksd,
                 lambda: eng.ksd(rows=True), ("out", "rows"))
    for m, row0 in _params(K.test_ksd_row_block, "m,row0"):
        X, target = K._problem(513, 64)
        h = float(np.float32(K.median_h64(X)))
        eng = K._run(*K._scores(X, target), h=h, m=m, row0=row0)[0]
        keep("ksd row block m=%d row0=%d" % (m, row0), eng, eng._ksd,
             lambda: eng.ksd(rows=True), ("out", "rows"))
    cases = [(s, k, o, None) for s in R.SHAPES for k in sorted(R.KERNELS) for o in (False, True)]
    cases += [(s, k, True, p) for s in R.SLICE_SHAPES for p in R.FORCED for k in sorted(R.KERNELS)]
    for (n, m, d), kernel, off, parts in cases:
        P, Q = R.problem(n, m, d, off)
        for h in (None, R.fixed_h(P, Q)):
            eng = M._run(P, Q, kernel, h, parts)[0]
            keep("mmd n=%d m=%d d=%d %s offcentre=%d parts=%s h=%s"
                 % (n, m, d, kernel, off, parts, "median" if h is None else "fixed"), eng,
                 eng._mmd, lambda: eng.mmd(n, rows=True, parts=parts),
                 ("out", "rp", "rq", "witness"))
    np.savez(path, **rec)
    print("%d arrays of %d cases -> %s" % (len(rec), len({k.split("/")[0] for k in rec}), path))


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), "the two files hold different cases"
    total, bad = 0, 0
    for case in sorted({k.split("/")[0] for k in A.files}):
        keys = sorted(k for k in A.files if k.split("/")[0] == case)
        nbytes = sum(A[k].nbytes for k in keys)
        same = all(A[k].tobytes() == B[k].tobytes() for k in keys)
        total += nbytes
        bad += not same
        print("%-66s %s %9d bytes  %s" % (case, ",".join(k.split("/")[1] for k in keys), nbytes,
                                         "equal" if same else "DIFFERENT"))
    print("%d bytes in %d arrays: %s" % (total, len(A.files),
                                         "all equal" if not bad else "%d cases DIFFER" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[4] if len(sys.argv) > 4 and sys.argv[3] == "--lib" else None)
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
