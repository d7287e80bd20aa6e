"""bench.py contract: the roofline traffic comes from the phi_mm launches of the
committed PMC summary, and the multi-rank path (barrier, max-over-ranks time,
one JSON line from rank 0) runs under torch.distributed.run."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_pmc_traffic_picks_phi_mm():
    """The quoted traffic is phi_mm's: on the symmetric layout phi_w1<4> (one
    launch per row), or with the two-launch form the sum of phi_w1<1>
    (transposed K-steps) and phi_w1<2> (the rest) of the same step -- never a
    logreg launch -- and nothing when a launch of the pair is missing."""
    import bench
    summ = os.path.join(ROOT, "profiles", "latest_summary.json")
    if not os.path.exists(summ):
        pytest.skip("no committed PMC summary")
    with open(summ) as f:
        ks = json.load(f)["kernels"]
    w1 = "_ZN5dsvgd13phi_w1_kernelILi1E"
    w2 = "_ZN5dsvgd13phi_w1_kernelILi2E"

    def per_launch(prefix):
        hit = [v["hbm_bytes_per_launch"] for k, v in ks.items()
               if k.startswith(prefix) and "hbm_bytes_per_launch" in v]
        return hit[0] if hit else None

    a, b = per_launch(w1), per_launch(w2)
    both, src = bench.pmc_traffic([w1, w2])
    if a is None or b is None:
        assert both is None   # a launch of the pair missing: nothing quoted
    else:
        assert both == a + b
        assert src == os.path.join("profiles", "latest_summary.json")
    assert bench.pmc_traffic(["no-such-kernel"]) == (None, None)
    w4 = "_ZN5dsvgd13phi_w1_kernelILi4E"   # the one-launch form (default since round 5)
    c = per_launch(w4)
    assert bench.pmc_traffic([w4])[0] == c
    lr = [k for k in ks if "logreg" in k and "hbm_bytes_per_launch" in ks[k]]
    if lr and a is not None:
        assert all(not k.startswith(w1) for k in lr)


def _env():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    return env


@pytest.mark.parametrize("n", [2, 4])
def test_bench_launches_its_own_ranks(n):
    """`python bench.py --gpus N` with no launcher starts N ranks itself
    (VERDICT r2 next #1): every rank joins one process group of N, rank 0
    prints the one line.  --launch-check stops before any GPU work, so this
    runs on the CPU."""
    cmd = [sys.executable, "bench.py", "--gpus", str(n), "--backend", "gloo", "--launch-check"]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and sorted(out["ranks"]) == list(range(n))


def test_bench_rejects_world_size_mismatch():
    """A launcher that starts fewer ranks than --gpus asks for is an error,
    not a silent one-GPU measurement."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29771", "bench.py", "--gpus", "4",
           "--backend", "gloo", "--launch-check"]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=240)
    assert r.returncode != 0


@pytest.mark.gpu
def test_bench_self_launch_two_ranks_gloo():
    """`python bench.py --gpus 2` (the driver's form) measures two ranks."""
    cmd = [sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--particles", "4096", "--dim", "64", "--data-rows", "1024", "--backend", "gloo",
           "--full"]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["process_group"]["world_size_seen"] == 2
    # all_scores with the logreg target: the own block's scores over the
    # gathered data, the score blocks all-gathered (DistSampler gather_data)
    assert "allgather_x" in out["stages_ms"] and "allgather_scores" in out["stages_ms"]
    assert out["multi_gpu"]["scores_gathered_data"] == [True, True]
    assert "hist_allreduce" in out["stages_ms"]


@pytest.mark.gpu
def test_bench_two_ranks_gloo():
    """2 ranks sharing cuda:0, gloo exchange: the N>1 timing/reporting path,
    at a shape where the pair-split layout applies (d = 256, m = 4096), with
    the self-describing multi-GPU keys: the layout each
    rank ran, the route probe, the first-step check, per-rank exchange times."""
    env = _env()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29763", "bench.py", "--gpus", "2",
           "--steps", "2", "--warmup", "1", "--particles", "8192", "--dim", "256",
           "--data-rows", "1024", "--backend", "gloo", "--full"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2
    assert out["config"]["particles_per_gpu"] == 4096
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 8192 * 2 / (out["ms_per_step"] * 2e-3)) < 1e-6 * out["value"]
    mg = out["multi_gpu"]
    assert mg["world_size"] == 2 and mg["backend"] == "gloo"
    assert mg["pair_split_engaged"] == [True, True] and mg["route_probe_ok"] == [True, True]
    assert mg["pair_split_first_step_check"] <= mg["pair_split_check_tol"] == 1e-5
    assert mg["scores_gathered_data"] == [True, True]
    assert len(mg["exchange_ms_per_rank"]) == 2
    for ex in mg["exchange_ms_per_rank"]:
        for k in ("allgather_x", "allgather_scores", "hist_allreduce", "partials_wait"):
            assert k in ex and ex[k] >= 0.0
    assert out["roofline"]["traffic"] is None   # N=1 PMC summary is not quoted at N>1
    assert "cpu_baseline" not in out


def test_dump_rows_fixed_sample():
    """--dump-outputs keeps every particle row while they fit the budget and
    else the same sorted sample on every call; the headline shape's dump stays
    under the 64 MB a dump may hold."""
    import numpy as np

    import bench
    assert np.array_equal(bench.dump_rows(4096, 64), np.arange(4096))
    a, b = bench.dump_rows(65536, 256), bench.dump_rows(65536, 256)
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0)
    assert 0 <= a[0] and a[-1] < 65536 and len(a) < 65536
    assert len(a) * 256 * 4 + 2 * 8 + 2 * 128 <= 64e6      # both arrays and their .npy headers


HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY_KEYS = ("roofline", "stages_ms", "passes", "cpu_baseline", "multi_gpu")


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(tmp_path):
    """A plain run prints the headline line without the --full sections and
    --dump-outputs writes the particles after the last timed step (float32)
    and that step's median and bandwidth (float64): the same sampler stepped
    warmup + steps times in this process arrives at the same arrays."""
    import numpy as np
    import torch

    import bench
    import dsvgd
    n, d, rows, warm, steps = 4096, 64, 1024, 1, 2
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warm),
           "--particles", str(n), "--dim", str(d), "--data-rows", str(rows),
           "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert all(k in out for k in HEADLINE_KEYS) and not any(k in out for k in FULL_ONLY_KEYS)
    assert out["steps"] == steps and out["ms_per_step"] > 0
    assert abs(out["value"] - n * steps / (out["ms_per_step"] * steps * 1e-3)) < 1e-6 * out["value"]
    got = np.load(tmp_path / "dump" / "particles.npy")
    bw = np.load(tmp_path / "dump" / "bandwidth.npy")
    assert got.dtype == np.float32 and got.shape == (n, d) and np.isfinite(got).all()
    assert bw.dtype == np.float64 and bw.shape == (2,) and (bw > 0).all()

    x, t = bench.synthetic_data(rows, d - 1)
    gen = torch.Generator(device="cpu").manual_seed(0)
    parts = (0.1 * torch.randn(n, d, generator=gen)).to("cuda:0")
    start = parts.cpu().numpy().copy()
    sampler = dsvgd.DistSampler(0, 1, dsvgd.targets.LogisticRegression(x, t, gemm="h2"),
                                dsvgd.RBF("median"), parts, rows, rows,
                                exchange_particles=True, exchange_scores=True,
                                include_wasserstein=False, order="jacobi")
    for _ in range(warm + steps):
        sampler.make_step(1e-4)
    torch.cuda.synchronize()
    want = sampler.particles.cpu().numpy()
    eng = sampler._engines[next(iter(sampler._engines))]
    med, h, _ = eng.state.read()
    # graph replay here, plain launches in the timed steps: phi may differ in
    # its last bits (1e-3 of the move is generous), and each step's x += eps*phi
    # rounds once more (one fp32 ulp of the particles' scale per step)
    moved = np.abs(want - start).max()
    err = np.abs(got - want).max()
    tol = (warm + steps) * 2.0 ** -23 * np.abs(want).max() + 1e-3 * moved
    print("dump vs in-process: err %.3g tol %.3g moved %.3g" % (err, tol, moved))
    assert moved > 0 and err <= tol
    assert abs(bw[0] - med) <= 1e-5 * med and abs(bw[1] - h) <= 1e-5 * h
