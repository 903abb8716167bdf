"""`python bench.py --gpus N` must really run N ranks (round-1 finding: the flag was parsed and ignored) on the FIXED global
grid (strong scaling, north_star; round-2 finding: the bench only scaled weakly).  The GPU box has ONE GPU, so the N ranks share
it (ICAR_BENCH_BACKEND=gloo: the library's host-staged halo transport, icar_hip_comm_init_host) -- a functional check of the
spawn + decomposition + halo path of the bench, never a performance number; with RCCL the same command line needs N GPUs and
says so."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "2", "--warmup", "1", "--nx", "64", "--ny", "48", "--nz", "12", "--no-cpu-baseline"]


def _run(args, env_extra, timeout=600):
    env = dict(os.environ); env.update(env_extra)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=timeout)


def _line(r):
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, f"no JSON line:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    return json.loads(lines[-1])


@pytest.mark.parametrize("n,decomp", [(2, "2x1"), (4, "2x2"), (8, "4x2")])
def test_bench_gpus_n_spawns_n_ranks_on_the_fixed_global_grid(n, decomp):
    r = _run(["--gpus", str(n)] + SMALL, {"ICAR_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-3000:]
    out = _line(r)
    assert out["n_gpus"] == n and out["config"]["decomposition"] == decomp and out["config"]["backend"].startswith("host-staged")
    # the transport proved itself before the timed region: it connects n images and every halo cell got its neighbour's stamp
    assert out["config"]["ranks_seen"] == n and out["config"]["halo_check"] == "ok"
    assert out["scaling"] == "strong" and out["config"]["global_grid"] == [64, 48, 12]
    # value = cells all ranks own (the interior of the GLOBAL grid, whatever N) x steps / time
    cells = out["value"] * out["ms_per_step"] * 1e-3
    assert abs(cells - 62 * 46 * 12) < 1e-6 * 62 * 46 * 12 and out["steps"] == 2


def test_bench_weak_scaling_keeps_the_tile():
    out = _line(_run(["--gpus", "2", "--scaling", "weak"] + SMALL, {"ICAR_BENCH_BACKEND": "gloo"}))
    assert out["scaling"] == "weak" and out["config"]["global_grid"] == [128, 48, 12] and out["config"]["decomposition"] == "2x1"


def test_bench_north_star_grid_on_eight_images():
    """the literal 512 x 512 x 40 of north_star split 2 x 4 (what the driver's 8-GPU run launches), 8 images sharing the GPU"""
    r = _run(["--gpus", "8", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"], {"ICAR_BENCH_BACKEND": "gloo"}, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _line(r)
    assert out["n_gpus"] == 8 and out["config"]["decomposition"] == "2x4" and out["config"]["global_grid"] == [512, 512, 40]
    assert out["config"]["tile_memory"][0] in (257, 258) and out["config"]["tile_memory"][2] in (129, 130)
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 - 510 * 510 * 40) < 1.0


def test_bench_single_rank_times_the_same_path():
    out = _line(_run(["--gpus", "1"] + SMALL, {}))
    assert out["n_gpus"] == 1 and out["config"]["decomposition"] == "1x1"
    assert out["config"]["ranks_seen"] == 1 and out["config"]["halo_check"].startswith("not applicable")
    assert "second stream" in out["config"]["halo"] and "self-exchange" in out["config"]["halo"]


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    env = dict(os.environ); env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"] + SMALL, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_bench_under_the_launcher_with_one_rank_initialises_rccl():
    """The driver's N > 1 launch line with N = 1 (all the one-GPU box allows): torch.distributed.run -> the nccl process group ->
    HaloComm.attach broadcasts the unique id and calls icar_hip_comm_init (ncclCommInitRank) -> update_dt all-reduces the CFL
    maximum over RCCL on the device.  The same code path as 8 ranks, minus the peers."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1"] + SMALL
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _line(r)
    assert out["n_gpus"] == 1 and out["config"]["backend"] == "rccl" and out["value"] > 0
    assert out["config"]["ranks_seen"] == 1 and out["config"]["halo_check"] == "ok"      # ncclCommCount, self-ring exchange checked


def test_bench_refuses_a_degraded_transport_when_a_gpu_per_rank_is_there():
    """An image whose ncclCommInitRank fails must not leave the others in a different transport: the outcome is agreed on over the
    launcher's process group, every image drops its communicator and all open the host-staged one (icar_amd/halo.py) -- and the
    BENCH then refuses to time it: with a GPU per rank a host-staged number must never pass for an RCCL one.  It prints an error
    line and exits non-zero."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "_rccl_fallback_child.py"), "--gpus", "1"] + SMALL
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode != 0
    out = _line(r)
    assert out["error"] == "transport self-check failed" and out["degraded_to_host_staged"] is True and "value" not in out
    assert out["halo_check"] == "ok" and out["ranks_seen"] == 1          # the host-staged transport itself works; it is refused for what it is


def test_a_failed_rccl_init_is_an_error_unless_the_host_transport_is_asked_for():
    """a library user whose RCCL communicator cannot be opened gets an error on every image, not a silent run on
    the ~100x slower host-staged transport; ICAR_ALLOW_HOST_STAGED=1 (previous test) is the explicit opt-in."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "ICAR_ALLOW_HOST_STAGED"):
        env.pop(k, None)
    env["ICAR_TEST_STRICT_TRANSPORT"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "_rccl_fallback_child.py"), "--gpus", "1"] + SMALL
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode != 0
    assert "ICAR_ALLOW_HOST_STAGED=1" in r.stderr and "RCCL communicator is not available on every image" in r.stderr
    assert '"value"' not in r.stdout


def test_bench_plain_line_carries_the_headline_and_full_the_rest():
    """A plain run does only what the headline needs; --full adds the figures that take runs of their own."""
    plain = _line(_run(["--gpus", "1"] + SMALL, {}))
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(plain) and plain["steps"] == 2
    assert not {"roofline", "microphysics", "later_window", "cpu_baseline"} & set(plain)
    full = _line(_run(["--gpus", "1", "--full"] + SMALL, {}))
    assert full["roofline"]["avg_ms"] > 0 and full["microphysics"]["ms_per_step"] > 0 and full["steps"] == 2
    assert 0.0 < full["config"]["mp_active_column_fraction"] <= 1.0


def test_bench_dump_outputs_repeat_bit_for_bit(tmp_path):
    """--dump-outputs: two runs with the same arguments write the same arrays, float32 / float64, a sample of the larger fields"""
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--nx", "96", "--ny", "96", "--nz", "40"]
    for run in ("a", "b"):
        r = _run(args + ["--dump-outputs", str(tmp_path / run)], {})
        assert r.returncode == 0, r.stderr[-3000:]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "water_vapor.npy" in names and "dt.npy" in names
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and a.dtype == b.dtype and a.shape == b.shape, n
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{n}: the two runs differ"
        total += a.nbytes
    assert np.load(tmp_path / "a" / "water_vapor.npy").size == 1 << 18       # 96 x 40 x 96 cells: the fixed sample
    assert total <= 64 << 20
