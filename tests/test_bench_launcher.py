"""CPU: bench.py's own rank launcher (`--gpus N` without torchrun) and CPU channel, rehearsed with
--dry-run (no device): N fresh rank processes rendezvous over gloo, time between barriers, take the
max over ranks, and rank 0 prints one JSON line with n_gpus = N.  The same under
torch.distributed.run (the driver's multi-GPU launcher)."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _last_json(out):
    return json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])


def test_bench_spawns_its_own_ranks():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--steps", "3",
                          "--warmup", "1"], capture_output=True, text=True, timeout=240,
                         env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
    assert out.returncode == 0, out.stderr[-2000:]
    line = _last_json(out.stdout)
    assert line["n_gpus"] == 2 and line["ranks_launched_by"] == "bench.py"
    assert line["ms_per_step"] >= 2.0  # the max over ranks (rank 1 sleeps 2 ms per step)


def test_bench_plain_run_options(tmp_path):
    """--full is off unless asked for, and --dump-outputs writes the step's arrays as finite float32,
    the losses that are not finite marked in a file of their own."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    args = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert (args.full, args.dump_outputs, args.steps, args.warmup) == (False, None, 3, 1)
    args = bench.parse_args(["--steps", "3", "--full", "--dump-outputs", str(tmp_path / "out")])
    assert args.full and args.dump_outputs == str(tmp_path / "out")
    loss = np.array([0.25, np.inf, 3.0, -np.inf, np.nan, 3.0e38], dtype=np.float32)
    comp = np.array([True, False, True, True, True, True])
    bench.dump_outputs(args.dump_outputs, loss, comp)
    got = {n: np.load(tmp_path / "out" / f"{n}.npy") for n in ("loss", "loss_nonfinite", "complete")}
    assert all(a.dtype == np.float32 and a.shape == (6,) and np.isfinite(a).all() for a in got.values())
    assert np.array_equal(got["loss"], np.array([0.25, 0.0, 3.0, 0.0, 0.0, 3.0e38], dtype=np.float32))
    assert np.array_equal(got["loss_nonfinite"], [0.0, 1.0, 0.0, 2.0, 3.0, 0.0])
    assert np.array_equal(got["complete"], [1.0, 0.0, 1.0, 1.0, 1.0, 1.0])


def test_bench_under_torchrun():
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
                          "--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1"],
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    line = _last_json(out.stdout)
    assert line["n_gpus"] == 2 and line["ranks_launched_by"] == "launcher"
