"""DDP on the GPU over RCCL (world_size 1 on the single-GPU test box - RCCL
refuses two ranks on one device, see tools/diag/rccl_probe.py): the apex
ddp_race_condition_test pattern - many iterations with
many small buckets whose all-reduces REALLY run on RCCL (``force_collectives``:
the reducer issues them on the 1-rank communicator, on its high-priority
streams) while backward keeps producing grads behind a ``torch.cuda._sleep``
skew, every grad checked against a closed form right after backward, and the
bucket buffers consumed immediately by an in-place op.  The bf16 variant
reduces through a separate fp32 staging tensor, so a missing stream join shows
up as stale gradients."""
import math
import os

import pytest
import torch
import torch.distributed as dist

import dist_workers as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pg(tmp_path_factory):
    # file rendezvous (no port to race for on a shared box)
    rdzv = str(tmp_path_factory.mktemp("pg") / "rdzv")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="file://" + rdzv, rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


class _Skew(torch.autograd.Function):
    """Identity whose backward keeps the compute stream busy (~ms) before the
    gradients of the parameters behind it are produced (apex race test)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        torch.cuda._sleep(2_000_000)
        return g


class _Model(torch.nn.Module):
    def __init__(self, n=24, numel=4096 * 64, dtype=torch.float32):
        super().__init__()
        self.ps = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.full((numel,), float(i + 1), device="cuda", dtype=dtype))
             for i in range(n)])

    def forward(self, x):
        # d(loss)/d(p_i) = x * (i + 1): a closed form per param and iteration (exact in
        # bf16 too: small integers); every 5th parameter sits behind a sleep skew
        out = 0
        for i, p in enumerate(self.ps):
            xi = _Skew.apply(x) if i % 5 == 0 else x
            out = out + (p * xi.to(p.dtype) * (i + 1)).float().sum()
        return out


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ddp_race_condition(pg, streams, dtype):
    from apex_example_amd.parallel import DistributedDataParallel

    model = _Model(dtype=dtype)
    ddp = DistributedDataParallel(model, message_size=4096 * 64 * 2,
                                  num_allreduce_streams=streams, force_collectives=True,
                                  allreduce_always_fp32=(dtype == torch.bfloat16))
    assert ddp.reducer.collectives_active()
    bad = torch.zeros((), device="cuda")
    for it in range(60):
        x = torch.tensor(float(it % 7 + 1), device="cuda")
        for p in model.ps:
            if p.grad is not None:
                p.grad.zero_()
        ddp(x).backward()
        for i, p in enumerate(model.ps):
            bad += (p.grad.float() - x * (i + 1)).abs().max()
            p.grad.mul_(0.5)  # consume the bucket in place right away
    torch.cuda.synchronize()
    assert bad.item() == 0.0
    assert len(ddp.bucket_layout()) >= 6


class _ConvNet(torch.nn.Module):
    """Own-kernel convs (3x3 MFMA implicit GEMM, 1x1 GEMM) whose weight gradients run on
    the DDP side stream and write their bucket views directly, plus a SyncBN on the
    forced collective path: every gradient has a closed form.  With an all-ones input
    and loss k * sum(conv(x)), dW[co, r, s, ci] = k * (number of pixels whose tap (r, s)
    lands inside the image) - integers, exact in the fp32 sums, rounded to bf16 once."""

    def __init__(self):
        super().__init__()
        from apex_example_amd.ops.conv import Conv2d1x1, Conv2d3x3
        from apex_example_amd.parallel import SyncBatchNorm

        self.convs = torch.nn.ModuleList(
            [Conv2d3x3(64, 64) if i % 2 == 0 else Conv2d1x1(64, 128) for i in range(8)])
        self.convs.to(device="cuda", dtype=torch.bfloat16, memory_format=torch.channels_last)
        self.bn = SyncBatchNorm(64, force_collectives=True).cuda()

    def forward(self, x, z, ks, kb):
        out = 0
        for i, c in enumerate(self.convs):
            xi = _Skew.apply(x) if i % 3 == 0 else x
            out = out + ks[i] * c(xi).float().sum()
        return out + kb * self.bn(z).float().sum()


def test_ddp_race_condition_round4_defaults(pg, monkeypatch):
    """The race test on the DDP defaults: bf16 buckets on the rsag wire (fp32
    reduce-scatter + bf16 all-gather), own-kernel convs whose weight gradients run on the
    high-priority side stream and write the (lazily zeroed) bucket views directly, sleep
    skews on BOTH the compute and the side stream, SyncBN collectives in the same step,
    zero_grad through the optimizer (lazy zero) and a step that consumes the buckets;
    60 iterations, every gradient compared exactly with its closed form."""
    from apex_example_amd.ops import conv as C
    from apex_example_amd.optimizers import FusedSGD
    from apex_example_amd.parallel import DistributedDataParallel

    monkeypatch.setattr(C, "_TEST_SIDE_SLEEP", 1_000_000)
    torch.manual_seed(0)
    net = _ConvNet()
    ddp = DistributedDataParallel(net, message_size=64 * 64 * 9 * 2, force_collectives=True)
    assert ddp.reducer.collectives_active()
    opt = FusedSGD(net.parameters(), lr=0.0)  # reads (consumes) every bucket, moves nothing
    n, h, w = 2, 8, 8
    x = torch.ones(n, 64, h, w, device="cuda", dtype=torch.bfloat16).to(
        memory_format=torch.channels_last).requires_grad_(True)
    # +-1 per channel in equal numbers: mean 0, biased variance 1 exactly
    z = torch.ones(n, 64, h, w, device="cuda")
    z[:, :, :, w // 2:] = -1.0
    z = z.to(memory_format=torch.channels_last)
    cnt = torch.zeros(3, 3, dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            cnt[r, s] = n * (h - abs(r - 1)) * (w - abs(s - 1))
    assert ddp._fp32_mode() == 3 and "reduce-scatter" in ddp.wire_format()["torch.bfloat16"]
    bad = torch.zeros((), device="cuda", dtype=torch.float64)
    for it in range(60):
        ks = [float((it + i) % 3 + 1) for i in range(len(net.convs))]
        kb = float(it % 4 + 1)
        opt.zero_grad()
        ddp(x, z, ks, kb).backward()
        for i, c in enumerate(net.convs):
            if c.kernel_size == (3, 3):
                ref = (ks[i] * cnt).view(1, 1, 3, 3).expand(64, 64, 3, 3)
            else:
                ref = torch.full((128, 64, 1, 1), ks[i] * n * h * w, dtype=torch.float64)
            ref = ref.to(torch.bfloat16).to("cuda").double()
            bad += (c.weight.grad.double() - ref).abs().max()
        bad += (net.bn.bias.grad.double() - kb * n * h * w).abs().max()
        bad += (net.bn.weight.grad.double().abs().max() > 1e-3).double()
        opt.step()
        x.grad = None
    torch.cuda.synchronize()
    assert bad.item() == 0.0
    # the DDP side stream (high priority) carried the conv weight gradients
    assert any(key[1] for key in C._SIDE), C._SIDE
    assert len(ddp.bucket_layout()) >= 4


def test_ddp_bucket_timing(pg):
    """Per-bucket launch / join times from the reducer's HIP events: buckets are
    launched in order during backward, and the exposed tail is measured."""
    from apex_example_amd.parallel import DistributedDataParallel

    model = _Model()
    ddp = DistributedDataParallel(model, message_size=4096 * 64 * 4, force_collectives=True)
    ddp.enable_bucket_timing()
    x = torch.tensor(2.0, device="cuda")
    for _ in range(3):  # iteration 1 builds the layout (untimed)
        ddp(x).backward()
    t = ddp.bucket_timing()
    assert t is not None
    nb = len(ddp.bucket_layout())
    assert len(t["launch_ms"]) == nb == len(t["joined_ms"]) == len(t["bucket_numel"])
    assert t["backward_ms"] > 0.0            # the sleep skews are inside backward
    assert t["exposed_tail_ms"] >= 0.0
    assert all(b >= a - 1e-3 for a, b in zip(t["launch_ms"], t["launch_ms"][1:]))
    assert all(j >= t["backward_ms"] - 1e-3 for j in t["joined_ms"])


def test_ddp_resnet_amp_step(pg):
    """ResNet-18 amp O2 + apex DDP + FusedSGD on RCCL: grads are bucket views and
    the step is sync-free."""
    from apex_example_amd import amp
    from apex_example_amd.models import resnet18
    from apex_example_amd.optimizers import FusedSGD
    from apex_example_amd.parallel import DistributedDataParallel

    torch.manual_seed(0)
    m = resnet18(num_classes=10).cuda().to(memory_format=torch.channels_last)
    opt = FusedSGD(m.parameters(), lr=0.05, momentum=0.9, materialize_master_grads=False)
    m, opt = amp.initialize(m, opt, opt_level="O2", half_dtype=torch.bfloat16, verbosity=0)
    ddp = DistributedDataParallel(m, message_size=2_000_000, force_collectives=True)
    x = torch.randn(16, 3, 64, 64, device="cuda").to(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (16,), device="cuda")
    losses = []
    for _ in range(8):
        loss = torch.nn.functional.cross_entropy(ddp(x), y)
        opt.zero_grad()
        with amp.scale_loss(loss, opt) as s:
            s.backward()
        opt.step()
        losses.append(loss.item())
    assert all(getattr(p, "_amd_grad_is_bucket_view", False) for p in m.parameters())
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("syncbn", [False, True])
def test_two_ranks_one_gpu_gloo(tmp_path, syncbn):
    """bench.py's N>1 code path (apex DDP over a process group, bucket views, fused
    kernels, SyncBN by default) with two processes on the one test GPU."""
    res = W.run("gpu_ddp_resnet", 2, str(tmp_path), syncbn=syncbn)
    for a, b in zip(res[0]["params"], res[1]["params"]):
        assert torch.equal(a, b)
    assert res[0]["views"] and res[1]["views"]
    assert res[0]["losses"][-1] < res[0]["losses"][0]


@pytest.mark.parametrize("opt_level", ["O0", "O2"])
def test_two_ranks_match_concatenated_batch(tmp_path, opt_level):
    """With SyncBN the two ranks compute exactly the math of ONE process on the
    concatenated batch (global BN statistics, averaged gradients).  In fp32 (O0)
    the loss curve and the parameter updates must agree to rounding-order noise
    (measured: identical to 4 decimals over 6 steps on one box, tools/diag/ddp_parity.py;
    on another the 4th loss, 0.099, differed by 9e-4 - the fp32 convolutions are
    MIOpen's, whose algorithm choice varies by box - hence 2e-3 relative + 1e-3
    absolute).
    In bf16 (O2) the two runs round differently, and at 32x32 images the deepest BNs
    normalise over 8-16 values per channel: their gradients are so ill-conditioned that
    two single-process runs differing only in BN-statistics summation order already
    disagree by ~20 % (relative L2) in the first update and by up to 8 % in the step-2
    loss (tools/diag/ddp_stats_diff.py).  O2 therefore runs on 64x64 images (4x the BN
    population per channel), where the step-2 losses of DDP + SyncBN and of the
    concatenated-batch reference agree to 0.4-0.8 % (same tool, DDP_DIFF_HW=64): pinned
    at 0.5 % (step 1) and 2 % (step 2)."""
    steps = 4 if opt_level == "O0" else 2
    hw = 32 if opt_level == "O0" else 64
    res = W.run("gpu_ddp_resnet", 2, str(tmp_path), syncbn=True, lr=0.01,
                opt_level=opt_level, steps=steps, hw=hw)
    ref = W.gpu_resnet_reference(world=2, lr=0.01, opt_level=opt_level, steps=steps, hw=hw)
    # the rank losses are per-half means; the global loss is their average
    ddp_loss = [(a + b) / 2 for a, b in zip(res[0]["losses"], res[1]["losses"])]
    if opt_level != "O0":
        assert abs(ddp_loss[0] - ref["losses"][0]) <= 5e-3 * abs(ref["losses"][0]), (
            ddp_loss, ref["losses"])
    tol, atol = (2e-3, 1e-3) if opt_level == "O0" else (2e-2, 0.0)
    for a, b in zip(ddp_loss, ref["losses"]):
        assert abs(a - b) <= tol * abs(b) + atol, (ddp_loss, ref["losses"])
    if opt_level != "O0":
        return

    def worst_update_diff(ma, mb):
        worst = 0.0
        assert len(ma) == len(mb) == len(ref["params0"])
        for a, b, p0 in zip(ma, mb, ref["params0"]):
            # compare the UPDATES (param - init): the init itself cancels out
            da, db = a - p0, b - p0
            scale = db.abs().max().item()
            if scale > 0:
                worst = max(worst, (da - db).abs().max().item() / scale)
        return worst

    # one step: DDP's averaged gradient IS the concatenated batch's gradient, so the
    # first update agrees to summation-order noise in every tensor
    w1 = worst_update_diff(res[0]["masters1"], ref["masters1"])
    assert w1 < 1e-2, w1
    # after 4 steps of this memorisation task the per-tensor max-relative update
    # difference has been amplified by the dynamics (measured 0.3-9 % across boxes
    # whose MIOpen fp32 conv algorithms differ) - a sanity bound only
    w4 = worst_update_diff(res[0]["masters"], ref["masters"])
    assert w4 < 0.25, w4


def test_distributed_fused_adam_two_ranks_one_gpu(tmp_path):
    res = W.run("gpu_dfa", 2, str(tmp_path))
    for a, b in zip(res[0]["params"], res[1]["params"]):
        assert torch.equal(a, b)
    for r in res:
        assert r["skipped"]          # the injected overflow skipped the step on both ranks
        assert r["step"] == 4        # 5 steps, one skipped
    assert res[0]["losses"][-1] < res[0]["losses"][0]


def test_syncbn_gpu_two_ranks_matches_global_batch(tmp_path):
    """GPU SyncBN (bench.py's N>1 default) == BN + residual + ReLU over the global batch."""
    sizes = (4, 6)
    res = W.run("gpu_syncbn_step", 2, str(tmp_path), sizes=sizes)
    torch.manual_seed(0)
    C = 16
    full = torch.randn(sum(sizes), C, 6, 6) * 2 + 1
    zfull = torch.randn(sum(sizes), C, 6, 6)
    x = full.to(torch.bfloat16).float().requires_grad_(True)
    z = zfull.to(torch.bfloat16).float().requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.linspace(0.5, 1.5, C))
        bn.bias.copy_(torch.linspace(-1, 1, C))
    y = torch.relu(bn(x) + z)
    g = torch.Generator().manual_seed(99)
    dy = torch.randn(sum(sizes), C, 6, 6, generator=g)
    (y * dy).sum().backward()
    ys = torch.cat([r["y"] for r in res])

    def rel(a, b):  # max error relative to the tensor's scale
        return float((a - b).abs().max() / b.abs().max())
    # bf16 outputs (y, dx, dz; 2^-8 relative rounding): two ulps at the tensor's scale.
    # The inputs of the fp32 reference are the same bf16-rounded values, so only the
    # output rounding and the summation order differ.
    assert rel(ys, y.detach()) < 8e-3
    # (dx also carries dy's rounding to bf16 - the gradient of a bf16 output - through k1)
    assert rel(torch.cat([r["dx"] for r in res]), x.grad) < 1.2e-2
    assert rel(torch.cat([r["dz"] for r in res]), z.grad) < 8e-3
    # dgamma / dbeta are per-rank partial sums (DDP all-reduces them as gradients); fp32
    # sums of bf16-rounded dy
    assert rel(res[0]["dw"] + res[1]["dw"], bn.weight.grad) < 4e-3
    assert rel(res[0]["db"] + res[1]["db"], bn.bias.grad) < 4e-3
    for r in res:
        torch.testing.assert_close(r["rm"], bn.running_mean, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(r["rv"], bn.running_var, rtol=1e-4, atol=1e-5)
        assert r["nbt"] == 1
        # both ranks gathered through their slot of the shared destination (the raw
        # RCCL path's in-place layout; rank 1 writes at offset 2C + 1)
        assert r["slot_calls"] == 1


def test_bench_self_spawn_two_ranks_one_gpu():
    """`python bench.py --gpus 2` (no torchrun) starts two ranks itself; on the
    1-GPU box both share cuda:0 over gloo (RCCL refuses that).  The JSON must
    report n_gpus 2, SyncBN on, and the per-bucket DDP timing block."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, APEX_AMD_SINGLE_DEVICE="1", APEX_AMD_DIST_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2",
                        "--model", "resnet18", "--batch-size", "16", "--image-size", "64",
                        "--steps", "3", "--warmup", "2", "--full", "--bucket-timing-steps", "2",
                        "--opt-step-iters", "2"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["n_gpus"] == 2 and rec["launcher"] == "self-spawn"
    assert rec["config"]["parallelism"] == "dp2" and rec["config"]["syncbn"]
    assert rec["ddp"]["buckets"] >= 1 and rec["ddp"]["exposed_tail_ms"] >= 0
    # the N > 1 self-check: both replicas bitwise equal, groups span 2 ranks
    rep = rec["replicas"]
    assert rep["in_sync"] and rep["comm_sizes_ok"], rep
    assert {"params", "optimizer_params", "buffers"} <= set(rep["required"])
    assert rep["comms"]["syncbn"]["size"] == 2 and rep["comms"]["ddp"]["size"] == 2


def test_bench_two_ranks_desynced_replica_fails():
    """One rank's weight perturbed by one bit after the timed steps (test hook): the JSON
    records the mismatch and bench.py exits 5 instead of reporting a valid number."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, APEX_AMD_SINGLE_DEVICE="1", APEX_AMD_DIST_BACKEND="gloo",
               APEX_AMD_TEST_DESYNC_RANK="1")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2",
                        "--model", "resnet18", "--batch-size", "8", "--image-size", "32",
                        "--steps", "2", "--warmup", "1", "--full", "--bucket-timing-steps", "0",
                        "--opt-step-iters", "1"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 5, p.stdout[-2000:] + p.stderr[-4000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["replicas"]["in_sync"] is False
    assert rec["replicas"]["digests"]["params"]["match"] is False


@pytest.mark.timeout(280)
@pytest.mark.parametrize("model", ["bert_large", "gpt2_medium"])
def test_bench_transformers_two_ranks_one_gpu(model):
    """The transformer bench configs at world 2 (BASELINE: BERT-large O2 FusedLAMB and
    GPT-2-medium O1 FusedAdam on 8 GPUs): full-size models, short sequences, both ranks
    on cuda:0 over gloo - apex DDP with the direct dense weight-gradient path, the
    side-stream wgrad4w calls, the tied-embedding bucket and the fused optimizers at N > 1.
    The loss must be finite and the JSON must carry the DDP timing block."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, APEX_AMD_SINGLE_DEVICE="1", APEX_AMD_DIST_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    shape = ["--batch-size", "2", "--seq-len", "128"] if model == "bert_large" else \
        ["--batch-size", "1", "--seq-len", "256", "--allow-skipped-steps"]
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2",
                        "--model", model, "--steps", "2", "--warmup", "2", "--full",
                        "--bucket-timing-steps", "1", "--opt-step-iters", "1",
                        "--message-size", str(8 << 20)] + shape,
                       env=env, capture_output=True, text=True, timeout=260)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["n_gpus"] == 2 and rec["config"]["parallelism"] == "dp2"
    assert math.isfinite(rec["final_loss"]) and rec["ddp"]["buckets"] >= 1


@pytest.mark.parametrize("residual", [False, True])
def test_syncbn_forced_collectives_match_local_bn(pg, monkeypatch, residual):
    """SyncBN's RCCL path on one GPU (VERDICT r2 missing 2): ``force_collectives``
    sends the packed statistics through an all-gather and the packed gradient sums
    through an in-place all-reduce on the strided [2C] view, on a 1-rank RCCL
    communicator - from C++ (csrc/torch/reducer.cpp: through the process group, or
    straight on the compute stream with the dedicated SyncBN group's communicator).
    Both must really run, and the result must equal the local (no-collective) path to
    rounding."""
    from apex_example_amd import _native
    from apex_example_amd.parallel import SyncBatchNorm

    R = _native.require().reducer
    kinds = {"syncbn_allgather_combine": "all_gather", "syncbn_allgather_combine_raw":
             "all_gather", "syncbn_allreduce": "all_reduce", "syncbn_allreduce_raw": "all_reduce"}
    calls = {"all_gather": 0, "all_reduce": 0}
    for name, kind in kinds.items():
        orig = getattr(R, name)

        def wrapped(*a, _orig=orig, _kind=kind, **k):
            calls[_kind] += 1
            return _orig(*a, **k)
        monkeypatch.setattr(R, name, wrapped)

    torch.manual_seed(0)
    C = 64
    x = (torch.randn(8, C, 14, 14, device="cuda") * 2 + 1).to(torch.bfloat16)
    x = x.contiguous(memory_format=torch.channels_last)
    z = torch.randn_like(x) if residual else None
    dy = torch.randn_like(x)
    outs = []
    for forced in (False, True):
        bn = SyncBatchNorm(C, fuse_relu=True, force_collectives=forced).cuda()
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, C))
            bn.bias.copy_(torch.linspace(-1, 1, C))
        xi = x.clone().requires_grad_(True)
        zi = z.clone().requires_grad_(True) if residual else None
        before = dict(calls)
        y = bn(xi, zi)
        y.backward(dy)
        torch.cuda.synchronize()
        ran = {k: calls[k] - before[k] for k in calls}
        if forced:
            assert ran == {"all_gather": 1, "all_reduce": 1}, ran
        else:
            assert ran == {"all_gather": 0, "all_reduce": 0}, ran
        outs.append([y.float(), xi.grad.float(), zi.grad.float() if residual else None,
                     bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var,
                     bn.num_batches_tracked])
    names = ["y", "dx", "dz", "dw", "db", "running_mean", "running_var", "nbt"]
    for n, a, b in zip(names, outs[0], outs[1]):
        if a is None:
            continue
        if n == "nbt":
            assert int(a) == int(b) == 1
            continue
        # bf16 outputs: at most one bf16 ulp apart; fp32 statistics / dgamma / dbeta
        # differ only by the combine's summation order
        tol = dict(rtol=2 ** -7, atol=2 ** -7) if n in ("y", "dx", "dz") else \
            dict(rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(b, a, **tol, msg=n)


def test_ddp_side_stream_weight_grads_match_main_stream(pg):
    """under DDP the conv weight gradients run on the side stream,
    accumulate into their bucket views there and are announced to the reducer, whose
    bucket all-reduces (forced RCCL collectives at world 1) then wait on side-stream
    events.  Gradients and the trained weights must be bitwise equal to the
    main-stream path, iteration after iteration."""
    from apex_example_amd import amp
    from apex_example_amd.models import resnet18
    from apex_example_amd.ops import conv as convmod
    from apex_example_amd.optimizers import FusedSGD
    from apex_example_amd.parallel import DistributedDataParallel

    x = torch.randn(16, 3, 64, 64, device="cuda").to(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (16,), device="cuda")
    results = {}
    used = {}
    prev = convmod._DDP_SIDE
    try:
        for side in (False, True):
            convmod._DDP_SIDE = side
            torch.manual_seed(0)
            m = resnet18(num_classes=10, fused_bn=True, gemm_1x1=True).cuda().to(
                memory_format=torch.channels_last)
            opt = FusedSGD(m.parameters(), lr=0.05, momentum=0.9, materialize_master_grads=False)
            m, opt = amp.initialize(m, opt, opt_level="O2", half_dtype=torch.bfloat16,
                                    verbosity=0)
            ddp = DistributedDataParallel(m, message_size=500_000, force_collectives=True)
            calls = {"n": 0}
            orig = convmod._SideWgrad.run

            modes = []

            def counting(self, fn, *a, _orig=orig, _calls=calls, _modes=modes):
                if self.mode == "ddp":
                    _calls["n"] += 1
                p = self.params[0]
                slot = getattr(p, "_amd_ddp_slot", None)
                red = slot[0]() if slot else None
                _modes.append((self.mode, slot is not None, red is not None and
                               red.async_ready_ok(), p.grad is None))
                return _orig(self, fn, *a)
            convmod._SideWgrad.run = counting
            grads = []
            try:
                for it in range(4):
                    loss = torch.nn.functional.cross_entropy(ddp(x), y)
                    opt.zero_grad()
                    with amp.scale_loss(loss, opt) as s:
                        s.backward()
                    grads.append([p.grad.detach().clone() for p in m.parameters()])
                    opt.step()
            finally:
                convmod._SideWgrad.run = orig
            torch.cuda.synchronize()
            results[side] = (grads, [p.detach().clone() for p in m.parameters()])
            used[side] = (calls["n"], sorted(set(modes), key=str))
    finally:
        convmod._DDP_SIDE = prev
    assert used[False][0] == 0 and used[True][0] > 0, used
    for it, (a, b) in enumerate(zip(results[False][0], results[True][0])):
        bad = [i for i, (u, v) in enumerate(zip(a, b)) if not torch.equal(u, v)]
        assert not bad, (it, bad)
    for u, v in zip(results[False][1], results[True][1]):
        assert torch.equal(u, v)


def test_ddp_direct_bucket_gradients_match_autograd_path(pg, monkeypatch):
    """Own-kernel weight gradients and SyncBN dgamma / dbeta accumulate straight into the
    DDP bucket views (ops/_ddp_direct.py) instead of autograd's add kernels: the
    iteration-2+ gradients must match the autograd path to one bf16 rounding (the
    direct path rounds the sum once) and the direct path must actually run."""
    from apex_example_amd import amp
    from apex_example_amd.models import resnet18
    from apex_example_amd.ops import _ddp_direct
    from apex_example_amd.optimizers import FusedSGD
    from apex_example_amd.parallel import (DistributedDataParallel, convert_syncbn_model,
                                           set_syncbn_force_collectives)

    x = torch.randn(16, 3, 64, 64, device="cuda").to(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (16,), device="cuda")
    grads, marks = {}, {}
    orig = _ddp_direct.mark_ready
    for on in (False, True):
        monkeypatch.setattr(_ddp_direct, "_ON", on)
        count = {"n": 0}

        def counting(sl, _c=count):
            _c["n"] += len(sl)
            return orig(sl)
        monkeypatch.setattr(_ddp_direct, "mark_ready", counting)
        torch.manual_seed(0)
        m = convert_syncbn_model(resnet18(num_classes=10, fused_bn=True, gemm_1x1=True))
        m = m.cuda().to(memory_format=torch.channels_last)
        set_syncbn_force_collectives(m, True)
        opt = FusedSGD(m.parameters(), lr=0.05, momentum=0.9, materialize_master_grads=False)
        m, opt = amp.initialize(m, opt, opt_level="O2", half_dtype=torch.bfloat16, verbosity=0)
        ddp = DistributedDataParallel(m, message_size=500_000, force_collectives=True)
        gs = []
        for it in range(3):
            loss = torch.nn.functional.cross_entropy(ddp(x).float(), y)
            opt.zero_grad()
            with amp.scale_loss(loss, opt) as s:
                s.backward()
            gs.append([p.grad.detach().float().clone() for p in m.parameters()])
            opt.step()
        torch.cuda.synchronize()
        grads[on], marks[on] = gs, count["n"]
    assert marks[False] == 0
    # from iteration 2 on every conv weight and BN affine pair goes direct
    n_conv = sum(1 for p in m.parameters() if p.dim() == 4)
    assert marks[True] >= 2 * n_conv, marks
    for it in range(3):
        for a, b in zip(grads[False][it], grads[True][it]):
            scale = float(a.abs().max()) + 1e-30
            assert float((a - b).abs().max()) / scale < 2e-2, it


@pytest.mark.parametrize("ddp_side", [False, True])
@pytest.mark.parametrize("opt_level", ["O1", "O2"])
def test_ddp_direct_dense_weight_gradients_match_autograd_path(pg, monkeypatch, opt_level,
                                                               ddp_side):
    """fused_dense weight gradients accumulate straight into the DDP bucket views
    (split-K slab reduction / GEMM beta = 1) instead of autograd's add kernel per weight:
    GPT-2 O1 (fp32 weights, fp16 GEMMs) and O2 (bf16 weights) must match the autograd
    path and the direct path must run for every dense weight from iteration 2 on.  With
    the DDP side stream on (the default), O1's fp32 dense weight gradients run on the
    side stream and reach their bucket views from there instead: gradients must match."""
    from apex_example_amd import amp
    from apex_example_amd.models.gpt2 import GPT2Config, GPT2LMHeadModel, lm_loss
    from apex_example_amd.ops import _ddp_direct, conv as conv_ops

    monkeypatch.setattr(conv_ops, "_DDP_SIDE", ddp_side)
    from apex_example_amd.optimizers import FusedAdam
    from apex_example_amd.parallel import DistributedDataParallel

    half = torch.float16 if opt_level == "O1" else torch.bfloat16
    cfg = dict(vocab_size=512, n_positions=256, n_embd=256, n_layer=2, n_head=4,
               resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0)
    ids = torch.randint(0, 512, (8, 256), device="cuda",
                        generator=torch.Generator("cuda").manual_seed(3))
    grads, marks = {}, {}
    orig = _ddp_direct.mark_ready
    for on in (False, True):
        monkeypatch.setattr(_ddp_direct, "_ON", on)
        count = {"n": 0}

        def counting(sl, _c=count):
            _c["n"] += len(sl)
            return orig(sl)
        monkeypatch.setattr(_ddp_direct, "mark_ready", counting)
        torch.manual_seed(0)
        m = GPT2LMHeadModel(GPT2Config(**cfg)).cuda()
        opt = FusedAdam(m.parameters(), lr=1e-4, materialize_master_grads=False)
        m, opt = amp.initialize(m, opt, opt_level=opt_level, half_dtype=half, verbosity=0)
        ddp = DistributedDataParallel(m, message_size=200_000, force_collectives=True)
        gs = []
        for it in range(3):
            loss = lm_loss(ddp(ids), ids)
            opt.zero_grad()
            with amp.scale_loss(loss, opt) as s:
                s.backward()
            gs.append([p.grad.detach().float().clone() for p in m.parameters()])
            opt.step()
        torch.cuda.synchronize()
        grads[on], marks[on] = gs, count["n"]
    assert marks[False] == 0
    n_dense = 4 * cfg["n_layer"]  # qkv, attention out, FFN in, FFN out
    if not (ddp_side and opt_level == "O1"):
        assert marks[True] >= 2 * n_dense, marks
    tol = 1e-3 if opt_level == "O1" else 2e-2
    for it in range(3):
        for a, b in zip(grads[False][it], grads[True][it]):
            if not torch.isfinite(a).all():  # an overflow step: both must see it
                assert not torch.isfinite(b).all()
                continue
            scale = float(a.abs().max()) + 1e-30
            assert float((a - b).abs().max()) / scale < tol, it


class _SharedNet(torch.nn.Module):
    """A 3x3 conv called twice per forward and a FusedDense head tied to an Embedding
    (parameters with more than one use per iteration)."""

    def __init__(self):
        super().__init__()
        from apex_example_amd.fused_dense import FusedDense
        from apex_example_amd.ops.conv import Conv2d3x3
        from apex_example_amd.ops.embedding import Embedding

        self.conv = Conv2d3x3(64, 64)
        self.other = Conv2d3x3(64, 64)          # used once: goes direct
        self.emb = Embedding(96, 64)
        self.head = FusedDense(64, 96, bias=False)
        self.head.weight = self.emb.weight      # tied

    def forward(self, x, ids):
        h = self.conv(torch.relu(self.conv(x)))  # same weight, two uses
        h = self.other(h)
        v = h.mean((2, 3)) + self.emb(ids)       # [B, 64]
        return self.head(v).float()


def test_ddp_direct_path_shared_parameters_gpu(pg, monkeypatch):
    """Own-kernel ops whose parameter is used twice (same conv module called twice) or
    tied (FusedDense head = Embedding table) under DDP with forced RCCL collectives: no
    'received a gradient twice' error, gradients equal to the autograd path (direct off),
    the tied weight excluded from the direct path and the once-used conv still direct."""
    from apex_example_amd.ops import _ddp_direct, conv as conv_ops
    from apex_example_amd.parallel import DistributedDataParallel

    # the direct path on the compute stream (the DDP side stream would take the conv's
    # weight gradient instead)
    monkeypatch.setattr(conv_ops, "_DDP_SIDE", False)
    x = torch.randn(8, 64, 16, 16, device="cuda").to(torch.bfloat16).to(
        memory_format=torch.channels_last)
    ids = torch.randint(0, 96, (8,), device="cuda")
    grads, marks = {}, {}
    orig = _ddp_direct.mark_ready
    for on in (False, True):
        monkeypatch.setattr(_ddp_direct, "_ON", on)
        count = {"n": 0}

        def counting(sl, _c=count):
            _c["n"] += len(sl)
            return orig(sl)
        monkeypatch.setattr(_ddp_direct, "mark_ready", counting)
        torch.manual_seed(0)
        m = _SharedNet().cuda().to(torch.bfloat16).to(memory_format=torch.channels_last)
        ddp = DistributedDataParallel(m, message_size=20_000, force_collectives=True)
        gs = []
        for it in range(3):
            for p in m.parameters():
                if p.grad is not None:
                    p.grad.zero_()
            (ddp(x, ids) ** 2).mean().backward()
            gs.append([p.grad.detach().float().clone() for p in m.parameters()])
        torch.cuda.synchronize()
        grads[on], marks[on] = gs, count["n"]
        if on:
            idx = {id(p): i for i, p in enumerate(ddp.active_params)}
            assert not ddp.reducer.direct_ok(idx[id(m.emb.weight)])
    assert marks[False] == 0 and marks[True] >= 2, marks  # `other` went direct (its. 2, 3)
    for it in range(3):
        for a, b in zip(grads[False][it], grads[True][it]):
            scale = float(a.abs().max()) + 1e-30
            assert float((a - b).abs().max()) / scale < 2e-2, it


def test_ddp_side_stream_weight_grad_plus_functional_penalty(pg, monkeypatch):
    """A conv weight whose gradient the DDP side stream writes into its (lazily zeroed)
    bucket view AND that an explicit penalty term uses through plain autograd
    (ADVICE r5): AccumulateGrad adds the penalty gradient into the same view on the
    compute stream, so it must wait for the side stream's write (the reducer's
    AccumulateGrad pre-hook).  The side stream sleeps before every weight gradient, so
    a missing wait loses the penalty (the side kernel overwrites the lazily zeroed
    view after the add).  Gradients have a closed form: k * tap count + lambda."""
    from apex_example_amd.ops import conv as C
    from apex_example_amd.optimizers import FusedSGD
    from apex_example_amd.parallel import DistributedDataParallel

    monkeypatch.setattr(C, "_TEST_SIDE_SLEEP", 2_000_000)
    torch.manual_seed(0)
    net = _ConvNet()
    ddp = DistributedDataParallel(net, message_size=64 * 64 * 9 * 2, force_collectives=True)
    opt = FusedSGD(net.parameters(), lr=0.0)
    n, h, w = 2, 8, 8
    x = torch.ones(n, 64, h, w, device="cuda", dtype=torch.bfloat16).to(
        memory_format=torch.channels_last)
    z = torch.ones(n, 64, h, w, device="cuda")
    z[:, :, :, w // 2:] = -1.0
    z = z.to(memory_format=torch.channels_last)
    cnt = torch.zeros(3, 3, dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            cnt[r, s] = n * (h - abs(r - 1)) * (w - abs(s - 1))
    lam = 4.0
    sides = {"n": 0}
    orig = C._SideWgrad.run

    def counting(self, fn, *a, _orig=orig):
        if self.mode == "ddp":
            sides["n"] += 1
        return _orig(self, fn, *a)
    monkeypatch.setattr(C._SideWgrad, "run", counting)
    bad = torch.zeros((), device="cuda", dtype=torch.float64)
    for it in range(8):
        ks = [float((it + i) % 3 + 1) for i in range(len(net.convs))]
        opt.zero_grad()
        loss = ddp(x, z, ks, 1.0)
        # the penalty: a second, plain-autograd use of conv 0's weight
        loss = loss + lam * net.convs[0].weight.float().sum()
        loss.backward()
        for i, c in enumerate(net.convs):
            if c.kernel_size == (3, 3):
                ref = (ks[i] * cnt).view(1, 1, 3, 3).expand(64, 64, 3, 3)
            else:
                ref = torch.full((128, 64, 1, 1), ks[i] * n * h * w, dtype=torch.float64)
            if i == 0:
                ref = ref + lam
            ref = ref.to(torch.bfloat16).to("cuda").double()
            bad += (c.weight.grad.double() - ref).abs().max()
        opt.step()
    torch.cuda.synchronize()
    assert sides["n"] > 0
    assert bad.item() == 0.0
