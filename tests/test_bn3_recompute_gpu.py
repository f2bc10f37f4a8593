"""conv3 recomputed inside bn3's passes (ops/conv.py forward_bn3, ops/batch_norm.py ConvRec,
csrc/hip/conv_igemm.hip conv_tap_k EPI 2 / 3 / 4): an identity bottleneck's conv3 with at
most 128 input channels launches statistics-only and then writes x3, bn3's y and the ReLU
mask from one kernel (bn3's forward takes them, no apply pass), and bn3's elementwise
backward recomputes x3 instead of reading it.

Every tensor must be BITWISE what the separate passes give (torch.equal, module flag on vs
off on identical inputs): y, x3, the statistics slab, the running statistics, and the
gradients of out2, z, W3, gamma and beta.  The consumer of y is a 1x1 conv with the
BN-backward epilogue (as conv1 of the next block), so bn3's backward gets g and its sums the
way it does in the model.

Shapes: 64 -> 256 (one K-tile, the ring-free kernel) and 128 -> 512 (two K-tiles, the
ring), with M = 128 (one full tile), 147 (a ragged tile) and 320 (several tiles).
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
CL = torch.channels_last

PAIRS = [(64, 256), (128, 512)]
ROWS = [(2, 8, 8), (3, 7, 7), (5, 8, 8)]   # M = 128, 147, 320


def _bf(t):
    return t.to(torch.bfloat16).contiguous(memory_format=CL)


def _force(monkeypatch, on):
    """The module flag, with both shapes routed to both kernels whatever the measured
    per-shape tables say (the kernels are tested even where the model does not use them)."""
    from apex_example_amd.ops import conv as convmod

    monkeypatch.setattr(convmod, "_BN3_RECOMPUTE", on)
    monkeypatch.setattr(convmod, "_REC_FWD", set(PAIRS))
    monkeypatch.setattr(convmod, "_REC_BWD", set(PAIRS))


def _tail_modules(ci, co):
    """conv3 + bn3 of a block and the next block's conv1, as models/resnet.py links them."""
    from apex_example_amd.models.resnet import _BNAct, _link_stats
    from apex_example_amd.ops.conv import Conv2d1x1

    torch.manual_seed(1)
    conv3 = Conv2d1x1(ci, co).to(dev).to(torch.bfloat16).to(memory_format=CL)
    bn3 = _BNAct(co, True, True).to(dev)
    conv1 = Conv2d1x1(co, ci).to(dev).to(torch.bfloat16).to(memory_format=CL)
    with torch.no_grad():
        bn3.bn.weight.uniform_(0.5, 1.5)
        bn3.bn.bias.uniform_(-0.3, 0.3)
        bn3.bn.running_mean.normal_(0, 0.1)
        bn3.bn.running_var.uniform_(0.5, 1.5)
    _link_stats(conv3, bn3)
    return conv3, bn3, conv1


def _inputs(ci, co, n, h, w):
    torch.manual_seed(2)
    out2 = _bf(torch.relu(torch.randn(n, ci, h, w, device=dev)))
    z = _bf(torch.randn(n, co, h, w, device=dev) * 1.5)
    r1 = torch.randn(n, ci, h, w, device=dev)
    r2 = torch.randn(n, co, h, w, device=dev)
    return out2, z, r1, r2


def _run_tail(mods, inp):
    """Forward + backward of conv3 -> bn3(+z, ReLU) -> conv1 (with the skip branch);
    everything the issue lists, as a dict of tensors."""
    from apex_example_amd.ops import batch_norm as bnmod
    from apex_example_amd.ops.conv import join_side_streams

    conv3, bn3, conv1 = copy.deepcopy(mods)
    from apex_example_amd.models.resnet import _link_stats
    _link_stats(conv3, bn3)          # (the weak reference does not survive the copy)
    out2, z, r1, r2 = inp
    out2 = out2.clone().requires_grad_(True)
    z = z.clone().requires_grad_(True)
    counts = [bnmod.FUSED_BWD_CALLS[0], bnmod.REC_FWD_CALLS[0], bnmod.REC_BWD_CALLS[0]]
    x3 = conv3.forward_bn3(out2, z)
    slab = x3._amd_bn_stats[0]
    y = bn3(x3, z)
    o, skip = conv1.forward_with_skip(y)
    ((o.float() * r1).sum() + (skip.float() * r2).sum()).backward()
    join_side_streams()
    torch.cuda.synchronize()
    counts = [bnmod.FUSED_BWD_CALLS[0] - counts[0], bnmod.REC_FWD_CALLS[0] - counts[1],
              bnmod.REC_BWD_CALLS[0] - counts[2]]
    res = {"y": y.detach(), "x3": x3.detach(), "slab": slab, "o": o.detach(),
           "running_mean": bn3.bn.running_mean, "running_var": bn3.bn.running_var,
           "nbt": bn3.bn.num_batches_tracked, "d_out2": out2.grad, "d_z": z.grad,
           "d_w3": conv3.weight.grad, "d_gamma": bn3.bn.weight.grad,
           "d_beta": bn3.bn.bias.grad, "d_w1": conv1.weight.grad}
    return res, counts


def _assert_same(new, old):
    for k in old:
        assert new[k] is not None and old[k] is not None, k
        assert new[k].shape == old[k].shape and new[k].dtype == old[k].dtype, k
        assert torch.equal(new[k], old[k]), "%s differs: max |d| = %g" % (
            k, float((new[k].double() - old[k].double()).abs().max()))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("pair", PAIRS)
def test_recompute_is_bitwise_the_separate_passes(pair, rows, monkeypatch):
    ci, co = pair
    mods = _tail_modules(ci, co)
    inp = _inputs(ci, co, *rows)
    _force(monkeypatch, False)
    old, c_old = _run_tail(mods, inp)
    _force(monkeypatch, True)
    new, c_new = _run_tail(mods, inp)
    # both paths took the consumer's epilogue sums; only the new one recomputed
    assert c_old == [1, 0, 0] and c_new == [1, 1, 1], (c_old, c_new)
    frac = float((old["y"] > 0).float().mean())
    assert 0.2 < frac < 0.8, frac              # both signs under the ReLU
    assert int(old["nbt"]) == 1
    _assert_same(new, old)


def test_ring_kernel_shape(monkeypatch):
    """128 -> 512 over >= 1024 workgroups takes the 32-deep ring kernel (the model's 28x28
    launch); the small cases above run the 64-deep one.  M = 32,928: a ragged last tile."""
    ci, co = PAIRS[1]
    mods = _tail_modules(ci, co)
    inp = _inputs(ci, co, 42, 28, 28)
    _force(monkeypatch, False)
    old, _ = _run_tail(mods, inp)
    _force(monkeypatch, True)
    new, c_new = _run_tail(mods, inp)
    assert c_new == [1, 1, 1], c_new
    _assert_same(new, old)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_each_form_alone(which, monkeypatch):
    """The per-shape tables route the forward and the backward form independently."""
    from apex_example_amd.ops import conv as convmod

    ci, co = PAIRS[0]
    mods = _tail_modules(ci, co)
    inp = _inputs(ci, co, *ROWS[1])
    _force(monkeypatch, False)
    old, _ = _run_tail(mods, inp)
    _force(monkeypatch, True)
    monkeypatch.setattr(convmod, "_REC_BWD" if which == "fwd" else "_REC_FWD", set())
    new, c_new = _run_tail(mods, inp)
    assert c_new == ([1, 1, 0] if which == "fwd" else [1, 0, 1]), c_new
    _assert_same(new, old)


def _chain(ci):
    from apex_example_amd.models.resnet import Bottleneck

    torch.manual_seed(3)
    net = torch.nn.Sequential(
        Bottleneck(4 * ci, ci, fused_bn=True, gemm_1x1=True),
        Bottleneck(4 * ci, ci, fused_bn=True, gemm_1x1=True)).to(dev)
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.to(torch.bfloat16)
    return net.to(memory_format=CL)


def _run_chain(net0, x0, r):
    from apex_example_amd.ops import batch_norm as bnmod
    from apex_example_amd.ops.conv import join_side_streams

    net = copy.deepcopy(net0)
    for blk in net:   # (weak references do not survive the copy)
        from apex_example_amd.models.resnet import _link_stats
        for c, b in ((blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)):
            _link_stats(c, b)
    x = x0.clone().requires_grad_(True)
    counts = [bnmod.FUSED_BWD_CALLS[0], bnmod.REC_FWD_CALLS[0], bnmod.REC_BWD_CALLS[0]]
    y = net(x)
    (y.float() * r).sum().backward()
    join_side_streams()
    torch.cuda.synchronize()
    counts = [bnmod.FUSED_BWD_CALLS[0] - counts[0], bnmod.REC_FWD_CALLS[0] - counts[1],
              bnmod.REC_BWD_CALLS[0] - counts[2]]
    res = {"y": y.detach(), "dx": x.grad}
    for k, p in net.named_parameters():
        res["grad:" + k] = p.grad
    for k, b in net.named_buffers():
        res["buf:" + k] = b
    return res, counts


@pytest.mark.parametrize("ci", [64, 128])
def test_two_block_chain_bitwise(ci, monkeypatch):
    """Two identity bottlenecks: the second block's conv1 dgrad epilogue hands the first
    block's bn3 its g and sums, as in the model."""
    net = _chain(ci)
    torch.manual_seed(4)
    x0 = _bf(torch.relu(torch.randn(3, 4 * ci, 7, 7, device=dev)))
    r = torch.randn(3, 4 * ci, 7, 7, device=dev)
    _force(monkeypatch, False)
    old, c_old = _run_chain(net, x0, r)
    _force(monkeypatch, True)
    new, c_new = _run_chain(net, x0, r)
    assert c_old[0] == c_new[0] and c_old[0] >= 5, (c_old, c_new)   # same fused backwards
    assert c_old[1:] == [0, 0]
    # both bn3s recompute forward; only the first block's bn3 has a consumer epilogue
    assert c_new[1:] == [2, 1], c_new
    _assert_same(new, old)


def test_bn3_hooks_see_the_real_input(monkeypatch):
    """A forward pre-hook on bn3 sees the complete x3 and the running statistics from
    before the update (the fused kernel runs inside the conv call, its finalize without
    side effects)."""
    ci, co = PAIRS[0]
    conv3, bn3, _ = _tail_modules(ci, co)
    out2, z, _, _ = _inputs(ci, co, *ROWS[1])
    rm0 = bn3.bn.running_mean.clone()
    seen = {}

    def pre(mod, args):
        seen["x"] = args[0].detach().clone()
        seen["rm"] = mod.running_mean.clone()
    h = bn3.bn.register_forward_pre_hook(pre)
    _force(monkeypatch, True)
    with torch.no_grad():
        x3 = conv3.forward_bn3(out2, z)
        bn3(x3, z)
    h.remove()
    with torch.no_grad():
        assert torch.equal(seen["x"], conv3(out2))      # the plain conv launch
    assert torch.equal(seen["x"], x3) and torch.equal(seen["rm"], rm0)
    assert not torch.equal(bn3.bn.running_mean, rm0)


def test_state_dict_keys_unchanged(monkeypatch):
    from apex_example_amd.models import resnet50

    keys = list(resnet50(fused_bn=True, gemm_1x1=True).state_dict().keys())
    assert len(keys) == 320 and "layer1.1.bn3.bn.running_var" in keys, len(keys)


def test_fallback_off_the_epilogue_branch(monkeypatch):
    """autograd.grad on part of the graph: bn3's gradient does not come from a consumer's
    epilogue, so the backward runs today's kernels on the stored x3 - same result as the
    old path, and weight.grad stays what it was.  (.grad is set beforehand: with .grad None
    the side-stream weight gradient stores .grad itself on either path, whatever inputs
    autograd.grad names.)"""
    from apex_example_amd.ops import batch_norm as bnmod

    ci, co = PAIRS[0]
    conv3, bn3, _ = _tail_modules(ci, co)
    out2, z, _, _ = _inputs(ci, co, *ROWS[1])
    torch.manual_seed(5)
    g0 = torch.randn_like(conv3.weight)
    got = {}
    for on in (False, True):
        _force(monkeypatch, on)
        c3, b3 = copy.deepcopy(conv3), copy.deepcopy(bn3)
        from apex_example_amd.models.resnet import _link_stats
        _link_stats(c3, b3)
        c3.weight.grad = g0.clone()
        a = out2.clone().requires_grad_(True)
        n0 = bnmod.REC_BWD_CALLS[0]
        y = b3(c3.forward_bn3(a, z), z)
        (da,) = torch.autograd.grad(y.float().sum(), a)
        torch.cuda.synchronize()
        assert bnmod.REC_BWD_CALLS[0] == n0
        assert torch.equal(c3.weight.grad, g0)
        assert b3.bn.weight.grad is None
        got[on] = (y.detach(), da)
    assert torch.equal(got[True][0], got[False][0])
    assert torch.equal(got[True][1], got[False][1])


def test_ineligible_inputs_keep_the_old_path(monkeypatch):
    """Eval mode and a wide conv3 do not defer (x3 is written by the conv itself)."""
    from apex_example_amd.ops import batch_norm as bnmod
    from apex_example_amd.ops import conv as convmod

    _force(monkeypatch, True)
    wide = _tail_modules(256, 1024)
    assert convmod._recompute_plan(wide[0], *_inputs(256, 1024, *ROWS[0])[:2])[0] is None
    conv3, bn3, _ = _tail_modules(64, 256)
    out2, z, _, _ = _inputs(64, 256, *ROWS[0])
    n0 = bnmod.REC_FWD_CALLS[0]
    bn3.eval()
    x3 = conv3.forward_bn3(out2, z)
    assert not hasattr(x3, "_amd_bn_rec")
    y = bn3(x3, z)
    assert bnmod.REC_FWD_CALLS[0] == n0
    ref = torch.relu(F.batch_norm(x3.float(), bn3.bn.running_mean, bn3.bn.running_var,
                                  bn3.bn.weight, bn3.bn.bias, False, 0.0, bn3.bn.eps)
                     + z.float())
    assert float((y.detach().float() - ref).abs().max()) < 5e-2


def test_against_fp32_reference(monkeypatch):
    """Sanity: the fused path against fp32 F.conv2d + F.batch_norm + add + ReLU, with the
    tolerances of tests/test_conv_bn_bwd_gpu.py."""
    _force(monkeypatch, True)
    ci, co = PAIRS[1]
    mods = _tail_modules(ci, co)
    inp = _inputs(ci, co, *ROWS[2])
    new, counts = _run_tail(mods, inp)
    assert counts == [1, 1, 1]
    conv3, bn3, conv1 = mods
    out2, z, r1, r2 = inp
    a = out2.float().requires_grad_(True)
    zz = z.float().requires_grad_(True)
    w3 = conv3.weight.detach().float().requires_grad_(True)
    gam = bn3.bn.weight.detach().clone().requires_grad_(True)
    bet = bn3.bn.bias.detach().clone().requires_grad_(True)
    w1 = conv1.weight.detach().float()
    x3 = F.conv2d(a, w3)
    # the BN reads x3 as stored (bf16), straight-through for the gradient: with the fp32
    # x3 a few pre-activations per row change sign against the bf16 chain, each a full-size
    # gradient element, which is no property of the kernels under test (that test's chain
    # feeds both sides the same bf16 BN input too)
    x3q = x3 + (x3.detach().to(torch.bfloat16).float() - x3.detach())
    y = torch.relu(F.batch_norm(x3q, None, None, gam, bet, True, 0.0, bn3.bn.eps) + zz)
    o = F.conv2d(y, w1)
    ((o * r1).sum() + (y * r2).sum()).backward()
    x3, y = x3.detach(), y.detach()
    errs = {"y": float((new["y"].float() - y).abs().max() / y.abs().max()),
            "x3": float((new["x3"].float() - x3).abs().max() / x3.abs().max())}
    for k, want in (("d_out2", a.grad), ("d_z", zz.grad), ("d_w3", w3.grad),
                    ("d_gamma", gam.grad), ("d_beta", bet.grad)):
        errs[k] = float((new[k].float() - want).abs().max() / want.abs().max())
    print("relative errors against fp32:", errs)
    assert errs["y"] < 2e-2 and errs["x3"] < 2e-2, errs
    for k in ("d_out2", "d_z", "d_w3", "d_gamma", "d_beta"):
        assert errs[k] < 3e-2, (k, errs)
