"""Boolean [Sq, Sk] attention masks in the fused attention kernels (the AMASK instantiations
of csrc/hip/attention.hip and attention_d128.hip, bit tiles from attention_pairmask.hip)
against an fp32 torch reference: dead, mixed and full tiles, ragged lengths, cross shapes,
per-batch masks merged with a key-padding mask, fully masked rows and keys, dropout with
the exact keep mask, the prepared tile classes, validation and the contrib modules."""
import math

import pytest
import torch

import dropout_hash
from attn_ref import DEV, NEG, close, finite, no_sdpa

pytestmark = pytest.mark.gpu

BOUND = {torch.bfloat16: 2e-2, torch.float16: 6e-3}
PATTERNS = ["tril", "band", "blockdiag", "bernoulli", "holes"]


def make_mask(pattern, Sq, Sk):
    """bool [Sq, Sk] on the GPU, True = masked pair."""
    i, j = torch.arange(Sq).view(Sq, 1), torch.arange(Sk).view(1, Sk)
    if pattern == "tril":         # dead, mixed and full tiles in one mask
        m = j > i
    elif pattern == "band":       # dead tiles on both sides of the live ones
        m = (i - j).abs() > 40
    elif pattern == "blockdiag":  # documents [0, 50), [50, 130), [130, ..): no tile-aligned edge
        seg = lambda t: (t >= 50).int() + (t >= 130).int()  # noqa: E731
        m = seg(i) != seg(j)
    elif pattern == "bernoulli":  # every tile mixed
        m = torch.rand(Sq, Sk, generator=torch.Generator().manual_seed(4321)) < 0.5
    elif pattern == "holes":      # a dead tile amid full ones, a dead query row, a dead key
        m = ((i >= 64) & (i < 192) & (j >= 64) & (j < 128)) | (i == 195) | (j == 9)
    else:
        raise AssertionError(pattern)
    return m.to(DEV)


def ref_attention(q, k, v, mask, p=0.0, seed=0):
    """fp32 reference: mask bool [Sq, Sk] or [B, Sq, Sk], True = masked -> (o [B, Sq, H, D],
    lse [B, H, Sq] log2, dead [B, H, Sq]); fully masked rows give o = 0 and zero gradients."""
    B, Sq, H, D = q.shape
    qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))
    s = (qf @ kf.transpose(-1, -2) / math.sqrt(D)).masked_fill(mask.view(-1, 1, Sq, k.size(1)), NEG)
    dead = (s == NEG).all(-1, keepdim=True)
    lse = torch.logsumexp(s, -1) / math.log(2.0)
    pr = torch.softmax(torch.where(dead, torch.zeros_like(s), s), -1)
    pr = torch.where(dead, torch.zeros_like(pr), pr)
    if p > 0:
        t = dropout_hash.thr8(p)
        keep = dropout_hash.hash_bytes(B, H, Sq, seed, SK=k.size(1), device=q.device) >= t
        pr = pr * keep * (256.0 / (256 - t))
    return (pr @ vf).permute(0, 2, 1, 3), lse, dead.squeeze(-1)


def ref_all(q, k, v, do, mask, p=0.0, seed=0):
    qf, kf, vf = (t.detach().float().clone().requires_grad_(True) for t in (q, k, v))
    o, lse, dead = ref_attention(qf, kf, vf, mask, p, seed)
    o.backward(do.float())
    return o.detach(), lse.detach(), dead, qf.grad, kf.grad, vf.grad


def rand_qkv(B, Sq, Sk, H, D, dt):
    torch.manual_seed(0)
    q = torch.randn(B, Sq, H, D, device=DEV, dtype=dt)
    kv = torch.randn(B, Sk, 2, H, D, device=DEV, dtype=dt)
    return q, kv, torch.randn(B, Sq, H, D, device=DEV, dtype=dt)


def check(q, kv, do, mask, bound, kpm=None):
    """fused_attention_kv under (mask, kpm) against the reference: o, lse, dq, dk, dv."""
    from apex_example_amd.ops import attention as A

    full = mask if kpm is None else mask | kpm.view(kpm.size(0), 1, -1)
    ro, rlse, dead, rdq, rdk, rdv = ref_all(q, kv[:, :, 0], kv[:, :, 1], do, full)
    qa, kva = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    o = A.fused_attention_kv(qa, kva, attn_mask=mask, key_padding_mask=kpm)
    o.backward(do)
    pm = A.prepare_attn_mask(mask, kpm)
    _, lse = A._C().fwd_amask(q, kv[:, :, 0], kv[:, :, 1], 0.0, 0, 1.0 / math.sqrt(q.size(-1)),
                              pm.wq, pm.cq, pm.wk, pm.ck)
    finite(o, qa.grad, kva.grad)
    close(o, ro, bound, "o")
    close(qa.grad, rdq, bound, "dq")
    close(kva.grad[:, :, 0], rdk, bound, "dk")
    close(kva.grad[:, :, 1], rdv, bound, "dv")
    assert (lse[~dead] - rlse[~dead]).abs().max().item() < 1e-3
    assert (lse[dead] == NEG).all()
    return o, qa.grad, kva.grad, full


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("pattern,dt", [(p, torch.bfloat16) for p in PATTERNS] +
                         [("band", torch.float16)])
def test_fwd_bwd_patterns(pattern, dt, D):
    S = 200  # two query tiles, four key tiles, ragged both ways
    check(*rand_qkv(2, S, S, 2, D, dt), make_mask(pattern, S, S), BOUND[dt])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,Sk", [(70, 200), (200, 70)])
def test_cross_shapes(Sq, Sk, D):
    check(*rand_qkv(2, Sq, Sk, 2, D, torch.bfloat16), make_mask("band", Sq, Sk), 2e-2)


@pytest.mark.parametrize("D", [64, 128])
def test_per_batch_mask_with_key_padding(D):
    B, S = 3, 200
    mask = torch.stack([make_mask(p, S, S) for p in ("tril", "band", "blockdiag")])
    kpm = torch.zeros(B, S, dtype=torch.bool, device=DEV)
    kpm[1, 150:] = True  # padded from key 150
    kpm[2] = True        # every key masked
    o, dq, dkv, full = check(*rand_qkv(B, S, S, 2, D, torch.bfloat16), mask, 2e-2, kpm)
    assert (o[2] == 0).all() and (dq[2] == 0).all()
    dead_key = full.all(1)  # [B, Sk]: nobody attends
    assert dead_key[1, 150:].all() and (dkv[dead_key] == 0).all()


@pytest.mark.parametrize("D", [64, 128])
def test_dropout_packed_qkv(D):
    from apex_example_amd.ops import attention as A

    B, S, H, p, seed = 2, 200, 2, 0.1, 77
    torch.manual_seed(0)
    qkv = torch.randn(B, S, 3, H, D, device=DEV, dtype=torch.bfloat16)
    do = torch.randn(B, S, H, D, device=DEV, dtype=torch.bfloat16)
    mask = make_mask("tril", S, S)
    ro, _, _, *rg = ref_all(*qkv.unbind(2), do, mask, p, seed)
    pm = A.prepare_attn_mask(mask)
    grads = []
    for _ in range(2):
        x = qkv.clone().requires_grad_(True)
        o = A.AttentionFunction.apply("packed_qkv", False, p, 1.0 / math.sqrt(D), seed, None,
                                      None, pm, x)
        o.backward(do)
        grads.append(x.grad)
    close(o, ro, 3e-2, "o")
    for i, what in enumerate(("dq", "dk", "dv")):
        close(grads[0][:, :, i], rg[i], 3e-2, what)
    assert torch.equal(grads[0], grads[1])


def _classes(attend, rows, cols):
    """dead / mixed / full (0 / 1 / 2) per rows x cols tile of a bool [R, C] matrix, tiles
    that reach past it counting the missing pairs as masked."""
    R, C = attend.shape
    nr, nc = -(-R // rows), -(-C // cols)
    pad = torch.zeros(nr * rows, nc * cols, dtype=torch.int64, device=attend.device)
    pad[:R, :C] = attend
    cnt = pad.view(nr, rows, nc, cols).sum((1, 3))
    return ((cnt > 0).int() + (cnt == rows * cols).int()).to(torch.uint8)


@pytest.mark.parametrize("pattern,kinds", [("tril", {0, 1, 2}), ("holes", {1, 2})])
def test_prepared_classes_and_reuse(pattern, kinds):
    from apex_example_amd.ops import fused_attention, prepare_attn_mask

    S = 200
    mask = make_mask(pattern, S, S)
    pm = prepare_attn_mask(mask)
    assert (pm.B, pm.Sq, pm.Sk) == (None, S, S) and pm.wq.shape == (1, 2, 4, 128)
    cq, ck = _classes(~mask, 128, 64), _classes(~mask.t(), 128, 64)
    assert torch.equal(pm.cq[0], cq) and torch.equal(pm.ck[0], ck)
    assert set(cq.flatten().tolist()) | set(ck.flatten().tolist()) == kinds
    q, kv, _ = rand_qkv(2, S, S, 2, 64, torch.bfloat16)
    a = fused_attention(q, kv[:, :, 0], kv[:, :, 1], attn_mask=mask)
    assert torch.equal(a, fused_attention(q, kv[:, :, 0], kv[:, :, 1], attn_mask=pm))


@pytest.mark.parametrize("bad", ["causal", "key_bias", "floating", "cpu", "shape"])
def test_validation(bad):
    from apex_example_amd.ops import fused_attention

    S = 70
    q, kv, _ = rand_qkv(2, S, S, 2, 64, torch.bfloat16)
    mask, kw = make_mask("band", S, S), {}
    if bad == "causal":
        kw = {"causal": True}
    elif bad == "key_bias":
        kw = {"key_bias": torch.zeros(2, S, device=DEV)}
    elif bad == "floating":
        mask = mask.float()
    elif bad == "cpu":
        mask = mask.cpu()
    elif bad == "shape":
        mask = mask[:, :-1]
    with pytest.raises(ValueError):
        fused_attention(q, kv[:, :, 0], kv[:, :, 1], attn_mask=mask, **kw)


@pytest.mark.parametrize("kind", ["self", "encdec"])
def test_module_routing(monkeypatch, kind):
    from apex_example_amd.contrib.multihead_attn import EncdecMultiheadAttn, SelfMultiheadAttn

    cls = SelfMultiheadAttn if kind == "self" else EncdecMultiheadAttn
    Tq, Tk, B = (70, 70, 2) if kind == "self" else (70, 200, 2)
    torch.manual_seed(0)
    fast = cls(128, 2, bias=True, fused_attn_mask=True).to(DEV).to(torch.bfloat16)
    ref = cls(128, 2, bias=True).to(DEV).to(torch.bfloat16)  # the default: SDPA
    ref.load_state_dict(fast.state_dict())
    x = torch.randn(Tq, B, 128, device=DEV, dtype=torch.bfloat16)
    mem = torch.randn(Tk, B, 128, device=DEV, dtype=torch.bfloat16)
    kpm = torch.zeros(B, Tk, dtype=torch.bool, device=DEV)
    kpm[1, Tk - 20:] = True
    am = make_mask("band", Tq, Tk)
    xa, xr = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    yr, _ = ref(xr, mem, key_padding_mask=kpm, attn_mask=am, is_training=False)
    dy = torch.randn_like(yr)
    yr.backward(dy)
    no_sdpa(monkeypatch)
    ya, _ = fast(xa, mem, key_padding_mask=kpm, attn_mask=am, is_training=False)
    ya.backward(dy)
    torch.testing.assert_close(ya.float(), yr.float(), rtol=2e-2, atol=2e-2)
    close(xa.grad, xr.grad.float(), 3e-2, "dx")
