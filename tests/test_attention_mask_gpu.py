"""Key-padding masks in the fused attention kernels (csrc/hip/attention.hip, KMASK
instantiations) vs fp32 torch references: boolean and additive per-batch key masks,
dead 64-key tiles anywhere in the row, fully masked rows, dropout with the exact
counter-hash keep mask, and the routing of the contrib modules and BERT."""
import math

import pytest
import torch

from attn_ref import (DEV, NEG, close as _close, finite as _finite, mask_kwargs as _mask_kwargs,
                      no_sdpa as _no_sdpa, ref_attention, ref_grads as _ref_grads)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64, 1), (6, 200, 2), (4, 320, 2)]
PATTERNS = ["right", "left", "hole", "bernoulli", "additive", "allmasked", "mixed"]


# ---------------------------------------------------------------------- masks
def _right_lens(B, S):
    lens = [S, 137, 129, 65, 64, 1]
    if B == 1:
        # not length 1 alone: one live key makes the softmax a constant, dq and dk of the
        # reference identically zero, and an error relative to their maximum meaningless
        return [min(41, S)]
    lens = [lens[i % 6] for i in range(B)] if B >= 6 else lens[-B:]
    return [min(n, S) for n in lens]


def _right(B, S):
    pos = torch.arange(S).view(1, S)
    return pos >= torch.tensor(_right_lens(B, S)).view(B, 1)


def make_bias(pattern, B, S):
    """The additive [B, S] fp32 key bias of a pattern (CPU) and whether the pattern is a
    boolean one (bias in {0, -inf}: key_padding_mask = bias == -inf)."""
    g = torch.Generator().manual_seed(1234)
    if pattern == "right":       # lengths 200, 137, 129, 65, 64, 1 at (6, 200)
        m = _right(B, S)
    elif pattern == "left":      # the first 70 keys masked
        m = (torch.arange(S) < (70 if S > 70 else S * 5 // 8)).expand(B, S)
    elif pattern == "hole":      # a whole dead 64-tile in the middle: keys 64..127
        lo, hi = (64, 128) if S >= 128 else (20, 40)
        pos = torch.arange(S)
        m = ((pos >= lo) & (pos < hi)).expand(B, S)
    elif pattern == "bernoulli":
        m = torch.rand(B, S, generator=g) < 0.3
    elif pattern == "additive":  # -10000 on padded keys, small finite biases on live ones
        m = _right(B, S)
        return torch.where(m, torch.full((B, S), -10000.0),
                           0.5 * torch.randn(B, S, generator=g)), False
    elif pattern == "allmasked":  # one batch element with every key masked
        m = _right(B, S).clone()
        m[B // 2] = True
    elif pattern == "mixed":      # row i = row i of pattern i, fully masked row last
        rows = [make_bias(p, B, S)[0][i] for i, p in enumerate(
            ["right", "left", "hole", "bernoulli", "additive", "allmasked"][:B])]
        if B >= 6:
            rows[5] = torch.full((S,), NEG)
        return torch.stack(rows), False
    else:
        raise AssertionError(pattern)
    return torch.zeros(B, S).masked_fill(m, NEG), True


def _packed(B, S, H, dt, seed=0):
    torch.manual_seed(seed)
    return torch.randn(B, S, 3, H, 64, device=DEV, dtype=dt)


_CASES = {}


def _case(B, S, H, dt, causal, pattern):
    """Inputs, fused results (separate q/k/v API) and the fp32 reference of one case,
    computed once and shared by the tests that look at it."""
    key = (B, S, H, dt, causal, pattern)
    if key not in _CASES:
        from apex_example_amd.ops import fused_attention
        from apex_example_amd import _native

        bias, boolean = make_bias(pattern, B, S)
        qkv = _packed(B, S, H, dt)
        q, k, v = (t.detach().clone().requires_grad_(True) for t in qkv.unbind(2))
        kw = _mask_kwargs(bias, boolean)
        o = fused_attention(q, k, v, causal=causal, **kw)
        torch.manual_seed(7)
        do = torch.randn_like(o)
        o.backward(do)
        prep = _native.require().attn.prepare_key_mask(
            (bias == NEG).to(DEV) if boolean else bias.to(DEV), S)
        _, lse = _native.require().attn.fwd(q.detach(), k.detach(), v.detach(), causal, 0.0, 0,
                                            0.125, *prep)
        bd = bias.to(DEV)
        ro, rlse, dead = ref_attention(q.detach(), k.detach(), v.detach(), causal, bd)
        rq, rk, rv = _ref_grads(q, k, v, do, causal, bd)
        _CASES[key] = dict(bias=bias, boolean=boolean, qkv=qkv, do=do, kw=kw, o=o.detach(),
                           lse=lse, dq=q.grad, dk=k.grad, dv=v.grad, ro=ro, rlse=rlse,
                           dead=dead, rq=rq, rk=rk, rv=rv)
    return _CASES[key]


def _params(f):
    # "mixed" is the six patterns in one batch of six, so only where B = 6
    cases = [(B, S, H, p) for (B, S, H) in SHAPES for p in PATTERNS if p != "mixed" or B >= 6]
    f = pytest.mark.parametrize("causal", [False, True])(f)
    f = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])(f)
    return pytest.mark.parametrize("B,S,H,pattern", cases)(f)


# ------------------------------------------------------------- prepared mask
@pytest.mark.parametrize("S", [1, 64, 200, 320])
@pytest.mark.parametrize("kind", ["bool", "uint8", "f32", "f16", "bf16"])
def test_prepare_key_mask(S, kind):
    from apex_example_amd import _native

    B = 6 if S >= 200 else 2
    bias, _ = make_bias("mixed" if B == 6 else "bernoulli", B, S)
    if kind in ("bool", "uint8"):
        bias = torch.zeros(B, S).masked_fill(bias == NEG, NEG)
        m = (bias == NEG).to(torch.bool if kind == "bool" else torch.uint8)
        if kind == "uint8":
            m = m * 3  # any non-zero byte masks
    else:
        m = bias.to({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[kind])
        bias = m.float()
    kb, live = _native.require().attn.prepare_key_mask(m.to(DEV), S)
    Sp = (S + 63) // 64 * 64
    assert kb.shape == (B, Sp) and kb.dtype == torch.float32
    assert live.shape == (B, Sp // 64) and live.dtype == torch.uint8
    want = torch.full((B, Sp), NEG)
    want[:, :S] = bias * math.log2(math.e)
    torch.testing.assert_close(kb.cpu(), want, rtol=1e-6, atol=0)
    want_live = (want.view(B, Sp // 64, 64) > NEG).any(-1).to(torch.uint8)
    assert torch.equal(live.cpu(), want_live)


# ------------------------------------------------------------ fwd / bwd parity
@_params
def test_masked_fwd(B, S, H, dt, causal, pattern):
    c = _case(B, S, H, dt, causal, pattern)
    _finite(c["o"])
    torch.testing.assert_close(c["o"].float(), c["ro"], rtol=2e-2, atol=2e-2)
    live = ~c["dead"]
    torch.testing.assert_close(c["lse"][live], c["rlse"][live], rtol=1e-3, atol=1e-3)
    # fully masked rows: exactly zero output
    dead_rows = c["dead"].permute(0, 2, 1)  # [B, S, H]
    assert (c["o"][dead_rows] == 0).all()


@_params
def test_masked_bwd(B, S, H, dt, causal, pattern):
    c = _case(B, S, H, dt, causal, pattern)
    rel = 2e-2 if dt == torch.bfloat16 else 6e-3
    _finite(c["dq"], c["dk"], c["dv"])
    _close(c["dq"], c["rq"], rel)
    _close(c["dk"], c["rk"], rel)
    _close(c["dv"], c["rv"], rel)
    # fully masked rows get exactly zero dq; masked keys exactly zero dk / dv
    assert (c["dq"][c["dead"].permute(0, 2, 1)] == 0).all()
    gone = (c["bias"] == NEG).to(DEV)
    assert (c["dk"][gone] == 0).all() and (c["dv"][gone] == 0).all()


@_params
def test_masked_qkv_packed(B, S, H, dt, causal, pattern):
    """fused_attention_qkv: same numbers, gradients in one packed dqkv of qkv's layout."""
    from apex_example_amd.ops import fused_attention_qkv

    c = _case(B, S, H, dt, causal, pattern)
    qkv = c["qkv"].detach().clone().requires_grad_(True)
    o = fused_attention_qkv(qkv, causal=causal, **c["kw"])
    o.backward(c["do"])
    g = qkv.grad
    assert g.shape == qkv.shape and g.is_contiguous()
    _finite(o, g)
    torch.testing.assert_close(o.float(), c["ro"], rtol=2e-2, atol=2e-2)
    rel = 2e-2 if dt == torch.bfloat16 else 6e-3
    _close(g[:, :, 0], c["rq"], rel)
    _close(g[:, :, 1], c["rk"], rel)
    _close(g[:, :, 2], c["rv"], rel)
    # the same kernels on the same values: bitwise the separate-tensor API's results
    assert torch.equal(o, c["o"])
    assert torch.equal(g[:, :, 0], c["dq"]) and torch.equal(g[:, :, 1], c["dk"])
    assert torch.equal(g[:, :, 2], c["dv"])


def test_all_masked_batch_element_exact_zeros():
    """Every key of one batch element masked: o, dq exactly 0 for it, nothing of it in
    dk / dv (exactly 0 there: its keys are masked too), no NaN / Inf anywhere."""
    for causal in (False, True):
        c = _case(6, 200, 2, torch.bfloat16, causal, "allmasked")
        b = 3
        assert c["dead"][b].all()
        for t in (c["o"], c["dq"], c["dk"], c["dv"]):
            assert (t[b] == 0).all()
            assert torch.isfinite(t.float()).all()


# ------------------------------------------------ boolean == 0 / -inf additive
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("pattern", ["right", "left", "hole", "bernoulli", "allmasked"])
def test_bool_and_inf_additive_bitwise_equal(pattern, dt, causal):
    from apex_example_amd.ops import fused_attention

    B, S, H = 6, 200, 2
    c = _case(B, S, H, dt, causal, pattern)
    assert c["boolean"]
    q, k, v = (t.detach().clone().requires_grad_(True) for t in c["qkv"].unbind(2))
    o = fused_attention(q, k, v, causal=causal, key_bias=c["bias"].to(DEV))
    o.backward(c["do"])
    assert torch.equal(o, c["o"])
    assert torch.equal(q.grad, c["dq"])
    assert torch.equal(k.grad, c["dk"])
    assert torch.equal(v.grad, c["dv"])


# -------------------------------------------------------------------- dropout
def _ratio(a, b):
    return (a.float() - b).abs().max().item() / (b.abs().max().item() + 1e-6)


def _dropout_case(causal, lens):
    """Dropout 0.1 under a right-padding mask of the given lengths, forward and the packed
    gradients against the fp32 reference with the exact keep mask."""
    from apex_example_amd.ops.attention import FusedQKVAttentionFunction, prepare_key_mask

    B, S, H, seed = len(lens), 200, 2, 4321
    gone = torch.arange(S).view(1, S) >= torch.tensor(lens).view(B, 1)
    bias = torch.zeros(B, S).masked_fill(gone, NEG).to(DEV)
    pm = prepare_key_mask(gone.to(DEV))
    qkv = _packed(B, S, H, torch.bfloat16, seed=1).requires_grad_(True)
    o = FusedQKVAttentionFunction.apply(qkv, causal, 0.1, 0.125, seed, pm.bias, pm.live)
    q, k, v = qkv.detach().unbind(2)
    ro, _, _ = ref_attention(q, k, v, causal, bias, p=0.1, seed=seed)
    do = torch.randn_like(o)
    o.backward(do)
    rq, rk, rv = _ref_grads(q, k, v, do, causal, bias, p=0.1, seed=seed)
    g = qkv.grad
    ratios = [_ratio(g[:, :, i], r) for i, r in enumerate((rq, rk, rv))]
    print("dropout causal=%s lens=%s: dq %.3e dk %.3e dv %.3e (bound 2e-2)" % (
        causal, lens, *ratios))
    _finite(o, g)
    torch.testing.assert_close(o.float(), ro, rtol=3e-2, atol=3e-2)
    assert (g[:, :, 1:][gone.to(DEV)] == 0).all()   # masked keys: exactly zero dk / dv
    assert max(ratios) < 2e-2, ratios


@pytest.mark.parametrize("causal", [False, True])
def test_masked_dropout_exact_keep_mask(causal):
    """Dropout 0.1 under the right-padding mask 200, 137, 129, 65, 64, 1: skipped tiles must
    not shift the keep hash, a pure function of (seed, b*H+h, q, key).

    The element of length 1 is the hard one for dk: with one live key p = 1 and the true
    dS = dP~ - D is exactly 0 for every query, so its dk is whatever error D carries,
    summed over all 200 queries onto that one key.  D = rowsum(dO * O) from the forward's
    bf16 O (rounded under dropout: O = bf16(V0 * 256 / 230)) put 0.08 there against a
    largest gradient of 3.1 (dk 4.0e-2 / 2.7e-2 of the maximum, non-causal / causal);
    the masked dQ kernel therefore hands dK/dV the D refined by its sum of dS (3.5e-3)."""
    _dropout_case(causal, [200, 137, 129, 65, 64, 1])


@pytest.mark.parametrize("causal", [False, True])
def test_masked_dropout_right_padding_no_single_key(causal):
    """The same with 33 live keys in place of 1 (no element whose p sits on one key): every
    tile boundary of the list above and the same seed."""
    _dropout_case(causal, [200, 137, 129, 65, 64, 33])


# ---------------------------------------------------------------- determinism
def test_masked_deterministic():
    from apex_example_amd.ops import fused_attention

    B, S, H = 6, 200, 2
    bias, _ = make_bias("mixed", B, S)
    q, k, v = (t.detach().clone().requires_grad_(True)
               for t in _packed(B, S, H, torch.bfloat16).unbind(2))
    do = torch.randn(B, S, H, 64, device=DEV, dtype=torch.bfloat16)
    runs = []
    for _ in range(2):
        for t in (q, k, v):
            t.grad = None
        o = fused_attention(q, k, v, causal=True, key_bias=bias.to(DEV))
        o.backward(do)
        runs.append([o.detach().clone()] + [t.grad.clone() for t in (q, k, v)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# --------------------------------------------------- all-False == mask-free
@pytest.mark.parametrize("B,S,H", SHAPES)
@pytest.mark.parametrize("causal", [False, True])
def test_all_false_mask_matches_mask_free(B, S, H, causal):
    from apex_example_amd.ops import fused_attention

    q, k, v = _packed(B, S, H, torch.bfloat16).unbind(2)
    o0 = fused_attention(q, k, v, causal=causal)
    o1 = fused_attention(q, k, v, causal=causal,
                         key_padding_mask=torch.zeros(B, S, dtype=torch.bool, device=DEV))
    torch.testing.assert_close(o1.float(), o0.float(), rtol=2e-2, atol=2e-2)


def test_prepared_mask_is_reusable():
    from apex_example_amd.ops import fused_attention, prepare_key_mask

    B, S, H = 6, 200, 2
    bias, _ = make_bias("right", B, S)
    m = (bias == NEG).to(DEV)
    pm = prepare_key_mask(m)
    q, k, v = _packed(B, S, H, torch.bfloat16).unbind(2)
    a = fused_attention(q, k, v, key_padding_mask=m)
    assert torch.equal(a, fused_attention(q, k, v, key_padding_mask=pm))
    assert torch.equal(a, fused_attention(q, k, v, key_bias=pm))


# -------------------------------------------------------------------- routing
def _mha_pair(**kw):
    from apex_example_amd.contrib.multihead_attn import SelfMultiheadAttn

    torch.manual_seed(0)
    fast = SelfMultiheadAttn(128, 2, bias=True, **kw).to(DEV).to(torch.bfloat16)
    ref = SelfMultiheadAttn(128, 2, bias=True, impl="default", **kw).to(DEV).to(torch.bfloat16)
    ref.load_state_dict(fast.state_dict())
    return fast, ref


@pytest.mark.parametrize("additive", [False, True])
def test_self_mha_key_padding_mask_takes_fused_path(monkeypatch, additive):
    T, B = 200, 6
    fast, ref = _mha_pair(mask_additive=additive)
    bias, _ = make_bias("right", B, T)
    kpm = (bias.to(DEV) if additive else (bias == NEG).to(DEV))
    x = torch.randn(T, B, 128, device=DEV, dtype=torch.bfloat16)
    xa, xr = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    yr, _ = ref(xr, key_padding_mask=kpm, is_training=False)
    dy = torch.randn_like(yr)
    yr.backward(dy)
    _no_sdpa(monkeypatch)
    ya, _ = fast(xa, key_padding_mask=kpm, is_training=False)
    ya.backward(dy)
    torch.testing.assert_close(ya.float(), yr.float(), rtol=2e-2, atol=2e-2)
    # two bf16 paths against each other, the bound the mask-free module tests use
    _close(xa.grad, xr.grad.float(), 3e-2)


def test_self_mha_attn_mask_still_reaches_sdpa(monkeypatch):
    T, B = 64, 2
    fast, _ = _mha_pair()
    x = torch.randn(T, B, 128, device=DEV, dtype=torch.bfloat16)
    am = torch.ones(T, T, device=DEV).triu(1).bool()
    y, _ = fast(x, attn_mask=am, is_training=False)   # works through SDPA
    assert torch.isfinite(y.float()).all()
    _no_sdpa(monkeypatch)
    with pytest.raises(AssertionError, match="scaled_dot_product_attention was called"):
        fast(x, attn_mask=am, is_training=False)
    with pytest.raises(AssertionError, match="scaled_dot_product_attention was called"):
        fast(x, attn_mask=am, key_padding_mask=torch.zeros(B, T, dtype=torch.bool, device=DEV),
             is_training=False)


def test_bert_attention_mask_takes_fused_path(monkeypatch):
    from apex_example_amd.models.bert import BertConfig, BertModel

    kw = dict(vocab_size=512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
              intermediate_size=256, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
              max_position_embeddings=256)
    torch.manual_seed(0)
    a = BertModel(BertConfig(**kw)).to(DEV).to(torch.bfloat16)
    r = BertModel(BertConfig(fused_attention=False, **kw)).to(DEV).to(torch.bfloat16)
    r.load_state_dict(a.state_dict())
    B, S = 6, 200
    ids = torch.randint(0, 512, (B, S), device=DEV)
    tt = torch.zeros(B, S, dtype=torch.long, device=DEV)
    am = (~_right(B, S)).long().to(DEV)   # 1 = attend, 0 = padding
    yr, pr = r(ids, tt, am)
    dy = torch.randn_like(yr)
    (yr * dy).sum().backward()
    _no_sdpa(monkeypatch)
    ya, pa = a(ids, tt, am)
    (ya * dy).sum().backward()
    torch.testing.assert_close(ya.float(), yr.float(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(pa.float(), pr.float(), rtol=2e-2, atol=2e-2)
    _close(a.layers[0].attention.qkv.weight.grad, r.layers[0].attention.qkv.weight.grad.float(),
           3e-2)


# ----------------------------------------------------------------- validation
def test_argument_validation():
    from apex_example_amd.ops import fused_attention, fused_attention_qkv, prepare_key_mask

    B, S, H = 2, 64, 1
    qkv = _packed(B, S, H, torch.bfloat16)
    q, k, v = qkv.unbind(2)
    ok = torch.zeros(B, S, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError, match=r"\[B, S\]"):
        fused_attention(q, k, v, key_padding_mask=torch.zeros(B, S + 1, dtype=torch.bool,
                                                              device=DEV))
    with pytest.raises(ValueError, match=r"\[B, S\]"):
        fused_attention_qkv(qkv, key_bias=torch.zeros(B + 1, S, device=DEV))
    with pytest.raises(ValueError, match="cpu"):
        fused_attention(q, k, v, key_padding_mask=ok.cpu())
    with pytest.raises(ValueError, match="not both"):
        fused_attention(q, k, v, key_padding_mask=ok, key_bias=torch.zeros(B, S, device=DEV))
    with pytest.raises(ValueError, match="not both"):
        fused_attention_qkv(qkv, key_padding_mask=ok, key_bias=torch.zeros(B, S, device=DEV))
    with pytest.raises(ValueError, match="key_bias"):
        fused_attention(q, k, v, key_padding_mask=torch.zeros(B, S, device=DEV))
    with pytest.raises(ValueError, match="prepared key mask is for"):
        fused_attention(q, k, v, key_bias=prepare_key_mask(torch.zeros(B, S + 64, device=DEV)))


def test_binding_validation():
    from apex_example_amd import _native

    C = _native.require().attn
    B, S, H = 2, 64, 1
    q, k, v = _packed(B, S, H, torch.bfloat16).unbind(2)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        C.prepare_key_mask(torch.zeros(B, S, dtype=torch.bool), S)
    with pytest.raises(RuntimeError, match=r"\[B, S\]"):
        C.prepare_key_mask(torch.zeros(B, S, dtype=torch.bool, device=DEV), S + 1)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.prepare_key_mask(torch.zeros(S, B, dtype=torch.bool, device=DEV).t(), S)
    with pytest.raises(RuntimeError, match="mask expected"):
        C.prepare_key_mask(torch.zeros(B, S, dtype=torch.int64, device=DEV), S)
    kb, live = C.prepare_key_mask(torch.zeros(B, S, dtype=torch.bool, device=DEV), S)
    with pytest.raises(RuntimeError, match="pair"):
        C.fwd(q, k, v, False, 0.0, 0, 0.125, kb)
    with pytest.raises(RuntimeError, match="key_bias must be"):
        C.fwd(q, k, v, False, 0.0, 0, 0.125, kb[:1], live)
    with pytest.raises(RuntimeError, match="key_live must be"):
        C.fwd(q, k, v, False, 0.0, 0, 0.125, kb, live[:1])
    with pytest.raises(RuntimeError, match="device"):
        C.fwd(q, k, v, False, 0.0, 0, 0.125, kb.cpu(), live.cpu())
