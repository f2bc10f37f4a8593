"""Fused attention over packed variable-length sequences (the VARLEN kernels of
csrc/hip/attention.hip, ``ops.fused_attention_varlen[_qkv]``, ``contrib.fmha.FMHA`` and
BERT's ``unpad`` option) against the padded definition: the packed inputs scattered into a
right-padded [B, max L, H, 64] batch, ``attn_ref.ref_attention`` with a -inf key bias past
each length (and its exact dropout keep mask, whose hash takes sequence-local indices and
no length), read back at the rows below each length; ``do`` is zero on padded rows.

Bounds are those of tests/test_attention_cross_gpu.py: o rtol = atol = 2e-2, lse 1e-3 on
live rows, gradients max-error / max-reference below 2e-2 (bf16) / 6e-3 (fp16), 3e-2 with
dropout."""
import itertools

import pytest
import torch

from attn_ref import DEV, NEG, _C, close as _close, finite as _finite, no_sdpa as _no_sdpa
from attn_ref import ref_attention, ref_grads as _ref_grads
import dropout_hash  # noqa: F401  (the reference's keep mask)

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
# single token, both sides of the 64-key tile and the 128-row workgroup, unaligned starts
LENS_MIXED = (1, 63, 64, 65, 127, 128, 129, 200)
LENGTH_SETS = [
    (LENS_MIXED, 2),
    ((0, 5, 0, 130, 0), 1),     # empty sequences first, between and last
    ((320,), 1),                # one sequence, more than four key tiles per wave
    ((64, 64, 64, 64), 3),      # everything aligned, B * H not a multiple of 8
]


def _rel(dt):
    return 2e-2 if dt == torch.bfloat16 else 6e-3


def _cu(lens):
    return torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32, device=DEV)


def _inputs(lens, H, dt, seed=0):
    torch.manual_seed(seed)
    T = sum(lens)
    return tuple(torch.randn(T, H, 64, device=DEV, dtype=dt) for _ in range(4))  # q, k, v, do


def _pad(x, lens):
    """packed [T, ...] -> right-padded [B, max L, ...], zeros on the padding"""
    out = x.new_zeros(len(lens), max(max(lens), 1), *x.shape[1:])
    s = 0
    for b, n in enumerate(lens):
        out[b, :n] = x[s:s + n]
        s += n
    return out


def _unpad(y, lens):
    """[B, max L, ...] -> packed [T, ...]: rows < L_b of every sequence"""
    return torch.cat([y[b, :n] for b, n in enumerate(lens)])


def _bias(lens):
    S = max(max(lens), 1)
    gone = torch.arange(S).view(1, S) >= torch.tensor(lens).view(-1, 1)
    return torch.zeros(len(lens), S).masked_fill(gone, NEG).to(DEV)


_REF = {}


def _reference(lens, H, dt, causal, p=0.0, seed=0, inputs_seed=0):
    """Packed inputs and the padded reference's o, lse ([B, H, max L]) and gradients in
    packed order, computed once per case and left unchanged."""
    key = (lens, H, dt, causal, p, seed, inputs_seed)
    if key not in _REF:
        q, k, v, do = _inputs(lens, H, dt, inputs_seed)
        pq, pk, pv, pdo = (_pad(t, lens) for t in (q, k, v, do))
        bias = _bias(lens)
        ro, rlse, _ = ref_attention(pq, pk, pv, causal, bias, p=p, seed=seed)
        rq, rk, rv = _ref_grads(pq, pk, pv, pdo, causal, bias, p=p, seed=seed)
        _REF[key] = dict(q=q, k=k, v=v, do=do, ro=_unpad(ro, lens), rlse=rlse,
                         rq=_unpad(rq, lens), rk=_unpad(rk, lens), rv=_unpad(rv, lens))
    return _REF[key]


def _run(q, k, v, do, cu, max_seqlen=None, **kw):
    """fused_attention_varlen forward + backward on fresh leaves -> (o, dq, dk, dv)."""
    from apex_example_amd.ops import fused_attention_varlen

    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = fused_attention_varlen(q, k, v, cu, max_seqlen, **kw)
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


def _apply(q, k, v, do, cu, max_seqlen, causal, p, seed):
    """The op with an explicit dropout seed -> (o, dq, dk, dv)."""
    from apex_example_amd.ops.attention import AttentionFunction

    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = AttentionFunction.apply("varlen_qkv", causal, p, 0.125, seed, None, None,
                                (cu, max_seqlen), q, k, v)
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


# ------------------------------------------------------- 1. fwd / bwd parity
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("lens,H", LENGTH_SETS)
def test_varlen_fwd_bwd(lens, H, causal, dt):
    c = _reference(lens, H, dt, causal)
    q, k, v, do = c["q"], c["k"], c["v"], c["do"]
    T, B, ms = sum(lens), len(lens), max(lens)
    cu = _cu(lens)
    o, lse = _C().fwd_varlen(q, k, v, cu, ms, causal, 0.0, 0, 0.125)
    assert o.shape == (T, H, 64) and o.is_contiguous() and lse.shape == (B, H, ms)
    _finite(o)
    torch.testing.assert_close(o.float(), c["ro"], rtol=2e-2, atol=2e-2)
    for b, n in enumerate(lens):   # rows >= L_b are unspecified
        _finite(lse[b, :, :n])
        torch.testing.assert_close(lse[b, :, :n], c["rlse"][b, :, :n], rtol=1e-3, atol=1e-3)
    o2, dq, dk, dv = _run(q, k, v, do, cu, causal=causal)   # max_seqlen from cu_seqlens
    assert torch.equal(o2, o)
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
    _finite(dq, dk, dv)
    _close(dq, c["rq"], _rel(dt), "dq")
    _close(dk, c["rk"], _rel(dt), "dk")
    _close(dv, c["rv"], _rel(dt), "dv")


# --------------------------------------------------------------- 2. packed qkv
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
def test_varlen_packed_qkv(causal, dt):
    """fused_attention_varlen_qkv on a [T, 3*H*64] projection viewed as [T, 3, H, 64]:
    qkv.grad has the projection's layout, matches the reference slice by slice and is
    bitwise the separate-q/k/v entry's."""
    from apex_example_amd.ops import fused_attention_varlen, fused_attention_varlen_qkv

    lens, H = LENS_MIXED, 2
    c = _reference(lens, H, dt, causal)
    T, cu = sum(lens), _cu(lens)
    proj = torch.stack((c["q"], c["k"], c["v"]), 1).reshape(T, 3 * H * 64)
    a = proj.clone().requires_grad_(True)
    oa = fused_attention_varlen_qkv(a.view(T, 3, H, 64), cu, causal=causal)
    oa.backward(c["do"])
    assert oa.shape == (T, H, 64)
    assert a.grad.shape == proj.shape and a.grad.stride() == proj.stride()
    torch.testing.assert_close(oa.float(), c["ro"], rtol=2e-2, atol=2e-2)
    g = a.grad.view(T, 3, H, 64)
    _finite(oa, g)
    _close(g[:, 0], c["rq"], _rel(dt), "dq")
    _close(g[:, 1], c["rk"], _rel(dt), "dk")
    _close(g[:, 2], c["rv"], _rel(dt), "dv")
    b = proj.clone().requires_grad_(True)
    ob = fused_attention_varlen(*b.view(T, 3, H, 64).unbind(1), cu, causal=causal)
    ob.backward(c["do"])
    assert torch.equal(oa, ob) and torch.equal(a.grad, b.grad)
    # the gradient the op itself returns: one tensor of qkv's shape and strides
    x = proj.view(T, 3, H, 64).transpose(1, 2).contiguous().requires_grad_(True)  # [T, H, 3, 64]
    seen = {}
    xv = x.transpose(1, 2)
    h = xv.register_hook(lambda gr: seen.__setitem__("s", gr.stride()))
    fused_attention_varlen_qkv(xv, cu, causal=causal).backward(c["do"])
    h.remove()
    assert seen["s"] == xv.stride()
    assert torch.equal(x.grad.transpose(1, 2), g)


# ------------------------------------------------- 3. writes stay inside sequences
def test_varlen_writes_stay_inside_sequences():
    lens, H, dt = LENS_MIXED, 2, torch.bfloat16
    C = _C()
    q, k, v, do = _inputs(lens, H, dt, seed=3)
    T, cu, ms = sum(lens), _cu(lens), max(lens)
    o, lse = C.fwd_varlen(q, k, v, cu, ms, False, 0.0, 0, 0.125)
    bufs = [torch.full((T + 64, H, 64), 7.0, device=DEV, dtype=dt) for _ in range(3)]
    C.bwd_varlen(do, q, k, v, o, lse, cu, ms, False, 0.0, 0, 0.125, *(b[:T] for b in bufs))
    for b in bufs:
        assert (b[T:] == 7.0).all()      # the 64 rows behind the last sequence
        _finite(b[:T])
    # a sequence's rows depend on that sequence alone: replace sequence 3's inputs
    s, e = int(cu[3]), int(cu[4])
    q2, k2, v2 = (t.clone() for t in (q, k, v))
    for t in (q2, k2, v2):
        t[s:e] = torch.randn_like(t[s:e])
    o2, lse2 = C.fwd_varlen(q2, k2, v2, cu, ms, False, 0.0, 0, 0.125)
    assert torch.equal(o2[:s], o[:s]) and torch.equal(o2[e:], o[e:])
    assert not torch.equal(o2[s:e], o[s:e])
    bufs2 = [torch.empty_like(q) for _ in range(3)]
    C.bwd_varlen(do, q2, k2, v2, o2, lse2, cu, ms, False, 0.0, 0, 0.125, *bufs2)
    for g2, g in zip(bufs2, bufs):
        assert torch.equal(g2[:s], g[:s]) and torch.equal(g2[e:], g[e:T])


# ------------------------------------------------------ 4. max_seqlen invariance
@pytest.mark.parametrize("causal", [False, True])
def test_varlen_max_seqlen_invariance(causal):
    lens, H = LENS_MIXED, 2
    q, k, v, do = _inputs(lens, H, torch.bfloat16, seed=4)
    cu = _cu(lens)
    runs = [_run(q, k, v, do, cu, ms, causal=causal) for ms in (200, 256, 1024)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


# ----------------------------------------------------------------- 5. dropout
@pytest.mark.parametrize("causal", [False, True])
def test_varlen_dropout_exact_keep_mask(causal):
    lens, H, dt, p, seed = LENS_MIXED, 2, torch.bfloat16, 0.1, 4321
    c = _reference(lens, H, dt, causal, p=p, seed=seed, inputs_seed=2)
    o, dq, dk, dv = _apply(c["q"], c["k"], c["v"], c["do"], _cu(lens), max(lens), causal, p, seed)
    _finite(o, dq, dk, dv)
    torch.testing.assert_close(o.float(), c["ro"], rtol=2e-2, atol=2e-2)
    _close(dq, c["rq"], 3e-2, "dq")
    _close(dk, c["rk"], 3e-2, "dk")
    _close(dv, c["rv"], 3e-2, "dv")


# ------------------------------------------------------------- 6. determinism
def test_varlen_deterministic():
    lens, H = LENS_MIXED, 2
    q, k, v, do = _inputs(lens, H, torch.bfloat16, seed=5)
    cu = _cu(lens)
    runs = [_apply(q, k, v, do, cu, 200, True, 0.1, 99) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ----------------------------------------------------------- 7. graph capture
def test_varlen_graph_replay_on_new_offsets():
    """max_seqlen given: no host sync, so forward + backward capture into a graph; cu_seqlens
    is read on the device, so a replay serves other lengths written into the same tensor."""
    from apex_example_amd.ops import fused_attention_varlen_qkv

    H, ms, dt = 2, 256, torch.bfloat16
    lens_a, lens_b = (100, 37, 256, 1, 70), (200, 64, 0, 130, 70)   # one B, one T
    T = sum(lens_a)
    assert sum(lens_b) == T and max(lens_a + lens_b) <= ms
    torch.manual_seed(7)
    qkv = torch.randn(T, 3, H, 64, device=DEV, dtype=dt, requires_grad=True)
    do = torch.randn(T, H, 64, device=DEV, dtype=dt)
    cu = _cu(lens_a)

    def step():
        o = fused_attention_varlen_qkv(qkv, cu, ms)
        (g,) = torch.autograd.grad(o, qkv, do)
        return o, g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, g = step()
    new = torch.randn(T, 3, H, 64, device=DEV, dtype=dt)
    with torch.no_grad():
        qkv.copy_(new)
        cu.copy_(_cu(lens_b))
    graph.replay()
    torch.cuda.synchronize()
    e = new.clone().requires_grad_(True)
    eo = fused_attention_varlen_qkv(e, _cu(lens_b), ms)
    eo.backward(do)
    assert torch.equal(o, eo.detach()) and torch.equal(g, e.grad)


# ------------------------------------------------------------- 8. validation
def test_varlen_argument_validation():
    from apex_example_amd.ops import fused_attention_varlen, fused_attention_varlen_qkv

    lens, H = (5, 60), 1
    q, k, v, _ = _inputs(lens, H, torch.bfloat16)
    T = sum(lens)
    bad = lambda *xs: torch.tensor(xs, dtype=torch.int32, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="non-decreasing"):
        fused_attention_varlen(q, k, v, bad(0, 70, T))
    with pytest.raises(ValueError, match="start at 0"):
        fused_attention_varlen(q, k, v, bad(1, 5, T))
    with pytest.raises(ValueError, match="end at T"):
        fused_attention_varlen(q, k, v, bad(0, 5, T - 1))
    with pytest.raises(ValueError, match="int32"):
        fused_attention_varlen(q, k, v, _cu(lens).long())
    with pytest.raises(ValueError, match="cpu"):
        fused_attention_varlen(q, k, v, _cu(lens).cpu())
    gone = torch.zeros(2, 60, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError, match="key masks"):
        fused_attention_varlen(q, k, v, _cu(lens), key_padding_mask=gone)
    with pytest.raises(ValueError, match="key masks"):
        fused_attention_varlen_qkv(torch.stack((q, k, v), 1), _cu(lens),
                                   key_bias=torch.zeros(2, 60, device=DEV))
    with pytest.raises(ValueError, match="qkv must be"):
        fused_attention_varlen_qkv(q, _cu(lens))
    with pytest.raises(ValueError, match="max_seqlen"):
        fused_attention_varlen(q, k, v, _cu(lens), max_seqlen=0)


def test_varlen_binding_validation():
    C = _C()
    lens, H = (5, 60), 2
    q, k, v, do = _inputs(lens, H, torch.bfloat16)
    T, cu, ms = sum(lens), _cu(lens), 60
    args = (False, 0.0, 0, 0.125)
    with pytest.raises(RuntimeError, match="int32"):
        C.fwd_varlen(q, k, v, cu.long(), ms, *args)
    with pytest.raises(RuntimeError, match="int32"):
        C.fwd_varlen(q, k, v, cu.view(1, -1), ms, *args)
    with pytest.raises(RuntimeError, match="int32"):
        C.fwd_varlen(q, k, v, torch.stack((cu, cu), 1)[:, 0], ms, *args)   # not contiguous
    with pytest.raises(RuntimeError, match="int32"):
        C.fwd_varlen(q, k, v, cu[:0], ms, *args)
    with pytest.raises(RuntimeError, match="q's device"):
        C.fwd_varlen(q, k, v, cu.cpu(), ms, *args)
    for bad_ms in (0, -1, 1 << 24):
        with pytest.raises(RuntimeError, match="max_seqlen"):
            C.fwd_varlen(q, k, v, cu, bad_ms, *args)
    with pytest.raises(RuntimeError, match="tokens or heads"):
        C.fwd_varlen(q, k[:-1], v[:-1], cu, ms, *args)
    with pytest.raises(RuntimeError, match="tokens or heads"):
        C.fwd_varlen(q, k[:, :1], v[:, :1], cu, ms, *args)
    with pytest.raises(RuntimeError, match="one dtype"):
        C.fwd_varlen(q, k.half(), v, cu, ms, *args)
    with pytest.raises(RuntimeError, match=r"\[T,H,64\]"):
        C.fwd_varlen(q[None], k[None], v[None], cu, ms, *args)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        C.fwd_varlen(torch.randn(T, H, 68, device=DEV, dtype=q.dtype)[:, :, 4:], k, v, cu, ms,
                     *args)
    wide = torch.empty(2, 1, 1 << 24, device=DEV, dtype=q.dtype)[:, :, :64]   # 64 MiB
    with pytest.raises(RuntimeError, match="token stride"):
        C.fwd_varlen(wide, wide, wide, _cu((2,)), 2, *args)
    o, lse = C.fwd_varlen(q, k, v, cu, ms, *args)
    dq, dk, dv = (torch.empty_like(q) for _ in range(3))
    with pytest.raises(RuntimeError, match="shaped like q"):
        C.bwd_varlen(do, q, k, v, o, lse, cu, ms, *args, dq[:-1], dk, dv)
    with pytest.raises(RuntimeError, match="lse must be"):
        C.bwd_varlen(do, q, k, v, o, lse[:, :, :-1], cu, ms, *args, dq, dk, dv)
    # T = 0 and B = 0: empty / zero results, no launch
    e = q[:0]
    o0, lse0 = C.fwd_varlen(e, e, e, _cu((0, 0)), 1, *args)
    assert o0.shape == (0, H, 64) and lse0.shape == (2, H, 1)
    C.bwd_varlen(e, e, e, e, o0, lse0, _cu((0, 0)), 1, *args, e.clone(), e.clone(), e.clone())
    o0, lse0 = C.fwd_varlen(q, k, v, cu[:1], ms, *args)
    assert o0.shape == q.shape and (o0 == 0).all() and lse0.shape == (0, H, ms)
    grads = [torch.full_like(q, 7.0) for _ in range(3)]
    C.bwd_varlen(do, q, k, v, o0, lse0, cu[:1], ms, *args, *grads)
    assert all((t == 0).all() for t in grads)


# ---------------------------------------------------------------- 9. FMHA
def _fmha(hidden=128, heads=2, p=0.0):
    from types import SimpleNamespace

    from apex_example_amd.contrib.fmha import FMHA

    return FMHA(SimpleNamespace(attention_probs_dropout_prob=p, num_attention_heads=heads,
                                hidden_size=hidden))


def test_fmha_takes_fused_path(monkeypatch):
    lens, dt = (40, 200, 1), torch.bfloat16
    m = _fmha()
    T, cu = sum(lens), _cu(lens)
    torch.manual_seed(9)
    qkv = torch.randn(T, 3 * 128, device=DEV, dtype=dt)
    dy = torch.randn(T, 128, device=DEV, dtype=dt)
    r = qkv.float().requires_grad_(True)      # fp32: the module's own per-sequence SDPA loop
    yr = m(r, cu, max(lens), is_training=False)
    yr.backward(dy.float())
    _no_sdpa(monkeypatch)
    a = qkv.clone().requires_grad_(True)
    ya = m(a, cu, max(lens), is_training=False, zero_tensors=True)
    ya.backward(dy)
    assert ya.shape == (T, 128) and ya.dtype == dt and a.grad.shape == qkv.shape
    _finite(ya, a.grad)
    torch.testing.assert_close(ya.float(), yr, rtol=2e-2, atol=2e-2)
    _close(a.grad, r.grad, _rel(dt), "dqkv")
    with pytest.raises(AssertionError, match="scaled_dot_product_attention was called"):
        m(r, cu, max(lens), is_training=False)


# ------------------------------------------------------------ 10. BERT unpad
def test_bert_unpad_matches_padded_fused_model(monkeypatch):
    from apex_example_amd.models.bert import BertConfig, BertModel

    kw = dict(vocab_size=512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
              intermediate_size=256, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
              max_position_embeddings=256)
    torch.manual_seed(0)
    a = BertModel(BertConfig(unpad=True, **kw)).to(DEV).to(torch.bfloat16)
    r = BertModel(BertConfig(**kw)).to(DEV).to(torch.bfloat16)
    r.load_state_dict(a.state_dict())
    B, S = 6, 200
    lens = torch.tensor([200, 137, 129, 65, 64, 1])
    ids = torch.randint(0, 512, (B, S), device=DEV)
    tt = torch.zeros(B, S, dtype=torch.long, device=DEV)
    keep = (torch.arange(S).view(1, S) < lens.view(B, 1)).to(DEV)
    am = keep.long()   # 1 = attend, 0 = padding
    _no_sdpa(monkeypatch)
    yr, pr = r(ids, tt, am)
    dy = torch.randn_like(yr) * keep.unsqueeze(-1)
    (yr * dy).sum().backward()
    ya, pa = a(ids, tt, am)
    (ya * dy).sum().backward()
    assert ya.shape == yr.shape and pa.shape == pr.shape
    torch.testing.assert_close(ya[keep].float(), yr[keep].float(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(pa.float(), pr.float(), rtol=2e-2, atol=2e-2)
    assert (ya[~keep] == 0).all()
    _close(a.layers[0].attention.qkv.weight.grad, r.layers[0].attention.qkv.weight.grad.float(),
           3e-2, "layer 0 qkv.weight.grad")
