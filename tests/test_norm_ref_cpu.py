"""The float64 LayerNorm / RMSNorm / residual-join references of tests/norm_ref.py are
right (no GPU, no extension needed): they agree with torch in float64 under double
autograd to 1e-12, their error magnitudes behave as documented, and the constant K of
the tolerance holds the float32 emulation of every reference under half the bound on
exactly the shapes and inputs the kernels are held to.  A wrong reference cannot bless a
wrong kernel."""
import pytest
import torch
import torch.nn.functional as F

import norm_ref as R
from norm_ref import BF16, F16, F32

F64 = torch.float64


def _close(got, want, what):
    # rtol 1e-12 of the element, plus 1e-12 of the largest element for results that are
    # themselves differences of O(max) terms (dx of a near-constant dy, mean of a
    # centred row): float64 cannot do better there in either implementation
    atol = 1e-12 * float(want.abs().max()) if want.numel() else 0.0
    torch.testing.assert_close(got, want, rtol=1e-12, atol=atol, msg=lambda m: what + ": " + m)


# ------------------------------------------------------------ reference vs torch float64
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("shape,nshape", [((5, 64), (64,)), ((33, 777), (777,)),
                                          ((2, 3, 4, 256), (4, 256)), ((7, 2, 3, 5), (3, 5))])
@pytest.mark.parametrize("eps", [1e-5, 1e-12, 0.1])
def test_ref_layer_norm_matches_torch(shape, nshape, affine, dtype, eps):
    n2 = 1
    for s in nshape:
        n2 *= s
    n1 = 1
    for s in shape:
        n1 *= s
    n1 //= n2
    x, dy, gamma, beta = R.make_inputs(n1, n2, dtype, shape=shape)
    gamma, beta = (gamma.reshape(nshape), beta.reshape(nshape)) if affine else (None, None)
    xd = x.to(F64).requires_grad_(True)
    gd = gamma.to(F64).requires_grad_(True) if affine else None
    bd = beta.to(F64).requires_grad_(True) if affine else None
    # eps as the kernels receive it (float32), like the reference takes it
    yd = F.layer_norm(xd, nshape, gd, bd, R.f32(eps))
    yd.backward(dy.to(F64))
    fw = R.ref_forward(x, gamma, beta, n2, eps, False)
    bw = R.ref_backward(dy, x, gamma, n2, eps, False)
    _close(fw["y"].v, yd.detach(), "y")
    x2 = x.to(F64).reshape(n1, n2)
    _close(fw["mean"].v, x2.mean(1), "mean")
    _close(fw["invvar"].v, (x2.var(1, unbiased=False) + R.f32(eps)).rsqrt(), "invvar")
    _close(bw["dx"].v, xd.grad, "dx")
    assert fw["y"].v.shape == x.shape and bw["dx"].v.shape == x.shape
    if affine:
        _close(bw["dgamma"].v.reshape(nshape), gd.grad, "dgamma")
        _close(bw["dbeta"].v.reshape(nshape), bd.grad, "dbeta")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("shape,nshape", [((5, 64), (64,)), ((33, 777), (777,)),
                                          ((7, 2, 3, 5), (3, 5))])
def test_ref_rms_norm_matches_torch(shape, nshape, affine, dtype):
    n2 = 1
    for s in nshape:
        n2 *= s
    n1 = 1
    for s in shape:
        n1 *= s
    n1 //= n2
    eps = 1e-5
    x, dy, gamma, _ = R.make_inputs(n1, n2, dtype, shape=shape)
    gamma = gamma.reshape(nshape) if affine else None
    xd = x.to(F64).requires_grad_(True)
    gd = gamma.to(F64).requires_grad_(True) if affine else None
    dims = tuple(range(-len(nshape), 0))
    yd = xd * torch.rsqrt(xd.pow(2).mean(dims, keepdim=True) + R.f32(eps))
    if affine:
        yd = yd * gd
    yd.backward(dy.to(F64))
    fw = R.ref_forward(x, gamma, None, n2, eps, True)
    bw = R.ref_backward(dy, x, gamma, n2, eps, True)
    _close(fw["y"].v, yd.detach(), "y")
    assert bool((fw["mean"].v == 0).all()) and bool((fw["mean"].e == 0).all())
    _close(bw["dx"].v, xd.grad, "dx")
    if affine:
        _close(bw["dgamma"].v.reshape(nshape), gd.grad, "dgamma")
        _close(bw["dbeta"].v, dy.to(F64).reshape(n1, n2).sum(0), "dbeta")


@pytest.mark.parametrize("dtype,wdtype", [(F32, F32), (BF16, F32), (BF16, BF16)])
@pytest.mark.parametrize("p", R.JOIN_P)
@pytest.mark.parametrize("use", ["both", "y", "s"])
def test_ref_join_matches_torch(dtype, wdtype, p, use):
    """The same chain in torch float64 with the given keep mask: s rounded once to x's
    type, LayerNorm of the stored s, double autograd for ds / dh / dgamma / dbeta."""
    n1, n2, eps = 9, 520, 1e-5
    x, h, keep, dy, de, gamma, beta = R.make_join_inputs(n1, n2, dtype, wdtype, p)
    dy_, de_ = (dy if use != "s" else None), (de if use != "y" else None)
    scale = R.join_scale(p)
    s64 = x.to(F64) + keep.to(F64) * h.to(F64) * scale
    s_st = s64.to(dtype)
    fw = R.ref_join_forward(x, h, keep, p, gamma, beta, n2, eps)
    _close(fw["s"].v, s64, "s")
    sd = s_st.to(F64).requires_grad_(True)
    gd, bd = gamma.to(F64).requires_grad_(True), beta.to(F64).requires_grad_(True)
    yd = F.layer_norm(sd, (n2,), gd, bd, R.f32(eps))
    _close(fw["y"].v, yd.detach(), "y")
    loss = (yd * dy.to(F64)).sum() if dy_ is not None else (yd * 0).sum()
    loss.backward()
    ds64 = sd.grad + (de.to(F64) if de_ is not None else 0)
    dh64 = keep.to(F64) * ds64 * scale
    bw = R.ref_join_backward(dy_, de_, s_st, keep, p, gamma, n2, eps, h_dtype=dtype)
    _close(bw["ds"].v, ds64, "ds")
    _close(bw["dh"].v, dh64, "dh")
    _close(bw["dgamma"].v, gd.grad, "dgamma")
    _close(bw["dbeta"].v, bd.grad, "dbeta")
    _close(bw["dhsum"].v, dh64.to(dtype).to(F64).sum(0), "dhsum")
    # given stored tensors are used instead of the ones rounded here
    bw2 = R.ref_join_backward(dy_, de_, s_st, keep, p, gamma, n2, eps, dh_stored=dh64.to(dtype) * 2)
    _close(bw2["dhsum"].v, bw["dhsum"].v * 2, "dhsum of the stored dh")
    fw2 = R.ref_join_forward(x, h, keep, p, gamma, beta, n2, eps, s_stored=s_st * 2)
    _close(fw2["mean"].v, fw["mean"].v * 2, "mean of the stored s")


# --------------------------------------------------------- chains and error magnitudes
def test_chain_constants():
    # fast: 8*VPT + 6; generic: ceil(n2/256) + 10; the larger where both exist
    assert R.row_chain(8) == 14 and R.row_chain(512) == 14 and R.row_chain(520) == 22
    assert R.row_chain(2048) == 38 and R.row_chain(2056) == 19 and R.row_chain(4100) == 27
    assert R.row_chain(7) == 11 and R.row_chain(777) == 14
    # fast: rows per wave + 4 + ceil(blocks/32) + 5; generic: rows per part + ceil(parts/32) + 5
    assert R.col_chain(5, 64) == max(1 + 4 + 1 + 5, 5 + 1 + 5)
    assert R.col_chain(4100, 64) == max(2 + 4 + 32 + 5, 32 + 5 + 5)
    assert R.col_chain(32772, 64) == max(9 + 4 + 32 + 5, 65 + 16 + 5)
    assert R.col_chain(16400, 7) == 33 + 16 + 5
    assert R.col_chain(33, 777) == 17 + 1 + 5
    assert R.col_chain(0, 64) == R.col_chain(1, 64)


def test_vsum_budgets_magnitudes_not_the_sum():
    v = R.Val(torch.tensor([[1.0, -1.0, 2.0, -2.0]], dtype=F64))
    s = R.vsum(v, 1, 10.0)
    assert float(s.v) == 0.0 and float(s.e) == 60.0
    w = R.Val(v.v, torch.full_like(v.v, 0.5))
    assert float(R.vsum(w, 1, 10.0, keepdim=True).e) == 62.0
    r = R.vrsqrt(R.Val(torch.tensor([4.0], dtype=F64), torch.tensor([8.0], dtype=F64)))
    assert float(r.v) == 0.5 and float(r.e) == 8.0 * 0.5 / 8.0 + 1.0


def test_error_magnitudes_scale_and_cover_the_value():
    x, dy, gamma, beta = R.make_inputs(5, 64, F32)
    a = R.ref_forward(x, gamma, beta, 64, 1e-5, False)
    assert bool((a["y"].e >= a["y"].v.abs()).all())
    # x scaled by 8 with eps scaled by 64: S of the mean scales by 8, invvar's by 1/8
    b = R.ref_forward(x * 8, gamma, None, 64, 1e-12, False)
    a = R.ref_forward(x, gamma, None, 64, 1e-12 / 64, False)
    torch.testing.assert_close(b["mean"].e, a["mean"].e * 8, rtol=1e-12, atol=0)
    torch.testing.assert_close(b["invvar"].e, a["invvar"].e / 8, rtol=1e-12, atol=0)
    torch.testing.assert_close(b["y"].e, a["y"].e, rtol=1e-12, atol=0)
    # the mean's error reaches y to first order but the variance to second order only
    off = R.ref_forward(x * 0.01 + 1000, None, None, 64, 1e-5, False)
    ctr = R.ref_forward(x * 0.01, None, None, 64, 1e-5, False)
    assert float((off["y"].e / ctr["y"].e).min()) > 100
    # (|mu| / sigma = 5e4: a first-order budget, 2*|d|*e_mu per element, would let invvar
    # be off by a third; the second-order one holds it to a few per cent)
    assert float((R.K * R.EPS32 * off["invvar"].e / off["invvar"].v).max()) < 0.05


# ------------------------------------------------------------------ the constant K
def _fwd_bwd(x, dy, gamma, beta, n2=None, eps=1e-5, rms=False, work=F64):
    out = R.ref_forward(x, gamma, beta, n2, eps, rms, work=work)
    out.update(R.ref_backward(dy, x, gamma, n2, eps, rms, work=work))
    return out


def _join(x, h, keep, dy, de, gamma, beta, p=0.0, n2=None, eps=1e-5, s_st=None, dh_st=None,
          work=F64):
    out = R.ref_join_forward(x, h, keep, p, gamma, beta, n2, eps, s_stored=s_st, work=work)
    out.update(R.ref_join_backward(dy, de, s_st, keep, p, gamma, n2, eps, dh_stored=dh_st,
                                   work=work))
    return out


def _k_cases():
    """(operator, fn, tensors, kwargs): every shape x {LayerNorm, RMSNorm} affine x
    {fp32, bf16}; every operator / type / parameter-type combination on a fast and a
    generic shape; eps; the conditioning inputs; the join corners."""
    def case(n1, n2, dt, wdt, rms, affine, eps=1e-5, kind="randn"):
        x, dy, gamma, beta = R.make_inputs(n1, n2, dt, wdt, kind=kind)
        if not affine:
            gamma = beta = None
        if rms:
            beta = None
        return ("rms_norm" if rms else "layer_norm", _fwd_bwd, (x, dy, gamma, beta),
                dict(n2=n2, eps=eps, rms=rms))

    for n1, n2 in R.shapes() + [(0, 64), (0, 777)]:
        for dt in (F32, BF16):
            for rms in (False, True):
                yield case(n1, n2, dt, None, rms, True)
    for n1, n2 in R.COMBO_SHAPES:
        for dt, wdt in R.TYPE_COMBOS:
            for rms, affine in R.OPERATORS:
                yield case(n1, n2, dt, wdt, rms, affine)
    for eps in (1e-12, 0.1):
        for n1, n2 in R.COMBO_SHAPES:
            for dt in (F32, BF16):
                for rms in (False, True):
                    yield case(n1, n2, dt, None, rms, True, eps=eps)
    for kind, dt, n2 in R.conditioning_cases():
        for rms in (False, True):
            yield case(R.COND_N1, n2, dt, None, rms, True, kind=kind)
    for i, (n1, n2) in enumerate(R.JOIN_SHAPES):
        p = R.JOIN_P[i % 3]
        x, h, keep, dy, de, gamma, beta = R.make_join_inputs(n1, n2, BF16, F32, p)
        fw = R.ref_join_forward(x, h, keep, p, gamma, beta, n2, 1e-5)
        s_st = fw["s"].v.to(BF16)
        bw = R.ref_join_backward(dy, de, s_st, keep, p, gamma, n2, 1e-5, h_dtype=BF16)
        yield ("join", _join, (x, h, keep, dy, de, gamma, beta),
               dict(p=p, n2=n2, s_st=s_st, dh_st=bw["dh"].v.to(BF16)))


def test_k_measured():
    """The float32 emulation of every reference (same formulas, float32 torch ops) stays
    under half the bound K*eps32*S; the worst ratios (in units of eps32*S) are the figures
    written next to K in norm_ref.py."""
    worst = {}
    for name, fn, tensors, kw in _k_cases():
        for out, r in R.emulation_ratio(fn, *tensors, **kw).items():
            key = "%s.%s" % (name, out)
            worst[key] = max(worst.get(key, 0.0), r)
    print("K measurement:", "  ".join("%s %.2f" % kv for kv in sorted(worst.items())))
    for name, r in worst.items():
        assert r <= R.K / 2, (name, r)


@pytest.mark.parametrize("kind,dtype,n2", [c for c in R.conditioning_cases()
                                           if c[0].startswith("offset")])
def test_offset_rows_separate_two_pass_from_one_pass(kind, dtype, n2):
    """The offset rows prove something only if the algorithm they are meant to catch fails
    on them: the two-pass float32 emulation stays inside K/2 while a one-pass
    E[x^2] - mu^2 in float32 lands outside the bound of invvar (or is not finite)."""
    x, dy, gamma, beta = R.make_inputs(R.COND_N1, n2, dtype, kind=kind)
    assert float(x.float().std(1).min()) > 0   # the rows did not round to a constant
    ratios = R.emulation_ratio(_fwd_bwd, x, dy, gamma, beta, n2=n2, eps=1e-5, rms=False)
    print("two-pass float32 emulation:", ratios)
    assert max(ratios.values()) <= R.K / 2
    ref = R.ref_forward(x, gamma, beta, n2, 1e-5, False)
    _, iv1 = R.one_pass_forward(x, n2, 1e-5)
    out = R.worst_ratio(iv1, ref["invvar"], R.K)
    print("one-pass float32 invvar: |err| / bound = %g" % out)
    assert out > 1.0
    # the same one-pass formula in float64 is fine: it is the precision, not the formula
    _, iv64 = R.one_pass_forward(x, n2, 1e-5, work=F64)
    assert R.worst_ratio(iv64.float(), ref["invvar"], R.K) <= 1.0


def test_constant_and_zero_rows_reference():
    """Constant rows give y = beta exactly, zero rows under RMS iv = rsqrt(eps); every
    reference value and error magnitude is finite."""
    for kind, dt, n2 in R.conditioning_cases():
        if kind.startswith("offset"):
            continue
        x, dy, gamma, beta = R.make_inputs(R.COND_N1, n2, dt, kind=kind)
        for rms in (False, True):
            r = _fwd_bwd(x, dy, gamma, None if rms else beta, n2=n2, rms=rms)
            for name, val in r.items():
                assert bool(torch.isfinite(val.v).all() and torch.isfinite(val.e).all()), name
            if not rms:
                assert torch.equal(r["y"].v, beta.to(F64).expand(R.COND_N1, n2))
            if kind == "zero" or not rms:   # zero variance: iv = rsqrt(eps)
                want = torch.tensor(R.f32(1e-5), dtype=F64).rsqrt()
                assert bool((r["invvar"].v == want).all())
