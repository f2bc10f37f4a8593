"""The LayerNorm / RMSNorm kernels (csrc/hip/layer_norm.hip) and the fused residual join
against the float64 references of tests/norm_ref.py, at every path the code takes: the
fast one-row-per-wave kernels at their lane-occupancy edges and grid limits, the generic
kernels (odd widths, widths above the fast limit, misaligned pointers, the part cap), all
four operators in every storage / parameter type, the saved statistics, ill-conditioned
rows, awkward layouts, partial gradients and the empty batch.

Every comparison is |got - ref| <= u_T*|ref| + tiny_T + K*eps32*S (optim_ref.bound) with
K measured on the reference alone (tests/test_norm_ref_cpu.py::test_k_measured).  Inputs
come from a seeded CPU generator; dy is drawn in fp32 and rounded to the type the kernel
reads, so the reference sees the same values."""
import pytest
import torch

import norm_ref as R
from norm_ref import BF16, F16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"


def L():
    from apex_example_amd import _native

    return _native.require().layer_norm


def _dev(t):
    return None if t is None else t.to(DEV)


def _name(dt):
    return {F32: "fp32", F16: "fp16", BF16: "bf16", None: "same"}[dt]


def _within(got, ref, what, shape=None):
    assert got is not None, what
    if shape is not None:
        ref = R._shaped(ref, shape)
    R.assert_within(got.detach().cpu(), ref, what, R.K)


def _op_run(x, dy, gamma, beta, n2, eps, rms, need_w=True, need_b=True):
    """forward + backward through the operators, as the autograd functions call them."""
    xg, dyg, gg, bg = _dev(x), _dev(dy), _dev(gamma), _dev(beta)
    y, mean, invvar = L().forward(xg, n2, gg, bg, eps, rms)
    dx, dgam, dbet = L().backward(dyg, xg, mean, invvar, n2, gg, need_w and gg is not None,
                                  need_b and gg is not None and not rms, rms)
    torch.cuda.synchronize()
    return {"y": y, "mean": mean, "invvar": invvar, "dx": dx, "dgamma": dgam, "dbeta": dbet}


def _compare(out, x, dy, gamma, beta, n2, eps, rms, tag, wshape=None):
    """``gamma`` / ``beta``: what the REFERENCE uses (None where the operator has none)."""
    fw = R.ref_forward(x, gamma, beta, n2, eps, rms)
    bw = R.ref_backward(dy, x, gamma, n2, eps, rms)
    n1 = x.numel() // n2
    assert out["y"].dtype == x.dtype and out["y"].shape == x.shape
    assert out["mean"].dtype == F32 and out["mean"].shape == (n1,)
    assert out["invvar"].dtype == F32 and out["invvar"].shape == (n1,)
    _within(out["y"], fw["y"], tag + " y")
    _within(out["mean"], fw["mean"], tag + " mean")
    if rms:
        assert bool((out["mean"] == 0).all()), tag + ": RMS mean is exactly 0"
    _within(out["invvar"], fw["invvar"], tag + " invvar")
    if out.get("dx") is not None:
        assert out["dx"].dtype == x.dtype
        _within(out["dx"], bw["dx"], tag + " dx")
    for name in ("dgamma", "dbeta"):
        if out.get(name) is not None:
            _within(out[name], bw[name], tag + " " + name, wshape or (n2,))
    return fw, bw


def _operator_run(n1, n2, dt, wdt, rms, affine, eps=1e-5, kind="randn", seed=0):
    """One operator through the ops: LayerNorm without affine parameters passes none,
    RMSNorm without them passes the ones weight its module builds and asks for no grad."""
    x, dy, gamma, beta = R.make_inputs(n1, n2, dt, wdt, seed=seed, kind=kind)
    if rms:
        beta = None
    if affine:
        out = _op_run(x, dy, gamma, beta, n2, eps, rms)
        assert out["dgamma"].dtype == gamma.dtype
        assert (out["dbeta"] is None) == rms
    else:
        ones = torch.ones(n2, dtype=dt) if rms else None
        out = _op_run(x, dy, ones, None, n2, eps, rms, need_w=False, need_b=False)
        assert out["dgamma"] is None and out["dbeta"] is None
        gamma = beta = None
    tag = "%s%s %s/%s (%d, %d)" % ("rms" if rms else "ln", "" if affine else "-noaffine",
                                   _name(dt), _name(wdt), n1, n2)
    _compare(out, x, dy, gamma, beta, n2, eps, rms, tag)
    return out, (x, dy, gamma, beta)


# ------------------------------------------------------------------------- shape sweep
@pytest.mark.parametrize("n1,n2", R.shapes(), ids=lambda v: str(v))
def test_shapes(n1, n2):
    """Every path-reaching shape with LayerNorm affine and RMSNorm affine in fp32 and bf16:
    one active lane (n2 = 8), a last 16-byte group held by lane 0 alone (520 / 1032 / 1544),
    idle waves (n1 < 4), more partial rows than ln_bwd_colsum has row lanes and its
    unrolled loop's tail, a second row per wave in the backward (4100) and in the forward
    (32772), odd / even-not-multiple-of-8 / too-wide generic widths, the short last part
    and the 512-part cap with empty trailing parts."""
    for dt in (F32, BF16):
        for rms in (False, True):
            _operator_run(n1, n2, dt, None, rms, True)


@pytest.mark.parametrize("n1,n2", R.COMBO_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("dt,wdt", R.TYPE_COMBOS, ids=_name)
@pytest.mark.parametrize("rms,affine", R.OPERATORS,
                         ids=["ln-affine", "ln-noaffine", "rms-affine", "rms-noaffine"])
def test_operators_and_types(rms, affine, dt, wdt, n1, n2):
    """Each operator / storage type / parameter type (x's own, or fp32 under 16-bit x - the
    T != TW instantiations) on a fast and a generic shape."""
    _operator_run(n1, n2, dt, wdt if affine else None, rms, affine, seed=1)


@pytest.mark.parametrize("n1,n2", R.COMBO_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("dt,wdt", R.TYPE_COMBOS, ids=_name)
@pytest.mark.parametrize("rms,affine", R.OPERATORS,
                         ids=["ln-affine", "ln-noaffine", "rms-affine", "rms-noaffine"])
def test_modules_and_functional(rms, affine, dt, wdt, n1, n2):
    """The same through autograd: the modules (parameters cast to x's type, or left fp32
    under 16-bit x) and, for mixed types, the functional entry points as well."""
    from apex_example_amd.normalization import FusedLayerNorm, FusedRMSNorm
    from apex_example_amd.normalization.fused_layer_norm import (fused_layer_norm_affine,
                                                                 fused_rms_norm_affine)

    eps = 1e-5
    x, dy, gamma, beta = R.make_inputs(n1, n2, dt, wdt if affine else None, seed=2)
    cls = FusedRMSNorm if rms else FusedLayerNorm
    m = cls(n2, eps=eps, elementwise_affine=affine).to(DEV)
    if affine:
        m = m.to(gamma.dtype)
        with torch.no_grad():
            m.weight.copy_(gamma)
            if not rms:
                m.bias.copy_(beta)
    xa = _dev(x).requires_grad_(True)
    y = m(xa)
    y.backward(_dev(dy))
    tag = "module %s%s %s/%s (%d, %d)" % ("rms" if rms else "ln", "" if affine else "-noaffine",
                                          _name(dt), _name(wdt), n1, n2)
    g_ref, b_ref = (gamma, None if rms else beta) if affine else (None, None)
    fw = R.ref_forward(x, g_ref, b_ref, n2, eps, rms)
    bw = R.ref_backward(dy, x, g_ref, n2, eps, rms)
    assert y.dtype == dt and xa.grad.dtype == dt
    _within(y, fw["y"], tag + " y")
    _within(xa.grad, bw["dx"], tag + " dx")
    if affine:
        assert m.weight.grad.dtype == gamma.dtype
        _within(m.weight.grad, bw["dgamma"], tag + " dgamma")
        if not rms:
            _within(m.bias.grad, bw["dbeta"], tag + " dbeta")
        # the functional entry points with the parameters as plain tensors
        xb, gb = _dev(x).requires_grad_(True), _dev(gamma).requires_grad_(True)
        if rms:
            yb = fused_rms_norm_affine(xb, gb, (n2,), eps)
        else:
            bb = _dev(beta).requires_grad_(True)
            yb = fused_layer_norm_affine(xb, gb, bb, (n2,), eps)
        yb.backward(_dev(dy))
        assert torch.equal(yb, y) and torch.equal(xb.grad, xa.grad)
        assert torch.equal(gb.grad, m.weight.grad)
        if not rms:
            assert torch.equal(bb.grad, m.bias.grad)


# ------------------------------------------------------------------------------ empty
@pytest.mark.parametrize("n2", [64, 777])
@pytest.mark.parametrize("dt,wdt", [(F32, None), (BF16, None), (BF16, F32)], ids=_name)
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
def test_empty_batch(rms, dt, wdt, n2):
    """n1 = 0: empty outputs, and parameter gradients of exact zeros (what torch returns) -
    not whatever the allocator handed over: buffers of the gradients' size are filled with
    a non-zero pattern and freed just before."""
    x, dy, gamma, beta = R.make_inputs(0, n2, dt, wdt)
    xg, dyg, gg = _dev(x), _dev(dy), _dev(gamma)
    bg = None if rms else _dev(beta)
    y, mean, invvar = L().forward(xg, n2, gg, bg, 1e-5, rms)
    assert y.shape == (0, n2) and y.dtype == dt
    assert mean.shape == (0,) and invvar.shape == (0,)
    junk = [torch.full((n2,), 7.0, dtype=gamma.dtype, device=DEV) for _ in range(4)]
    torch.cuda.synchronize()
    del junk
    dx, dgam, dbet = L().backward(dyg, xg, mean, invvar, n2, gg, True, not rms, rms)
    assert dx.shape == (0, n2) and dx.dtype == dt
    assert dgam.shape == (n2,) and dgam.dtype == gamma.dtype
    assert bool((dgam == 0).all()), "dgamma of an empty batch"
    if not rms:
        assert bool((dbet == 0).all()), "dbeta of an empty batch"


@pytest.mark.parametrize("dt,wdt", [(F32, None), (BF16, F32)], ids=_name)
def test_empty_batch_join(dt, wdt):
    n2 = 64
    x, dy, gamma, beta = R.make_inputs(0, n2, dt, wdt)
    xg, dyg, gg, bg = _dev(x), _dev(dy), _dev(gamma), _dev(beta)
    y, s, mean, invvar = L().add_dropout_forward(xg, xg.clone(), n2, gg, bg, 1e-5, 0.1, 5, False)
    assert y.shape == (0, n2) and s.shape == (0, n2) and mean.shape == (0,)
    junk = [torch.full((n2,), 7.0, dtype=gamma.dtype, device=DEV) for _ in range(6)]
    torch.cuda.synchronize()
    del junk
    ds, dh, dgam, dbet, dhs = L().add_dropout_backward(dyg, s, mean, invvar, n2, gg, None, 0.1, 5,
                                                       True, True, None, True)
    assert ds.shape == (0, n2) and dh.shape == (0, n2)
    for name, t in (("dgamma", dgam), ("dbeta", dbet), ("dhsum", dhs)):
        assert t.shape == (n2,) and bool((t == 0).all()), name + " of an empty batch"


# ------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("kind,dt,n2", R.conditioning_cases(),
                         ids=lambda v: v if isinstance(v, str) else (_name(v) if isinstance(
                             v, torch.dtype) else str(v)))
def test_conditioning(kind, dt, n2):
    """Offset rows (|mu| / sigma up to 1e5: a one-pass E[x^2] - mu^2 variance lands outside
    the bound of invvar, tests/test_norm_ref_cpu.py shows it on the same inputs), constant
    rows (y = beta) and zero rows (RMS: iv = rsqrt(eps)); everything finite."""
    for rms in (False, True):
        out, (x, dy, gamma, beta) = _operator_run(R.COND_N1, n2, dt, None, rms, True, kind=kind)
        for name, t in out.items():
            if t is not None:
                assert bool(torch.isfinite(t).all()), (name, rms)
        if kind == "const" and not rms and n2 == 1024:
            # 1024 * 0.5 and 1 / 1024 are exact: mu = 0.5, x - mu = 0, y = fma(0, g, b) = b
            assert torch.equal(out["y"].cpu(), beta.expand(R.COND_N1, n2))
            assert bool((out["mean"] == 0.5).all())


@pytest.mark.parametrize("eps", [1e-12, 0.1])
@pytest.mark.parametrize("n1,n2", R.COMBO_SHAPES, ids=lambda v: str(v))
def test_eps(n1, n2, eps):
    for dt in (F32, BF16):
        for rms in (False, True):
            _operator_run(n1, n2, dt, None, rms, True, eps=eps, seed=3)


# ----------------------------------------------------------------- pointers and layouts
def _offset_view(t, pad=1):
    """A contiguous view of ``t``'s values starting ``pad`` elements into a larger buffer
    (not 16-byte aligned), and the buffer."""
    buf = torch.full((t.numel() + 16,), 3.0, dtype=t.dtype, device=DEV)
    v = buf[pad:pad + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v, buf


@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
@pytest.mark.parametrize("which", ["x", "dy", "params"])
def test_misaligned_views(which, rms, dt):
    """A fast-path width on the generic kernels: x one element into a larger buffer (both
    directions generic), only dy misaligned (fast forward, generic backward), gamma / beta
    as offset views through the functional API.  The inputs stay bitwise unchanged."""
    from apex_example_amd.normalization.fused_layer_norm import (fused_layer_norm_affine,
                                                                 fused_rms_norm_affine)

    n1, n2, eps = 5, 1024, 1e-5
    x, dy, gamma, beta = R.make_inputs(n1, n2, dt, seed=4)
    xg, dyg, gg, bg = _dev(x), _dev(dy), _dev(gamma), _dev(beta)
    bufs = []
    if which == "x":
        xg, b = _offset_view(xg)
        bufs.append(b)
    elif which == "dy":
        dyg, b = _offset_view(dyg)
        bufs.append(b)
    else:
        gg, b1 = _offset_view(gg)
        bg, b2 = _offset_view(bg, pad=3)
        bufs += [b1, b2]
    before = [b.clone() for b in bufs]
    xa, ga = xg.requires_grad_(True), gg.requires_grad_(True)
    if rms:
        y = fused_rms_norm_affine(xa, ga, (n2,), eps)
    else:
        ba = bg.requires_grad_(True)
        y = fused_layer_norm_affine(xa, ga, ba, (n2,), eps)
    y.backward(dyg)
    torch.cuda.synchronize()
    for b, b0 in zip(bufs, before):
        assert torch.equal(b, b0), "input buffer modified"
    assert torch.equal(xg.detach().cpu(), x) and torch.equal(dyg.cpu(), dy)
    tag = "misaligned %s %s %s" % (which, "rms" if rms else "ln", _name(dt))
    fw = R.ref_forward(x, gamma, None if rms else beta, n2, eps, rms)
    bw = R.ref_backward(dy, x, gamma, n2, eps, rms)
    _within(y, fw["y"], tag + " y")
    _within(xa.grad, bw["dx"], tag + " dx")
    _within(ga.grad, bw["dgamma"], tag + " dgamma")
    if not rms:
        _within(ba.grad, bw["dbeta"], tag + " dbeta")
    # the statistics of the misaligned forward, through the operator
    _, mean, invvar = L().forward(xg.detach(), n2, gg.detach(), None if rms else bg.detach(), eps,
                                  rms)
    _within(mean, fw["mean"], tag + " mean")
    _within(invvar, fw["invvar"], tag + " invvar")


@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("n1,n2", R.COMBO_SHAPES, ids=lambda v: str(v))
def test_noncontiguous_x_and_stride0_dy(n1, n2, dt):
    """x a transposed view; dy the stride-0 expansion y.sum().backward() hands over."""
    from apex_example_amd.normalization import FusedLayerNorm, FusedRMSNorm

    eps = 1e-5
    xt, _, gamma, beta = R.make_inputs(n2, n1, dt, seed=5, shape=(n2, n1))
    gamma, beta = R.make_inputs(n1, n2, dt, seed=5)[2:]
    x = xt.t().contiguous()     # the values the kernel must see, row-major [n1, n2]
    dy = torch.ones(n1, n2, dtype=dt)
    for rms in (False, True):
        m = (FusedRMSNorm if rms else FusedLayerNorm)(n2, eps=eps).to(DEV).to(dt)
        with torch.no_grad():
            m.weight.copy_(gamma)
            if not rms:
                m.bias.copy_(beta)
        xa = _dev(xt).requires_grad_(True)
        xv = xa.t()
        assert not xv.is_contiguous()
        y = m(xv)
        y.sum().backward()
        tag = "transposed x / stride-0 dy %s %s (%d, %d)" % ("rms" if rms else "ln", _name(dt), n1,
                                                             n2)
        fw = R.ref_forward(x, gamma, None if rms else beta, n2, eps, rms)
        bw = R.ref_backward(dy, x, gamma, n2, eps, rms)
        _within(y, fw["y"], tag + " y")
        assert xa.grad.shape == (n2, n1)
        _within(xa.grad.t(), bw["dx"], tag + " dx")
        _within(m.weight.grad, bw["dgamma"], tag + " dgamma")
        if not rms:
            _within(m.bias.grad, bw["dbeta"], tag + " dbeta")


@pytest.mark.parametrize("dt,wdt", [(F32, None), (BF16, None), (BF16, F32)], ids=_name)
@pytest.mark.parametrize("shape,nshape", [((3, 4, 256), (4, 256)), ((2, 7, 3, 5), (3, 5))],
                         ids=["fast", "generic"])
def test_multi_dim_normalized_shape(shape, nshape, dt, wdt):
    """normalized_shape of two dimensions over a 3-D / 4-D input: the parameter gradients
    have the parameter's shape."""
    from apex_example_amd.normalization import FusedLayerNorm, FusedRMSNorm

    eps = 1e-5
    n2 = nshape[0] * nshape[1]
    n1 = 1
    for s in shape:
        n1 *= s
    n1 //= n2
    x, dy, gamma, beta = R.make_inputs(n1, n2, dt, wdt, seed=6, shape=shape)
    for rms in (False, True):
        m = (FusedRMSNorm if rms else FusedLayerNorm)(nshape, eps=eps).to(DEV).to(gamma.dtype)
        with torch.no_grad():
            m.weight.copy_(gamma.reshape(nshape))
            if not rms:
                m.bias.copy_(beta.reshape(nshape))
        xa = _dev(x).requires_grad_(True)
        y = m(xa)
        y.backward(_dev(dy))
        tag = "normalized_shape %s %s %s/%s" % (nshape, "rms" if rms else "ln", _name(dt),
                                                _name(wdt))
        fw = R.ref_forward(x, gamma, None if rms else beta, n2, eps, rms)
        bw = R.ref_backward(dy, x, gamma, n2, eps, rms)
        assert y.shape == x.shape and xa.grad.shape == x.shape
        _within(y, fw["y"], tag + " y")
        _within(xa.grad, bw["dx"], tag + " dx")
        assert m.weight.grad.shape == tuple(nshape)
        _within(m.weight.grad, bw["dgamma"], tag + " dgamma", nshape)
        if not rms:
            assert m.bias.grad.shape == tuple(nshape)
            _within(m.bias.grad, bw["dbeta"], tag + " dbeta", nshape)


@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("n1,n2", R.COMBO_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("need", [(True, False, True), (True, True, False), (True, False, False),
                                  (False, True, True)],
                         ids=["w-frozen", "b-frozen", "x-only", "params-only"])
def test_partial_needs_input_grad(need, n1, n2, dt):
    """(x, weight, bias) requiring grad in part: a frozen parameter gets None, the others
    still match the reference (dbeta without dgamma and the reverse; dx alone: no partial
    sums, no dynamic LDS)."""
    from apex_example_amd.normalization import FusedLayerNorm, FusedRMSNorm

    eps = 1e-5
    nx, nw, nb = need
    x, dy, gamma, beta = R.make_inputs(n1, n2, dt, seed=7)
    for rms in (False, True):
        if rms and nw != nb:
            continue        # no bias: the two-parameter combinations are LayerNorm's
        m = (FusedRMSNorm if rms else FusedLayerNorm)(n2, eps=eps).to(DEV).to(dt)
        with torch.no_grad():
            m.weight.copy_(gamma)
            if not rms:
                m.bias.copy_(beta)
        m.weight.requires_grad_(nw)
        if not rms:
            m.bias.requires_grad_(nb)
        xa = _dev(x).requires_grad_(nx)
        y = m(xa)
        y.backward(_dev(dy))
        tag = "needs %s %s %s (%d, %d)" % (need, "rms" if rms else "ln", _name(dt), n1, n2)
        bw = R.ref_backward(dy, x, gamma, n2, eps, rms)
        if nx:
            _within(xa.grad, bw["dx"], tag + " dx")
        else:
            assert xa.grad is None
        if nw:
            _within(m.weight.grad, bw["dgamma"], tag + " dgamma")
        else:
            assert m.weight.grad is None
        if not rms:
            if nb:
                _within(m.bias.grad, bw["dbeta"], tag + " dbeta")
            else:
                assert m.bias.grad is None


# ------------------------------------------------------ determinism, the one-row switch
@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("n1,n2", [(37, 1024), (37, 2048), (33, 777), (4100, 64)],
                         ids=lambda v: str(v))
def test_backward_deterministic(n1, n2, dt):
    x, dy, gamma, beta = R.make_inputs(n1, n2, dt, seed=8)
    a = _op_run(x, dy, gamma, beta, n2, 1e-5, False)
    b = _op_run(x, dy, gamma, beta, n2, 1e-5, False)
    for name in ("y", "mean", "invvar", "dx", "dgamma", "dbeta"):
        assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("n2", [1024, 2048])
def test_one_row_combine_bitwise_plain_backward(n2, dt):
    """layer_norm.set_bwd_one_row(1) in the plain (non-fused) backward: one [2][n2] LDS row
    set with the waves adding in turn, in the per-wave rows' order - bitwise equal to the
    default, which at n2 = 2048 uses exactly 64 KB of dynamic LDS.  Both match the
    reference."""
    n1 = 37
    x, dy, gamma, beta = R.make_inputs(n1, n2, dt, seed=9)

    def run(one):
        L().set_bwd_one_row(one)
        try:
            assert L().bwd_one_row() == bool(one)
            return _op_run(x, dy, gamma, beta, n2, 1e-5, False)
        finally:
            L().set_bwd_one_row(0)

    a, b = run(0), run(1)
    assert not L().bwd_one_row()
    for name in ("dx", "dgamma", "dbeta"):
        assert torch.equal(a[name], b[name]), name
    _compare(b, x, dy, gamma, beta, n2, 1e-5, False, "one-row %s n2=%d" % (_name(dt), n2))


# --------------------------------------------------------------- fused residual join
def _hsum_ok(n2):
    # a third [4 waves][n2] fp32 LDS row within 64 KB (layer_norm_bwd_hsum_ok)
    return 4 * 3 * n2 * 4 <= 65536


def _recover_keep(shape, dt, n2, p, seed):
    """The keep mask of (seed, p): replay with x = 0, h = 1, so that s = keep * scale."""
    z = torch.zeros(shape, dtype=dt, device=DEV)
    _, m, _, _ = L().add_dropout_forward(z, torch.ones_like(z), n2, None, None, 1e-5, p, seed,
                                         False)
    keep = (m != 0).float().cpu()
    if p == 0.0:
        assert bool((keep == 1).all())
    return keep


@pytest.mark.parametrize("i", range(len(R.JOIN_SHAPES)),
                         ids=["%dx%d" % s for s in R.JOIN_SHAPES])
def test_join_corners(i):
    """bf16 x / h with fp32 parameters (the existing join tests cast the module) at one
    active lane, a lane-0-only last group and the widest row, 3 rows and more rows than
    the backward grid holds, p in 0 / 0.1 / 0.9: s, y, mean, invvar, ds, dh, dgamma, dbeta
    and - where the third LDS row fits - dhsum, read through the operators."""
    n1, n2 = R.JOIN_SHAPES[i]
    p, seed, eps = R.JOIN_P[i % 3], 1234 + i, 1e-5
    x, h, _, dy, de, gamma, beta = R.make_join_inputs(n1, n2, BF16, F32, p)
    keep = _recover_keep((n1, n2), BF16, n2, p, seed)
    if p > 0:
        frac = float(keep.mean())
        assert abs(frac - (1 - p)) < 0.02 + 3 / (n1 * n2) ** 0.5, frac
    xg, hg, gg, bg = _dev(x), _dev(h), _dev(gamma), _dev(beta)
    y, s, mean, invvar = L().add_dropout_forward(xg, hg, n2, gg, bg, eps, p, seed, False)
    ds, dh, dgam, dbet, dhs = L().add_dropout_backward(_dev(dy), s, mean, invvar, n2, gg,
                                                       _dev(de), p, seed, True, True, None, True)
    torch.cuda.synchronize()
    tag = "join (%d, %d) p=%g" % (n1, n2, p)
    fw = R.ref_join_forward(x, h, keep, p, gamma, beta, n2, eps, s_stored=s.cpu())
    assert s.dtype == BF16 and y.dtype == BF16 and dh.dtype == BF16 and dgam.dtype == F32
    _within(s, fw["s"], tag + " s")
    _within(y, fw["y"], tag + " y")
    _within(mean, fw["mean"], tag + " mean")
    _within(invvar, fw["invvar"], tag + " invvar")
    bw = R.ref_join_backward(dy, de, s.cpu(), keep, p, gamma, n2, eps, dh_stored=dh.cpu())
    _within(ds, bw["ds"], tag + " ds")
    _within(dh, bw["dh"], tag + " dh")
    _within(dgam, bw["dgamma"], tag + " dgamma")
    _within(dbet, bw["dbeta"], tag + " dbeta")
    if _hsum_ok(n2):
        assert dhs is not None and dhs.dtype == F32
        _within(dhs, bw["dhsum"], tag + " dhsum")
    else:
        assert dhs is None
    assert bool((dh.cpu().float()[keep == 0] == 0).all())


@pytest.mark.parametrize("use", ["s", "y"])
@pytest.mark.parametrize("n1,n2,p", [(3, 520, 0.1), (5, 8, 0.9), (3, 2048, 0.0)])
def test_join_one_output_consumed(n1, n2, p, use):
    """Only s consumed (dy is None: ds = ds_ext exactly, dgamma = dbeta = 0) and only y
    consumed (ds_ext is None), through the autograd function."""
    from apex_example_amd.normalization.fused_layer_norm import AddDropoutLayerNormFunction

    eps = 1e-5
    x, h, _, dy, de, gamma, beta = R.make_join_inputs(n1, n2, BF16, F32, p, seed=1)
    xa, ha = _dev(x).requires_grad_(True), _dev(h).requires_grad_(True)
    ga, ba = _dev(gamma).requires_grad_(True), _dev(beta).requires_grad_(True)
    torch.manual_seed(11)
    y, s = AddDropoutLayerNormFunction.apply(xa, ha, ga, ba, (n2,), eps, p)
    with torch.no_grad():
        torch.manual_seed(11)
        z = torch.zeros_like(xa)
        _, m = AddDropoutLayerNormFunction.apply(z, torch.ones_like(z), ga, ba, (n2,), eps, p)
    keep = (m != 0).float().cpu()
    if use == "s":
        s.backward(_dev(de))
        dy_, de_ = None, de
    else:
        y.backward(_dev(dy))
        dy_, de_ = dy, None
    tag = "join %s only (%d, %d) p=%g" % (use, n1, n2, p)
    fw = R.ref_join_forward(x, h, keep, p, gamma, beta, n2, eps, s_stored=s.detach().cpu())
    _within(s, fw["s"], tag + " s")
    _within(y, fw["y"], tag + " y")
    bw = R.ref_join_backward(dy_, de_, s.detach().cpu(), keep, p, gamma, n2, eps,
                             dh_stored=ha.grad.cpu())
    _within(xa.grad, bw["ds"], tag + " ds")
    _within(ha.grad, bw["dh"], tag + " dh")
    _within(ga.grad, bw["dgamma"], tag + " dgamma")
    _within(ba.grad, bw["dbeta"], tag + " dbeta")
    if use == "s":
        assert torch.equal(xa.grad.cpu(), de)
        assert bool((ga.grad == 0).all()) and bool((ba.grad == 0).all())
