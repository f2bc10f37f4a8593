"""The BatchNorm kernels (csrc/hip/batch_norm.hip, bn_nhwc.hip, csrc/include/bn_common.h)
against the float64 references of tests/bn_ref.py, at every path the launchers take: the
NHWC scalar and vector paths at their lane / row-group / channel-block edges, the reduction
splits (ragged, empty), the NCHW scalar / vector / split / grid-stride paths, 2-D to 5-D
inputs, every storage and parameter type, every ReLU mode with the mask bits themselves,
the gradient targets, the SyncBN pieces on one GPU, the slab finalizes on synthetic slabs,
the fused two-BN forms, and the modules' options through autograd.

Every comparison is |got - ref| <= u_T*|ref| + tiny_T + K*eps32*S (optim_ref.bound) with K
measured on the reference alone (tests/test_bn_ref_cpu.py::test_k_measured), and the
condition each shape is listed for is asserted there by the geometry mirror.  The ops of
``_native.require().bn`` are called directly, as the autograd function calls them; the
backward ops are fed the device's own saved mean / invstd while the reference recomputes
its own.  Every op runs twice on the same inputs and must return identical bits.  ReLU
inputs have no ambiguous element (bn_ref.make_inputs), so the mask, y > 0 and the
backward's d are compared everywhere."""
import pytest
import torch

import bn_ref as R
from bn_ref import BF16, F16, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}


def B():
    from apex_example_amd import _native

    return _native.require().bn


def _name(v):
    return {F32: "fp32", F16: "fp16", BF16: "bf16"}.get(v, str(v))


def _case_id(c):
    return "%s-%s%s%s" % ("x".join(map(str, c.shape)), c.layout, "-off" if c.offset else "",
                          "-tuned" if c.tune else "")


@pytest.fixture(autouse=True)
def _tuning():
    """The tuning is process-global: every test starts from the mirrored defaults (which
    the geometry mirror's claims rest on) and leaves them behind."""
    C = B()
    assert list(C.get_tuning()) == [R.DEFAULT_TUNING[k] for k in R.TUNING_KEYS]
    try:
        yield
    finally:
        C.set_tuning(**R.DEFAULT_TUNING)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst |err| / bound per output over the run:")
    for k in sorted(WORST):
        print("  WORST %-36s %.3f" % (k, WORST[k]))


def _within(got, ref, name, tag):
    assert got is not None, (name, tag)
    g = got.detach().cpu()
    if g.shape != ref.v.shape:
        assert g.numel() == ref.v.numel(), (name, tag, g.shape, ref.v.shape)
        g = g.reshape(ref.v.shape)
    r = R.worst_ratio(g, ref, R.K)
    key = "%s [%s]" % (name.split(".fp32")[0].split(".bf16")[0].split(".fp16")[0],
                       _name(got.dtype))
    WORST[key] = max(WORST.get(key, 0.0), r)
    print("%-60s worst |err| / bound = %.3f" % (tag + " " + name, r))
    assert r <= 1.0, "%s %s: |err| / bound = %g" % (tag, name, r)


def _same(a, b, what):
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (p, q) in enumerate(zip(a, b)):
            _same(p, q, "%s[%d]" % (what, i))
    elif a is None or b is None:
        assert a is None and b is None, what
    else:
        assert a.dtype == b.dtype and torch.equal(a, b), what + ": not bitwise reproducible"


def twice(fn, what):
    """Determinism: the op twice on the same inputs, identical bits."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    _same(a, b, what)
    return a


def _place(t, c, offset=None):
    """A CPU [N, C, *] tensor on the device as case ``c`` stores it: channels-last for a 4-D
    NHWC case, and ``offset`` elements into its storage (a contiguous, misaligned view)."""
    if t is None:
        return None
    off = c.offset if offset is None else offset
    cl4 = c.layout == "nhwc" and t.dim() == 4
    if not off:
        t = t.to(DEV)
        return t.contiguous(memory_format=torch.channels_last) if cl4 else t.contiguous()
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    if cl4:
        n, ch, h, w = t.shape
        v = buf[off:].view(n, h, w, ch).permute(0, 3, 1, 2)
    else:
        v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.storage_offset() == off
    return v


def _dev(t):
    return None if t is None else t.to(DEV)


def _cl4(c):
    return c.layout == "nhwc" and len(c.shape) == 4


def _mask_expected(c, relu, want_mask):
    """norm_ops.cpp relu_mask_ok: the NHWC vector path (C % 8 == 0, aligned) only."""
    cl, _, C, _ = R.view(c.shape, _cl4(c))
    return bool(want_mask and relu and cl and C % 8 == 0 and not c.offset)


class Run:
    """One case on the device: inputs, the reference, forward and backward results."""


def run_case(c, dt, wdt, mode, kind="randn", affine=True, seed=0):
    C = B()
    relu, residual, want_mask = R.MODES[mode]
    tune = c.tune or R.DEFAULT_TUNING
    inp = R.make_inputs(c.shape, dt, wdt, c.layout, kind, relu, residual, seed, tune=c.tune,
                        affine=affine)
    chain = R.red_chain(c.shape, _cl4(c), tune)
    ref, mask = R.ref_all(inp["x"], inp["dy"], inp["z"], inp["weight"], inp["bias"],
                          inp["running_mean"], inp["running_var"], chain=chain, relu=relu)
    if c.tune:
        C.set_tuning(**c.tune)
    tag = "%s %s/%s %s %s" % (_case_id(c), _name(dt), _name(wdt), mode, kind)
    x, dy, z = _place(inp["x"], c), _place(inp["dy"], c), _place(inp["z"], c)
    w, b = _dev(inp["weight"]), _dev(inp["bias"])
    n = x.numel() // x.shape[1]
    Cn = x.shape[1]

    def fwd():
        rm, rv = _dev(inp["running_mean"]), _dev(inp["running_var"])
        nbt = torch.tensor(3, dtype=torch.int64, device=DEV)
        y, mean, invstd, m = C.forward_local(x, w, b, rm, rv, nbt, R.EPS, R.MOMENTUM, z, relu,
                                             want_mask)
        return y, mean, invstd, m, rm, rv, nbt

    y, mean, invstd, m, rm, rv, nbt = twice(fwd, tag + " forward_local")
    assert y.dtype == dt and y.shape == x.shape and mean.dtype == F32 and invstd.dtype == F32
    assert mean.shape == (Cn,) and invstd.shape == (Cn,)
    _within(mean, ref["mean"], "mean", tag)
    _within(invstd, ref["invstd"], "invstd", tag)
    _within(rm, ref["running_mean"], "running_mean", tag)
    _within(rv, ref["running_var"], "running_var", tag)
    assert int(nbt) == 4, "num_batches_tracked goes up by exactly one per call"
    _within(y, ref["y"], "y", tag)
    if relu:
        assert torch.equal(y.cpu() > 0, mask), tag + ": y > 0 is not o_ref > 0"
    if _mask_expected(c, relu, want_mask):
        assert m is not None and m.dtype == torch.uint8 and m.shape == (n, Cn // 8)
        assert torch.equal(m.cpu(), R.mask_bytes(mask)), tag + ": ReLU mask bits"
    else:
        assert m is None, tag + ": a mask outside relu_mask_ok"

    # the same statistics from the stats-only ops, and without running stats / counter
    def stats():
        rm2, rv2 = _dev(inp["running_mean"]), _dev(inp["running_var"])
        nbt2 = torch.tensor(3, dtype=torch.int64, device=DEV)
        return C.train_stats(x, rm2, rv2, nbt2, R.EPS, R.MOMENTUM) + (rm2, rv2, nbt2)

    _same(twice(stats, tag + " train_stats"), (mean, invstd, rm, rv, nbt), tag + " train_stats")
    mean_l, var_l = twice(lambda: C.local_stats(x), tag + " local_stats")
    _within(mean_l, ref["mean"], "mean", tag + " local_stats")
    _within(var_l, ref["var"], "var", tag + " local_stats")
    bare = C.forward_local(x, w, b, None, None, None, R.EPS, R.MOMENTUM, z, relu, want_mask)
    _same(bare, (y, mean, invstd, m), tag + " forward_local without running stats")
    ya = twice(lambda: C.apply(x, mean, invstd, w, b, z, relu), tag + " apply")
    _same(ya, y, tag + " apply")

    # backward, from the device's own saved statistics
    zb = z if m is None else None

    def red():
        return C.reduce_grad(dy, x, mean, invstd, w, b, zb, relu, True, mask=m)

    sdy, sdx, gw, gb = twice(red, tag + " reduce_grad")
    _within(sdy, ref["sum_dy"], "sum_dy", tag)
    _within(sdx, ref["sum_dy_xmu"], "sum_dy_xmu", tag)
    assert sdy.dtype == F32 and sdx.dtype == F32
    if affine:
        assert gw.dtype == w.dtype and gb.dtype == w.dtype
        _within(gw, ref["dgamma"], "dgamma." + _name(gw.dtype), tag)
        _within(gb, ref["dbeta"], "dbeta." + _name(gb.dtype), tag)
    else:
        assert gw is None and gb is None

    def elem():
        return C.backward_elemt(dy, x, mean, invstd, w, b, sdy, sdx, float(n), zb, relu,
                                residual, mask=m)

    dx, dz = twice(elem, tag + " backward_elemt")
    assert dx.dtype == dt and dx.shape == x.shape
    _within(dx, ref["dx"], "dx", tag)
    if residual:
        assert dz.dtype == dt
        _within(dz, ref["dz"], "dz", tag)
    else:
        assert dz is None

    def local():
        return C.backward_local(dy, x, mean, invstd, w, b, zb, relu, True, residual, mask=m)

    _same(twice(local, tag + " backward_local"), (dx, dz, gw, gb), tag + " backward_local")
    r = Run()
    r.__dict__.update(inp=inp, ref=ref, mask=mask, x=x, dy=dy, z=z, zb=zb, w=w, b=b, n=n,
                      mean=mean, invstd=invstd, m=m, y=y, dx=dx, dz=dz, sdy=sdy, sdx=sdx,
                      gw=gw, gb=gb, chain=chain, tag=tag, relu=relu, residual=residual)
    return r


# ------------------------------------------------------------------------- shape sweeps
def test_tuning_is_the_mirrored_default():
    assert list(B().get_tuning()) == [R.DEFAULT_TUNING[k] for k in R.TUNING_KEYS]


@pytest.mark.parametrize("c", R.NHWC_CASES, ids=_case_id)
def test_nhwc_shapes(c):
    """Every NHWC path-reaching shape (bn_ref.NHWC_CASES names the condition) in fp32 and
    bf16 under every ReLU mode: none, ReLU (RM 3), ReLU + z recomputed (RM 2) and ReLU + z
    from the mask (RM 1 where the vector path writes one, else RM 2 and no mask)."""
    for dt in (F32, BF16):
        for mode in R.MODES:
            run_case(c, dt, F32, mode)


@pytest.mark.parametrize("c", R.NCHW_CASES, ids=_case_id)
def test_nchw_shapes(c):
    """The NCHW kernels: scalar and vector, misaligned, more than one reduction split with
    boundaries inside a sample, 3-D and 5-D inputs; [N, C, 1, 1] takes the NHWC kernels.
    No mask is ever returned for an NCHW tensor."""
    for dt in (F32, BF16):
        for mode in R.MODES:
            run_case(c, dt, F32, mode)


def test_nchw_grid_stride():
    """More than 8192 * 256 scalar elements: the elementwise grid-stride loops run twice."""
    run_case(R.NCHW_BIG, F32, F32, "none")
    run_case(R.NCHW_BIG, BF16, F32, "relu_z")
    run_case(R.NCHW_BIG, BF16, BF16, "relu")


@pytest.mark.parametrize("c", R.TUNED_CASES, ids=lambda c: _case_id(c) + "-" + c.reaches[-1])
def test_loop_edges_through_tuning(c):
    """bn.set_tuning reaches the loop edges at small shapes: all rows in one split, one
    block grid-striding over every row, the per-shape elem_rpt rule, one row group per
    split.  The same bound under every tuning."""
    for dt in (F32, BF16):
        for mode in ("none", "relu", "relu_z_mask"):
            run_case(c, dt, F32, mode)


@pytest.mark.parametrize("kind,dt,c", R.KIND_CASES,
                         ids=lambda v: v if isinstance(v, str) else
                         _name(v) if isinstance(v, torch.dtype) else _case_id(v))
def test_input_kinds(kind, dt, c):
    """Large mean (mean / sigma = 1e5 in fp32), first element an outlier at 100 sigma,
    a constant channel (var = 0), a channel all-negative under ReLU (mask all zero)."""
    if kind == "allneg":
        r = run_case(c, dt, F32, "relu_z_mask", kind=kind)
        ch = 1 % c.shape[1]
        assert not bool(r.mask[:, ch].any()) and not bool((r.y[:, ch] != 0).any())
        assert not bool((r.dx[:, ch] != 0).any()) and not bool((r.dz[:, ch] != 0).any())
    else:
        r = run_case(c, dt, F32, "none", kind=kind)
        run_case(c, dt, F32, "relu_z", kind=kind)
        if kind == "const":
            assert float(r.invstd[0]) == pytest.approx(R.EPS ** -0.5, rel=1e-6)
            assert float(r.mean[0]) == 0.5


# ------------------------------------------------------------------------- types, options
@pytest.mark.parametrize("c", R.OPTION_CASES, ids=_case_id)
@pytest.mark.parametrize("dt,wdt", R.TYPE_COMBOS, ids=_name)
def test_types(c, dt, wdt):
    """T in fp32 / fp16 / bf16, TW in {fp32, T}, and no weight / bias at all."""
    run_case(c, dt, wdt, "relu_z_mask", seed=1)
    run_case(c, dt, wdt, "relu", seed=1)
    run_case(c, dt, wdt, "relu_z_mask", affine=False, seed=1)
    run_case(c, dt, wdt, "none", affine=False, seed=1)


@pytest.mark.parametrize("c", R.OPTION_CASES, ids=_case_id)
@pytest.mark.parametrize("dt,wdt", [(F32, F32), (BF16, F32), (BF16, BF16)], ids=_name)
def test_backward_options(c, dt, wdt):
    """need_wgrad false, want_dz false, the grad_weight / grad_bias targets with accumulate
    true (added to known contents) and false (overwritten), sum_scale as a device scalar."""
    C = B()
    r = run_case(c, dt, wdt, "relu_z_mask", seed=2)
    a = (r.dy, r.x, r.mean, r.invstd, r.w, r.b, r.zb, r.relu)
    Cn = r.x.shape[1]
    s1, s2, gw, gb = twice(lambda: C.reduce_grad(*a, False, mask=r.m), r.tag + " no wgrad")
    assert gw is None and gb is None
    _same((s1, s2), (r.sdy, r.sdx), r.tag + " need_wgrad=False sums")
    dx, dz, gw, gb = C.backward_local(*a, False, False, mask=r.m)
    assert dz is None and gw is None and gb is None
    _same(dx, r.dx, r.tag + " want_dz=False dx")
    dx, dz = C.backward_elemt(r.dy, r.x, r.mean, r.invstd, r.w, r.b, r.sdy, r.sdx, float(r.n),
                              r.zb, r.relu, False, mask=r.m)
    assert dz is None
    _same(dx, r.dx, r.tag + " backward_elemt want_dz=False dx")

    g = torch.Generator().manual_seed(5)
    gw0 = torch.randn(Cn, generator=g).to(wdt)
    gb0 = torch.randn(Cn, generator=g).to(wdt)
    ref = R.ref_backward(r.inp["dy"], r.inp["x"], r.mask, r.ref["mean"], r.ref["invstd"],
                         r.inp["weight"], r.chain, gw0=gw0, gb0=gb0)

    def acc(on):
        tw, tb = gw0.to(DEV), gb0.to(DEV)
        out = C.reduce_grad(*a, True, mask=r.m, grad_weight=tw, grad_bias=tb, accumulate=on)
        assert out[2].data_ptr() == tw.data_ptr() and out[3].data_ptr() == tb.data_ptr()
        return out

    _, _, gw, gb = twice(lambda: acc(True), r.tag + " accumulate")
    _within(gw, ref["dgamma"], "dgamma.accumulate." + _name(wdt), r.tag)
    _within(gb, ref["dbeta"], "dbeta.accumulate." + _name(wdt), r.tag)
    _, _, gw, gb = twice(lambda: acc(False), r.tag + " overwrite")
    _same((gw, gb), (r.gw, r.gb), r.tag + " accumulate=False overwrites the targets")

    sc = torch.tensor([1.0 / r.n], dtype=F32)
    ref = R.ref_backward(r.inp["dy"], r.inp["x"], r.mask, r.ref["mean"], r.ref["invstd"],
                         r.inp["weight"], r.chain, sum_scale=sc)
    scd = sc.to(DEV)
    s1, s2, gw, gb = twice(lambda: C.reduce_grad(*a, True, mask=r.m, sum_scale=scd),
                           r.tag + " sum_scale")
    _within(s1, ref["sum_dy"], "sum_dy.scaled", r.tag)
    _within(s2, ref["sum_dy_xmu"], "sum_dy_xmu.scaled", r.tag)
    # one [2C] buffer: SyncBN all-reduces (sum_dy | sum_dy_xmu) in place
    assert s2.data_ptr() == s1.data_ptr() + 4 * Cn
    _same((gw, gb), (r.gw, r.gb), r.tag + " dgamma / dbeta stay local sums")
    dx, dz = C.backward_elemt(r.dy, r.x, r.mean, r.invstd, r.w, r.b, s1, s2, 1.0, r.zb, r.relu,
                              True, mask=r.m)
    _within(dx, ref["dx"], "dx.scaled", r.tag)
    _same(dz, r.dz, r.tag + " dz")


@pytest.mark.parametrize("c", [R.OPTION_CASES[0], R.NHWC_CASES[-1]], ids=_case_id)
@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
def test_mask_written_by_vector_apply_read_by_scalar_backward(c, dt):
    """A vectorised apply wrote the mask; a misaligned dy sends reduce / backward down the
    scalar path, which finds its bit as byte [row][c / 8], bit c & 7."""
    C = B()
    r = run_case(c, dt, F32, "relu_z_mask", seed=3)
    assert r.m is not None
    dy = _place(r.inp["dy"], c, offset=1)
    a = (dy, r.x, r.mean, r.invstd, r.w, r.b, None, True)
    s1, s2, gw, gb = twice(lambda: C.reduce_grad(*a, True, mask=r.m), r.tag + " scalar reduce")
    tag = r.tag + " misaligned dy"
    _within(s1, r.ref["sum_dy"], "sum_dy", tag)
    _within(s2, r.ref["sum_dy_xmu"], "sum_dy_xmu", tag)
    _within(gw, r.ref["dgamma"], "dgamma.fp32", tag)
    _within(gb, r.ref["dbeta"], "dbeta.fp32", tag)
    dx, dz = twice(lambda: C.backward_elemt(dy, r.x, r.mean, r.invstd, r.w, r.b, s1, s2,
                                            float(r.n), None, True, True, mask=r.m),
                   tag + " backward_elemt")
    _within(dx, r.ref["dx"], "dx", tag)
    _within(dz, r.ref["dz"], "dz", tag)


@pytest.mark.parametrize("c", R.OPTION_CASES + [R.NHWC_CASES[-1], R.NCHW_CASES[5]], ids=_case_id)
@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
def test_apply_with_given_statistics(c, dt):
    """apply / apply_mask with statistics that are not those of x (given exactly)."""
    C = B()
    inp = R.make_inputs(c.shape, dt, F32, c.layout, residual=True, seed=4)
    g = torch.Generator().manual_seed(9)
    Cn = c.shape[1]
    mean = torch.randn(Cn, generator=g) * 0.3
    invstd = torch.rand(Cn, generator=g) + 0.5
    x, z = _place(inp["x"], c), _place(inp["z"], c)
    for zz, zd in ((None, None), (inp["z"], z)):
        ref = R.ref_apply(inp["x"], mean, invstd, inp["weight"], inp["bias"], zz, False)
        y = twice(lambda: C.apply(x, mean.to(DEV), invstd.to(DEV), _dev(inp["weight"]),
                                  _dev(inp["bias"]), zd, False), "apply")
        _within(y, ref["y"], "y.given_stats", _case_id(c) + " " + _name(dt))
        y2, m = C.apply_mask(x, mean.to(DEV), invstd.to(DEV), _dev(inp["weight"]),
                             _dev(inp["bias"]), zd, False)
        assert m is None, "no mask without ReLU"
        _same(y2, y, "apply_mask")


# ------------------------------------------------------------------------- SyncBN pieces
@pytest.mark.parametrize("c", R.OPTION_CASES + [R.NHWC_CASES[0]], ids=_case_id)
@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
def test_local_stats_packed(c, dt):
    """[mean | var | count] in one buffer; with ``out=`` into a slot in the middle of a
    larger buffer whose neighbours stay untouched."""
    C = B()
    inp = R.make_inputs(c.shape, dt, F32, c.layout, seed=6)
    ref = R.ref_stats(inp["x"], R.EPS, R.red_chain(c.shape, _cl4(c)))
    x = _place(inp["x"], c)
    Cn, n = x.shape[1], x.numel() // x.shape[1]
    packed = twice(lambda: C.local_stats_packed(x), "local_stats_packed")
    assert packed.shape == (2 * Cn + 1,) and packed.dtype == F32
    tag = _case_id(c) + " " + _name(dt) + " packed"
    _within(packed[:Cn], ref["mean"], "mean", tag)
    _within(packed[Cn:2 * Cn], ref["var"], "var", tag)
    assert float(packed[2 * Cn]) == float(n)
    w = 2 * Cn + 1
    buf = torch.full((3 * w,), -7.0, device=DEV)
    out = C.local_stats_packed(x, out=buf[w:2 * w])
    assert out.data_ptr() == buf[w:2 * w].data_ptr()
    _same(buf[w:2 * w], packed, tag + " out= slot")
    assert bool((buf[:w] == -7.0).all()) and bool((buf[2 * w:] == -7.0).all())


@pytest.mark.parametrize("Cn", [20, 520])
@pytest.mark.parametrize("counts", R.COMBINE_WORLDS, ids=str)
def test_combine_stats(counts, Cn):
    """combine_stats_sync / combine_stats on hand-built gathered rows: worlds of 1, 2, 3
    with unequal counts and a one-element rank; the running stats use the GLOBAL count."""
    C = B()
    _, means, vars_, cnt = R.combine_inputs(counts, Cn)
    g = torch.Generator().manual_seed(11)
    rm0, rv0 = torch.randn(Cn, generator=g), torch.rand(Cn, generator=g) + 0.5
    ref = R.ref_combine(means, vars_, cnt, R.EPS, R.MOMENTUM, rm0, rv0)
    gathered = torch.cat([means, vars_, cnt.reshape(-1, 1)], 1).to(DEV)
    tag = "combine %s C=%d" % (counts, Cn)

    def sync():
        rm, rv = rm0.to(DEV), rv0.to(DEV)
        nbt = torch.tensor(7, dtype=torch.int64, device=DEV)
        return C.combine_stats_sync(gathered, R.EPS, R.MOMENTUM, rm, rv, nbt) + (rm, rv, nbt)

    mean, invstd, inv_total, rm, rv, nbt = twice(sync, tag + " sync")
    for got, name in ((mean, "mean"), (invstd, "invstd"), (inv_total, "inv_total"),
                      (rm, "running_mean"), (rv, "running_var")):
        _within(got, ref[name], "combine." + name, tag + " sync")
    assert int(nbt) == 8
    bare = C.combine_stats_sync(gathered, R.EPS, R.MOMENTUM, None, None)
    _same(bare, (mean, invstd, inv_total), tag + " sync without running stats")

    def plain():
        rm, rv = rm0.to(DEV), rv0.to(DEV)
        return C.combine_stats(means.to(DEV), vars_.to(DEV), cnt.to(DEV), R.EPS, R.MOMENTUM,
                               rm, rv) + (rm, rv)

    mean, invstd, var, rm, rv = twice(plain, tag)
    for got, name in ((mean, "mean"), (invstd, "invstd"), (var, "var"), (rm, "running_mean"),
                      (rv, "running_var")):
        _within(got, ref[name], "combine." + name, tag)


# ------------------------------------------------------------------------- slab finalizes
@pytest.mark.parametrize("Cn", R.SLAB_C)
@pytest.mark.parametrize("S", R.SLAB_S)
def test_slab_stats(S, Cn):
    """slab_train_stats / slab_packed_stats on a synthetic [2][C][S] slab (the layout the
    conv epilogues write), with and without a shift: every slab_ch instantiation, the
    unrolled loop with and without its tail, S below the threads per channel."""
    C = B()
    for with_shift in (True, False):
        slab, count, shift = R.slab_inputs(S, Cn, with_shift=with_shift)
        g = torch.Generator().manual_seed(13)
        rm0, rv0 = torch.randn(Cn, generator=g), torch.rand(Cn, generator=g) + 0.5
        ref = R.ref_slab_stats(slab, count, shift, R.EPS, R.MOMENTUM, rm0, rv0)
        sd, shd = slab.to(DEV), _dev(shift)
        tag = "slab S=%d C=%d shift=%s" % (S, Cn, with_shift)

        def train():
            rm, rv = rm0.to(DEV), rv0.to(DEV)
            nbt = torch.tensor(0, dtype=torch.int64, device=DEV)
            return C.slab_train_stats(sd, count, shd, rm, rv, nbt, R.EPS, R.MOMENTUM) + (
                rm, rv, nbt)

        mean, invstd, rm, rv, nbt = twice(train, tag)
        for got, name in ((mean, "mean"), (invstd, "invstd"), (rm, "running_mean"),
                          (rv, "running_var")):
            _within(got, ref[name], "slab." + name, tag)
        assert int(nbt) == 1
        bare = C.slab_train_stats(sd, count, shd, None, None, None, R.EPS, R.MOMENTUM)
        _same(bare, (mean, invstd), tag + " without running stats")
        packed = twice(lambda: C.slab_packed_stats(sd, count, shd), tag + " packed")
        _same(packed[:Cn], mean, tag + " packed mean")
        _within(packed[Cn:2 * Cn], ref["var"], "slab.var", tag)
        assert float(packed[2 * Cn]) == float(count)
        w = 2 * Cn + 1
        buf = torch.full((3 * w,), -7.0, device=DEV)
        out = C.slab_packed_stats(sd, count, shd, out=buf[w:2 * w])
        assert out.data_ptr() == buf[w:2 * w].data_ptr()
        _same(buf[w:2 * w], packed, tag + " out= slot")
        assert bool((buf[:w] == -7.0).all()) and bool((buf[2 * w:] == -7.0).all())


@pytest.mark.parametrize("wdt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("Cn", R.SLAB_C)
@pytest.mark.parametrize("S", R.SLAB_S)
def test_slab_reduce_grad(S, Cn, wdt):
    """slab_reduce_grad: plain, with sum_scale, and into targets (accumulate / overwrite)."""
    C = B()
    slab, invstd = R.grad_slab_inputs(S, Cn)
    g = torch.Generator().manual_seed(17)
    weight = (torch.rand(Cn, generator=g) + 0.5).to(wdt).to(DEV)
    gw0, gb0 = torch.randn(Cn, generator=g).to(wdt), torch.randn(Cn, generator=g).to(wdt)
    sd, ivd = slab.to(DEV), invstd.to(DEV)
    tag = "slab reduce S=%d C=%d %s" % (S, Cn, _name(wdt))
    ref = R.ref_slab_reduce(slab, invstd)
    s1, s2, gw, gb = twice(lambda: C.slab_reduce_grad(sd, ivd, weight, True), tag)
    _within(s1, ref["sum_dy"], "slab.sum_dy", tag)
    _within(s2, ref["sum_dy_xmu"], "slab.sum_dy_xmu", tag)
    assert gw.dtype == wdt and gb.dtype == wdt
    _within(gw, ref["dgamma"], "slab.dgamma." + _name(wdt), tag)
    _within(gb, ref["dbeta"], "slab.dbeta." + _name(wdt), tag)
    none = C.slab_reduce_grad(sd, ivd, weight, False)
    assert none[2] is None and none[3] is None
    _same(none[:2], (s1, s2), tag + " need_wgrad=False")
    sc = torch.tensor([1.0 / 3], dtype=F32)
    ref = R.ref_slab_reduce(slab, invstd, sum_scale=sc, gw0=gw0, gb0=gb0)

    def acc(on):
        tw, tb = gw0.to(DEV), gb0.to(DEV)
        out = C.slab_reduce_grad(sd, ivd, weight, True, sum_scale=sc.to(DEV), grad_weight=tw,
                                 grad_bias=tb, accumulate=on)
        assert out[2].data_ptr() == tw.data_ptr() and out[3].data_ptr() == tb.data_ptr()
        return out

    t1, t2, tw, tb = twice(lambda: acc(True), tag + " accumulate")
    _within(t1, ref["sum_dy"], "slab.sum_dy.scaled", tag)
    _within(t2, ref["sum_dy_xmu"], "slab.sum_dy_xmu.scaled", tag)
    _within(tw, ref["dgamma"], "slab.dgamma.accumulate." + _name(wdt), tag)
    _within(tb, ref["dbeta"], "slab.dbeta.accumulate." + _name(wdt), tag)
    _, _, tw, tb = twice(lambda: acc(False), tag + " overwrite")
    _same((tw, tb), (gw, gb), tag + " accumulate=False overwrites the targets")


# ------------------------------------------------------------------------- fused forms
def _x2_chain(M, Cn):
    """backward_k<X2>: a thread's rows of the elementwise grid, the LDS row-group combine,
    then slab_t_sum over the blocks."""
    g = R.ngeom(Cn, True)
    blocks = R.elem_blocks(M, g, M * Cn * 2)
    return float(-(-M // (blocks * g.rows_iter)) + g.rows_iter - 1 + R.slab_chain(blocks))


@pytest.mark.parametrize("M,Cn", R.FUSED_X2, ids=str)
@pytest.mark.parametrize("dt", [BF16, F16], ids=_name)
def test_fused_two_bn_forms_at_the_new_edges(M, Cn, dt):
    """apply2_mask and backward_elemt_x2 at a second channel block with one lane (520) and
    four channel blocks (2048), with an M that leaves a clamped tail: bitwise the separate
    passes checked above; the second BN's sums within the bound of the reference."""
    C = B()
    c = R.case(R.rows_shape(M, Cn), "nhwc", "vec")
    a = R.make_inputs(c.shape, dt, F32, "nhwc", seed=21)
    d = R.make_inputs(c.shape, dt, F32, "nhwc", seed=22)
    x, xd, dy = _place(a["x"], c), _place(d["x"], c), _place(a["dy"], c)
    assert C.backward_x2_ok(dy, x, xd)
    g = torch.Generator().manual_seed(23)
    st = [(torch.randn(Cn, generator=g) * 0.3).to(DEV) for _ in range(2)]
    iv = [(torch.rand(Cn, generator=g) + 0.5).to(DEV) for _ in range(2)]
    w, b, wd, bd = (_dev(t) for t in (a["weight"], a["bias"], d["weight"], d["bias"]))
    y, mask = twice(lambda: C.apply2_mask(x, st[0], iv[0], w, b, xd, st[1], iv[1], wd, bd),
                    "apply2_mask")
    z = C.apply(xd, st[1], iv[1], wd, bd, None, False)
    _same((y, mask), C.apply_mask(x, st[0], iv[0], w, b, z, True), "apply2_mask == two passes")
    sdy = torch.randn(Cn, generator=g).to(DEV)
    sdx = torch.randn(Cn, generator=g).to(DEV)
    dx, s1, s2, gw2, gb2 = twice(
        lambda: C.backward_elemt_x2(dy, x, st[0], iv[0], w, b, sdy, sdx, float(M), xd, st[1],
                                    iv[1], wd, True), "backward_elemt_x2")
    dx_sep, _ = C.backward_elemt(dy, x, st[0], iv[0], w, b, sdy, sdx, float(M), None, False,
                                 False)
    _same(dx, dx_sep, "backward_elemt_x2 dx == backward_elemt")
    ref = R.ref_backward(a["dy"], d["x"], None, st[1].cpu(), iv[1].cpu(), d["weight"],
                         max(_x2_chain(M, Cn), R.nhwc_chain(M, Cn)))
    tag = "x2 (%d, %d) %s" % (M, Cn, _name(dt))
    _within(s1, ref["sum_dy"], "x2.sum_dy", tag)
    _within(s2, ref["sum_dy_xmu"], "x2.sum_dy_xmu", tag)
    _within(gw2, ref["dgamma"], "x2.dgamma", tag)
    _within(gb2, ref["dbeta"], "x2.dbeta", tag)
    r1, r2, rw, rb = C.reduce_grad(dy, xd, st[1], iv[1], wd, bd, None, False, True)
    _within(r1, ref["sum_dy"], "sum_dy", tag + " separate")
    _within(r2, ref["sum_dy_xmu"], "sum_dy_xmu", tag + " separate")


# ------------------------------------------------------------------------- through autograd
def _module_inputs(shape, layout, dt, relu, affine=True, seed=30):
    c = R.case(shape, layout, "vec")
    inp = R.make_inputs(shape, dt, F32, layout, relu=relu, seed=seed, affine=affine)
    return c, inp, R.red_chain(shape, layout == "nhwc")


def _load(mod, inp, affine, track):
    with torch.no_grad():
        if affine:
            mod.weight.copy_(inp["weight"])
            mod.bias.copy_(inp["bias"])
        if track:
            mod.running_mean.copy_(inp["running_mean"])
            mod.running_var.copy_(inp["running_var"])
    return mod


def _step(mod, c, inp, affine):
    x = _place(inp["x"], c).requires_grad_(True)
    y = mod(x)
    y.backward(_place(inp["dy"], c))
    torch.cuda.synchronize()
    return x, y


def _check_step(mod, x, y, ref, mask, affine, tag, relu):
    _within(y, ref["y"], "y", tag)
    if relu:
        assert torch.equal(y.detach().cpu() > 0, mask)
    _within(x.grad, ref["dx"], "dx", tag)
    if affine:
        _within(mod.weight.grad, ref["dgamma"], "dgamma.fp32", tag)
        _within(mod.bias.grad, ref["dbeta"], "dbeta.fp32", tag)


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("shape", R.MODULE_SHAPES, ids=str)
@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("option", ["momentum_none", "no_running_stats", "no_affine"])
def test_batchnorm2d_relu_options(option, dt, shape, layout):
    from apex_example_amd.ops.batch_norm import BatchNorm2dReLU

    affine = option != "no_affine"
    track = option != "no_running_stats"
    kw = dict(momentum=None) if option == "momentum_none" else {}
    c, inp, chain = _module_inputs(shape, layout, dt, True, affine)
    mod = _load(BatchNorm2dReLU(shape[1], eps=R.EPS, affine=affine, track_running_stats=track,
                                **kw).to(DEV), inp, affine, track)
    w, b = (inp["weight"], inp["bias"]) if affine else (None, None)
    tag = "BatchNorm2dReLU %s %s %s %s" % (option, _name(dt), shape, layout)
    steps = 3 if option == "momentum_none" else 1
    for k in range(1, steps + 1):
        mom = 1.0 / k if option == "momentum_none" else R.MOMENTUM
        rm0 = mod.running_mean.detach().cpu().clone() if track else None
        rv0 = mod.running_var.detach().cpu().clone() if track else None
        mod.zero_grad(set_to_none=True)
        x, y = _step(mod, c, inp, affine)
        st = R.ref_stats(inp["x"], R.EPS, chain, mom, rm0, rv0)
        fw = R.ref_apply(inp["x"], st["mean"], st["invstd"], w, b, None, True)
        bw = R.ref_backward(inp["dy"], inp["x"], fw["mask"], st["mean"], st["invstd"], w, chain)
        _check_step(mod, x, y, dict(fw, **bw), fw["mask"], affine, tag + " step %d" % k, True)
        if track:
            # cumulative average: momentum 1 / k, each step from what the device stored
            _within(mod.running_mean, st["running_mean"], "running_mean", tag)
            _within(mod.running_var, st["running_var"], "running_var", tag)
            assert int(mod.num_batches_tracked) == k
        else:
            assert mod.running_mean is None and mod.num_batches_tracked is None


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("shape", R.MODULE_SHAPES, ids=str)
def test_batchnorm2d_relu_eval(shape, layout):
    """Eval mode: the running statistics, given exactly."""
    from apex_example_amd.ops.batch_norm import BatchNorm2dReLU

    c, inp, chain = _module_inputs(shape, layout, F32, False)
    mod = _load(BatchNorm2dReLU(shape[1], eps=R.EPS).to(DEV), inp, True, True).eval()
    y = mod(_place(inp["x"], c))
    iv = R.vrsqrt(R.Val(inp["running_var"].double()) + R.f32(R.EPS))
    ref = R.ref_apply(inp["x"], inp["running_mean"], iv, inp["weight"], inp["bias"], None, True)
    # (the zero set of relu needs no ambiguity handling here: y is compared, not a mask)
    _within(y, ref["y"], "y.eval", "BatchNorm2dReLU eval %s %s" % (shape, layout))
    assert int(mod.num_batches_tracked) == 0
    _same(mod.running_mean.cpu(), inp["running_mean"], "eval leaves the running stats")


@pytest.mark.parametrize("shape", R.MODULE_SHAPES, ids=str)
@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("convention", ["nchw", "nhwc", "channel_last_shape"])
def test_sync_batchnorm_local(convention, dt, shape):
    """SyncBatchNorm with a local process group, also in apex's channel_last=True shape
    convention (C is the last dimension of the shape)."""
    from apex_example_amd.parallel import SyncBatchNorm

    layout = "nchw" if convention == "nchw" else "nhwc"
    c, inp, chain = _module_inputs(shape, layout, dt, False)
    cl_shape = convention == "channel_last_shape"
    mod = _load(SyncBatchNorm(shape[1], eps=R.EPS, channel_last=cl_shape).to(DEV), inp, True,
                True)
    tag = "SyncBatchNorm %s %s %s" % (convention, _name(dt), shape)
    if cl_shape:
        x = inp["x"].permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
        y = mod(x)
        y.backward(inp["dy"].permute(0, 2, 3, 1).contiguous().to(DEV))
        assert y.shape == x.shape
        yv, xg = y.permute(0, 3, 1, 2), x.grad.permute(0, 3, 1, 2)
    else:
        x, y = _step(mod, c, inp, True)
        yv, xg = y, x.grad
    st = R.ref_stats(inp["x"], R.EPS, max(chain, R.red_chain(shape, True)), R.MOMENTUM,
                     inp["running_mean"], inp["running_var"])
    fw = R.ref_apply(inp["x"], st["mean"], st["invstd"], inp["weight"], inp["bias"], None, False)
    bw = R.ref_backward(inp["dy"], inp["x"], None, st["mean"], st["invstd"], inp["weight"],
                        max(chain, R.red_chain(shape, True)))
    _within(yv, fw["y"], "y", tag)
    _within(xg, bw["dx"], "dx", tag)
    _within(mod.weight.grad, bw["dgamma"], "dgamma.fp32", tag)
    _within(mod.bias.grad, bw["dbeta"], "dbeta.fp32", tag)
    _within(mod.running_mean, st["running_mean"], "running_mean", tag)
    _within(mod.running_var, st["running_var"], "running_var", tag)
    assert int(mod.num_batches_tracked) == 1
