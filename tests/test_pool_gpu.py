"""The pooling kernels (csrc/hip/pool.hip) against the float64 references of
tests/pool_ref.py, at every kernel and template instantiation the dispatch can select.

The bindings of ``_native.require().pool`` are called directly, so that the saved tap index
and the BatchNorm slab are visible; one test goes through MaxPool2dNHWC / bn_relu_maxpool
to show that autograd returns the same tensors.  Forward outputs and tap indices must be
EQUAL to the reference (bit patterns, signed zeros included; NaN where it has NaN); with
the BatchNorm on load and operands that are not exactly representable, a window the
reference cannot decide (pool_ref.decided, at least 99 % are decided) may take another tap
under the rule of pool_ref's docstring.  Gradients are equal under exactly representable
inputs and within optim_ref.bound otherwise; every backward runs twice and must return
identical bits.

Which kernel a case reaches is computed by pool_ref.fwd_kernel / bwd_kernel (the dispatch
conditions of maxpool2d_nhwc_fwd / _bwd) and named in each test;
``test_every_instantiation_is_reached`` holds the case lists to the full set.

  kernel (types)                               reached by
  maxpool_fwd_k<T, VEC, plain> (fp32/16)       test_max_pool: C = 8, 24, 64; 16-bit: every
                                               geometry but 3x3 / 2 / 1
  maxpool_fwd_k<T, scalar, plain> (all)        test_max_pool: C = 1, 5; C = 8, 64 one element
                                               into the storage; test_grid_stride_generic
  maxpool_fwd_k<T, VEC, BN> (all)              test_max_pool_bn_forward: as above; C = 520 at
                                               3x3 / 2 / 1 (above kPoolBNMaxC)
  maxpool_fwd_k<T, scalar, BN> (all)           test_max_pool_bn_forward: C = 1, 5, offset 1
  maxpool3s2_fwd_k<T, plain> (fp16, bf16)      test_max_pool 3x3 / 2 / 1, C % 8 == 0;
                                               test_grid_stride_stem
  maxpool3s2_fwd_k<T, BN> (fp16, bf16)         test_max_pool_bn_forward 3x3 / 2 / 1;
                                               test_stem_backward_bn (its idx)
  maxpool_bwd_k<T, VEC | scalar> (all)         test_max_pool, test_grid_stride_generic
  maxpool3s2_bwd2_k<T, plain> (fp16, bf16)     test_max_pool 3x3 / 2 / 1; test_grid_stride_stem
  maxpool3s2_bwd2_k<T, BNR> (fp16, bf16)       test_stem_backward_bn,
                                               test_grid_stride_stem_backward_bn
  gap_bwd_k<T, VEC | scalar> (all)             test_gap_backward, test_grid_stride_gap_backward

Worst |err| / bound measured on an MI355X (printed at the end of a run with -s).  Outputs
stored in fp32 (or summed in fp32) show the arithmetic: maxpool_bwd_k dx 0.06, BN forward
y 0.07, gap_bwd_k dx 0.09, the stem backward's sum_dy 0.00 and sum_dy_xmu 0.01 (float32
emulation on the CPU: 0.19, -, 0.46, 0.01, 0.02).  With 16-bit outputs every ratio is
0.92 .. 1.00: the final rounding to the storage type, which the bound's u_T*|ref| term is
there for (a half-ulp tie is attained, never exceeded)."""
import functools

import pytest
import torch

import pool_ref as R
from pool_ref import BF16, F16, F32, F64, Val

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}
GEOMS = R.geometries()
DTYPES = [F32, F16, BF16]
HALF = [F16, BF16]
STEM_HW = [(8, 10), (9, 11), (7, 6), (1, 1), (2, 2), (30, 30)]
N = 2


def P():
    from apex_example_amd import _native

    return _native.require().pool


def _name(v):
    return {F32: "fp32", F16: "fp16", BF16: "bf16"}.get(v, str(v))


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst |err| / bound per kernel output over the run:")
    for k in sorted(WORST):
        print("  WORST %-44s %.3f" % (k, WORST[k]))


def _within(got, ref, name, tag=""):
    r = R.worst_ratio(got.detach().to(ref.v.device), ref)
    key = "%s [%s]" % (name, _name(got.dtype))
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1.0, "%s %s: |err| / bound = %g" % (tag, name, r)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_values(got, ref64, what):
    """``got`` holds exactly the reference's values: NaN where it has NaN, the same bit
    pattern (the sign of a zero included) everywhere else."""
    want = ref64.to(got.device).to(got.dtype)
    assert got.shape == want.shape, what
    assert torch.equal(got.isnan(), want.isnan()), what + ": NaN positions"
    ok = ~want.isnan()
    assert torch.equal(_bits(got)[ok], _bits(want)[ok]), what


def _twice(fn, what):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b)), what + ": not bitwise reproducible"
    return a


def _offsets(C):
    """Storage offsets walked for a channel count: 1 element (a misaligned view: the scalar
    kernels although C % 8 == 0) for C = 8 and 64."""
    return (0, 1) if C in (8, 64) else (0,)


# ------------------------------------------------------------ shared references (CPU)
MAKERS = ("tie_free", "tied", "exact", "special")


@functools.lru_cache(maxsize=None)
def _plain_case(geom, C, maker):
    """x, the exact-integer dy, (y, tap) and the exact dx of one case: built once, shared by
    the three storage types (every value is representable in each)."""
    k, s, p, (H, W) = geom
    shape = (N, C, H, W)
    ex = R.exact_ints(shape, k, s, p, 11)
    x = {"tie_free": lambda: R.tie_free(shape, k, 1), "tied": lambda: R.tied(shape, 2),
         "exact": lambda: ex["x"], "special": lambda: R.special(shape, k, 3)}[maker]()
    y, tap = R.ref_maxpool_fwd(x, k, s, p)
    return x, ex["dy"], y, tap, R.ref_maxpool_bwd(ex["dy"], tap, H, W, k, s, p)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom", GEOMS, ids=R.geom_id)
def test_max_pool(geom, dtype):
    """maxpool_fwd_k<T, VEC | scalar, plain> and maxpool_bwd_k<T, VEC | scalar>; for 16-bit
    types, C % 8 == 0, aligned storage and 3x3 / 2 / 1 the stem kernels
    maxpool3s2_fwd_k<T, plain> and maxpool3s2_bwd2_k<T, plain>."""
    k, s, p, (H, W) = geom
    for C in R.CHANNELS:
        for off in _offsets(C):
            for maker in MAKERS:
                tag = "%s C=%d off=%d %s [%s / %s]" % (
                    R.geom_id(geom), C, off, maker, R.fwd_kernel(dtype, C, k, s, p, off == 0),
                    R.bwd_kernel(dtype, C, k, s, p, off == 0))
                x, dyi, ry, tap, rdx = _plain_case(geom, C, maker)
                xg = R.place(x, dtype, DEV, off)
                assert (xg.data_ptr() % 16 == 0) == (off == 0)
                y, idx = P().max_fwd(xg, k, s, p)
                _same_values(y, ry, tag + " y")
                assert torch.equal(idx.cpu().long(), tap), tag + " idx"
                # exactly representable dy: equality
                dyg = R.place(dyi, dtype, DEV, off)
                dx = _twice(lambda: P().max_bwd(dyg, idx, H, W, k, s, p), tag + " dx")
                _same_values(dx, rdx.v, tag + " dx (exact)")
                # random dy: the bound of the addition chain
                dyr = R.rand_dy(dyi.shape, 4).to(dtype)
                dx = _twice(lambda: P().max_bwd(R.place(dyr, dtype, DEV, off), idx, H, W, k, s, p),
                            tag + " dx")
                _within(dx.cpu(), R.ref_maxpool_bwd(dyr, tap, H, W, k, s, p),
                        R.bwd_kernel(dtype, C, k, s, p, off == 0) + " dx", tag)


# ------------------------------------------------------------ BatchNorm + ReLU on load
@functools.lru_cache(maxsize=None)
def _bn_case(geom, C, dtype, exact):
    k, s, p, (H, W) = geom
    shape = (N, C, H, W)
    if exact:
        inp = R.zero_channel(R.exact_ints(shape, k, s, p, 13))
        x, bn = inp["x"].to(dtype), tuple(inp[n] for n in ("mean", "invstd", "w", "b"))
    else:
        x, bn = R.bn_x(shape, k, 7).to(dtype), R.bn_params(C, 7)
    return (x, bn) + tuple(R.ref_maxpool_fwd(x, k, s, p, bn=bn))


def _check_bn_forward(y, idx, ref, dtype, geom, exact, kern, tag):
    k, s, p, _ = geom
    ry, tap, pre = ref
    y, idx = y.cpu(), idx.cpu().long()
    if exact:
        _same_values(y, ry, tag + " y")
        assert torch.equal(idx, tap), tag + " idx"
        return
    dec = R.decided(pre, tap, dtype, k, s, p)
    assert float(dec.double().mean()) >= 0.99, tag + " decided share"
    same = idx == tap
    assert bool(same[dec].all()), tag + " idx differs in a decided window"
    at = Val(R.at_tap(pre.v, idx, k, s, p), R.at_tap(pre.e, idx, k, s, p))
    _within(y, at, kern + " y", tag)
    if not bool(same.all()):
        top = Val(R.at_tap(pre.v, tap, k, s, p), R.at_tap(pre.e, tap, k, s, p))
        near = (top.v - at.v).abs() <= R.bound(top, dtype)
        assert bool(near[~same].all()), tag + " another tap that is not within the bound"


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom", GEOMS, ids=R.geom_id)
def test_max_pool_bn_forward(geom, dtype):
    """maxpool_fwd_k<T, VEC | scalar, BN>; for 16-bit types, C % 8 == 0, aligned storage,
    3x3 / 2 / 1 and C <= 512 maxpool3s2_fwd_k<T, BN>; C = 520 falls off it (kPoolBNMaxC)
    onto the generic VEC + BN kernel.  With and without weight / bias."""
    k, s, p, (H, W) = geom
    for C in R.CHANNELS + [520]:
        for off in _offsets(C):
            for exact in (False, True):
                kern = R.fwd_kernel(dtype, C, k, s, p, off == 0, bn=True)
                tag = "%s C=%d off=%d %s [%s]" % (R.geom_id(geom), C, off,
                                                  "exact" if exact else "bn_x", kern)
                x, bn, ry, tap, pre = _bn_case(geom, C, dtype, exact)
                xg = R.place(x, dtype, DEV, off)
                bng = [t.to(DEV) for t in bn]
                y, idx = P().max_fwd_bn(xg, *bng, k, s, p)
                _check_bn_forward(y, idx, (ry, tap, pre), dtype, geom, exact, kern, tag)
    # null weight / bias pointers
    C = 8
    x, bn, _, _, _ = _bn_case(geom, C, dtype, False)
    bn0 = (bn[0], bn[1], None, None)
    y, idx = P().max_fwd_bn(x.to(DEV).contiguous(memory_format=torch.channels_last),
                            bn[0].to(DEV), bn[1].to(DEV), None, None, k, s, p)
    _check_bn_forward(y, idx, R.ref_maxpool_fwd(x, k, s, p, bn=bn0), dtype, geom, False,
                      R.fwd_kernel(dtype, C, k, s, p, True, bn=True), "no affine")


# ------------------------------------------------------------ the fused stem backward
def _check_bnr(x, dy, bn, dtype, exact, tag, dev="cpu"):
    """maxpool3s2_bwd2_k<T, true> on device tensors; the reference on ``dev``."""
    Nn, C, H, W = x.shape
    mean, invstd, w, b = bn
    y, idx = P().max_fwd_bn(x, mean, invstd, w, b, 3, 2, 1)
    plain = P().max_bwd(dy, idx, H, W, 3, 2, 1)
    outs = [P().max_bwd_bn(dy, idx, H, W, x, mean, invstd, w, b) for _ in range(2)]
    torch.cuda.synchronize()
    dx, slab = outs[0]
    assert torch.equal(_bits(dx), _bits(outs[1][0])) and torch.equal(slab, outs[1][1]), \
        tag + ": not bitwise reproducible"
    assert torch.equal(_bits(dx), _bits(plain)), tag + " dx differs from max_bwd's"
    assert slab.shape == (2, 64, R.bnr_grid(Nn, H, W)) and slab.dtype == F32
    to = (lambda t: None if t is None else t.to(dev))
    ref = R.ref_maxpool_bwd_bn(to(dy), to(idx).long(), to(x), to(mean), to(invstd), to(w), to(b),
                               dx_stored=to(dx))
    got = slab.to(F64).sum(-1).to(dev)
    kern = "maxpool3s2_bwd2_k<BNR>"
    if exact:
        xm = (to(x).to(F64) - to(mean).to(F64).view(1, -1, 1, 1)).abs()
        assert float((to(dx).to(F64).abs() * xm).sum((0, 2, 3)).max()) < 2 ** 24
        _same_values(dx, ref["dx"].v, tag + " dx (exact)")
        assert torch.equal(got[0], ref["sum_dy"].v), tag + " sum_dy (exact)"
        assert torch.equal(got[1], ref["sum_dy_xmu"].v), tag + " sum_dy_xmu (exact)"
    else:
        assert not bool(R.bnr_ambiguous(to(x), to(mean), to(invstd), to(w), to(b)).any())
        _within(dx.to(dev), ref["dx"], kern + " dx", tag)
        # as the consumer stores them: fp32 (a channel that ReLU closes sums to an exact 0)
        _within(got[0].to(F32), ref["sum_dy"], kern + " sum_dy", tag)
        _within(got[1].to(F32), ref["sum_dy_xmu"], kern + " sum_dy_xmu", tag)
    return ref


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("hw", STEM_HW, ids=lambda hw: "%dx%d" % hw)
def test_stem_backward_bn(hw, dtype):
    """maxpool3s2_bwd2_k<T, true> (C = 64): dx, and the slab of sum(d), sum(d*(x - mean))
    itself; odd sizes reach the h >= H, w >= W and !ok[q] branches; exact operands with a
    whole channel at fma(x, sc, sh) == 0; without weight / bias."""
    H, W = hw
    shape = (N, 64, H, W)
    oshape = (N, 64, R.out_size(H, 3, 2, 1), R.out_size(W, 3, 2, 1))
    for exact in (True, False):
        if exact:
            inp = R.zero_channel(R.exact_ints(shape, 3, 2, 1, 17))
            x, dy = inp["x"], inp["dy"]
            bn = [inp[n] for n in ("mean", "invstd", "w", "b")]
        else:
            x, dy, bn = R.bn_x(shape, 3, 7), R.rand_dy(oshape, 4), list(R.bn_params(64, 7))
        xg = R.place(x, dtype, DEV)
        dyg = R.place(dy, dtype, DEV)
        bng = [t.to(DEV) for t in bn]
        tag = "%dx%d %s %s" % (H, W, _name(dtype), "exact" if exact else "random")
        ref = _check_bnr(xg, dyg, bng, dtype, exact, tag)
        if exact:
            assert float(ref["sum_dy"].v[0]) == 0.0 and not bool(ref["cond"][:, 0].any())
        _check_bnr(xg, dyg, [bng[0], bng[1], None, None], dtype, exact, tag + " no affine")


# ------------------------------------------------------------ grid-stride loops
def _over(items, cap, what):
    assert items > cap, "%s: %d items do not exceed the grid's %d threads" % (what, items, cap)


def test_grid_stride_generic():
    """maxpool_fwd_k<bf16, scalar, plain> / maxpool_bwd_k<bf16, scalar> with more items than
    pool_grid's 16384 blocks of 256 threads: the second iteration of both loops."""
    c = R.BIG["generic"]
    k, s, p, shape = c["k"], c["s"], c["p"], c["shape"]
    _over(c["fwd_items"], R.GRID_CAP * R.THREADS, "forward")
    _over(c["bwd_items"], R.GRID_CAP * R.THREADS, "backward")
    assert R.fwd_kernel(BF16, shape[1], k, s, p) == "maxpool_fwd_k<scalar,plain>"
    x = R.tied(shape, 2, DEV)
    xg = R.place(x, BF16, DEV)
    y, idx = P().max_fwd(xg, k, s, p)
    ry, tap = R.ref_maxpool_fwd(x, k, s, p)
    _same_values(y, ry, "y")
    assert torch.equal(idx.long(), tap)
    dy = torch.randint(-8, 9, tap.shape, device=DEV).float()
    dx = _twice(lambda: P().max_bwd(R.place(dy, BF16, DEV), idx, shape[2], shape[3], k, s, p), "dx")
    _same_values(dx, R.ref_maxpool_bwd(dy, tap, shape[2], shape[3], k, s, p).v, "dx")


def test_grid_stride_stem():
    """maxpool3s2_fwd_k<bf16, plain> / maxpool3s2_bwd2_k<bf16, plain> above the cap."""
    c = R.BIG["stem"]
    shape = c["shape"]
    _over(c["fwd_items"], R.GRID_CAP * R.THREADS, "forward")
    _over(c["blk_items"], R.GRID_CAP * R.THREADS, "backward")
    assert R.fwd_kernel(BF16, shape[1], 3, 2, 1) == "maxpool3s2_fwd_k<plain>"
    x = R.tied(shape, 2, DEV)
    xg = R.place(x, BF16, DEV)
    y, idx = P().max_fwd(xg, 3, 2, 1)
    ry, tap = R.ref_maxpool_fwd(x, 3, 2, 1)
    _same_values(y, ry, "y")
    assert torch.equal(idx.long(), tap)
    dy = torch.randint(-8, 9, tap.shape, device=DEV).float()
    dx = _twice(lambda: P().max_bwd(R.place(dy, BF16, DEV), idx, shape[2], shape[3], 3, 2, 1), "dx")
    _same_values(dx, R.ref_maxpool_bwd(dy, tap, shape[2], shape[3], 3, 2, 1).v, "dx")


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
def test_grid_stride_stem_backward_bn(exact):
    """maxpool3s2_bwd2_k<bf16, true> with more 2x2-block items than 2048 blocks of 256
    threads: a thread's s1 / s2 carry over its iterations, its channel group must stay
    fixed (the grid stride is a multiple of 8), and the odd H puts the h >= H branch into
    the later iterations."""
    c = R.BIG["bnr"]
    shape = c["shape"]
    Nn, C, H, W = shape
    _over(R.bnr_items(Nn, H, W), R.BNR_GRID_CAP * R.THREADS, "stem backward with BN sums")
    assert H % 2 == 1 and C == 64
    oshape = (Nn, C, R.out_size(H, 3, 2, 1), R.out_size(W, 3, 2, 1))
    if exact:
        inp = R.zero_channel(R.exact_ints(shape, 3, 2, 1, 19, DEV, dmax=1))
        x, dy = inp["x"], inp["dy"]
        bn = [inp[n] for n in ("mean", "invstd", "w", "b")]
    else:
        x, dy, bn = R.bn_x(shape, 3, 7, DEV), R.rand_dy(oshape, 4, DEV), list(R.bn_params(64, 7, DEV))
    _check_bnr(R.place(x, BF16, DEV), R.place(dy, BF16, DEV), bn, BF16, exact,
               "grid stride", dev=DEV)


def test_grid_stride_gap_backward():
    """gap_bwd_k<bf16, scalar> above the cap."""
    c = R.BIG["gap"]
    Nn, C, H, W = c["shape"]
    _over(c["items"], R.GRID_CAP * R.THREADS, "gap backward")
    assert C % 8 != 0
    dy = torch.randn(Nn, C, device=DEV).to(BF16)
    dx = P().gap_bwd(dy, H, W)
    _within(dx, R.ref_gap_bwd(dy, H, W)["dx"], "gap_bwd_k<scalar> dx", "grid stride")


# ------------------------------------------------------------ global average pool
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_gap_backward(dtype):
    """gap_bwd_k<T, VEC> (C % 8 == 0, aligned dy), gap_bwd_k<T, scalar> (C = 12, and C = 8
    with dy one element into its storage)."""
    for (Nn, C, H, W), off in (((3, 2048, 7, 7), 0), ((2, 12, 5, 3), 0), ((3, 8, 4, 5), 1),
                               ((2, 8, 1, 1), 0)):
        dy = torch.randn(Nn, C).to(dtype)
        buf = torch.empty(Nn * C + off, dtype=dtype, device=DEV)
        dyg = buf[off:].view(Nn, C)
        dyg.copy_(dy)
        vec = C % 8 == 0 and off == 0
        assert (dyg.data_ptr() % 16 == 0) == (off == 0)
        dx = _twice(lambda: P().gap_bwd(dyg, H, W), "gap dx")
        assert dx.shape == (Nn, C, H, W) and dx.is_contiguous(memory_format=torch.channels_last)
        _within(dx.cpu(), R.ref_gap_bwd(dy, H, W)["dx"],
                "gap_bwd_k<%s> dx" % ("VEC" if vec else "scalar"), str((Nn, C, H, W, off)))
    # a power-of-two HW and exactly representable dy: equality
    dy = torch.randint(-64, 65, (3, 16)).float()
    dx = P().gap_bwd(dy.to(dtype).to(DEV), 4, 8)
    _same_values(dx, R.ref_gap_bwd(dy, 4, 8)["dx"].v, "gap dx (exact)")


# ------------------------------------------------------------ the autograd wiring
def test_autograd_returns_the_bindings_tensors():
    from apex_example_amd import _native
    from apex_example_amd.ops import BatchNorm2dReLU
    from apex_example_amd.ops.pool import (GlobalAvgPool2dNHWC, MaxPool2dNHWC, bn_relu_maxpool,
                                           bn_relu_maxpool_fusable)

    C = _native.require()
    x = R.place(R.special((N, 8, 9, 11), 3, 3), BF16, DEV)
    dy = R.place(R.rand_dy((N, 8, 5, 6), 4), BF16, DEV)
    xa = x.clone().requires_grad_(True)
    ya = MaxPool2dNHWC(3, 2, 1)(xa)
    y, idx = C.pool.max_fwd(x, 3, 2, 1)
    _same_values(ya.detach(), y.to(F64), "module y")
    ya.backward(dy)
    assert torch.equal(_bits(xa.grad), _bits(C.pool.max_bwd(dy, idx, 9, 11, 3, 2, 1)))

    shape = (N, 64, 9, 11)
    x = R.place(R.bn_x(shape, 3, 7), BF16, DEV)
    dy = R.place(R.rand_dy((N, 64, 5, 6), 4), BF16, DEV)
    bn = BatchNorm2dReLU(64).to(DEV)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    rm, rv, nbt = bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()
    pool = MaxPool2dNHWC(3, 2, 1)
    xa = x.clone().requires_grad_(True)
    assert bn_relu_maxpool_fusable(xa, bn, pool)
    ya = bn_relu_maxpool(xa, bn, pool)
    ya.backward(dy)
    mean, invstd = C.bn.train_stats(x, rm, rv, nbt, float(bn.eps), float(bn.momentum))
    w, b = bn.weight.detach(), bn.bias.detach()
    y, idx = C.pool.max_fwd_bn(x, mean, invstd, w, b, 3, 2, 1)
    assert torch.equal(_bits(ya.detach()), _bits(y))
    dbn, slab = C.pool.max_bwd_bn(dy, idx, 9, 11, x, mean, invstd, w, b)
    sum_dy, sum_dy_xmu, gw, gb = C.bn.slab_reduce_grad(slab, invstd, w, True)
    dx, _ = C.bn.backward_elemt(dbn, x, mean, invstd, w, b, sum_dy, sum_dy_xmu,
                                float(x.numel() // 64), None, True, False)
    assert torch.equal(_bits(xa.grad), _bits(dx))
    assert torch.equal(bn.weight.grad, gw) and torch.equal(bn.bias.grad, gb)

    xg = x.clone().requires_grad_(True)
    g = torch.randn(N, 64, 1, 1, device=DEV).to(BF16)
    GlobalAvgPool2dNHWC()(xg).backward(g)
    assert torch.equal(_bits(xg.grad), _bits(C.pool.gap_bwd(g, 9, 11)))


# ------------------------------------------------------------ coverage of the dispatch
def test_every_instantiation_is_reached():
    """The case lists above reach every kernel name of pool.hip for every type its
    dispatch admits (no GPU work: the mirror of the dispatch conditions)."""
    fwd, bwd = set(), set()
    for k, s, p, _ in GEOMS:
        for dtype in DTYPES:
            for C in R.CHANNELS + [520]:
                for off in _offsets(C):
                    fwd.add((_name(dtype), R.fwd_kernel(dtype, C, k, s, p, off == 0, bn=True)))
                    if C != 520:
                        fwd.add((_name(dtype), R.fwd_kernel(dtype, C, k, s, p, off == 0)))
                        bwd.add((_name(dtype), R.bwd_kernel(dtype, C, k, s, p, off == 0)))
    want_f = {(t, "maxpool_fwd_k<%s,%s>" % (v, b)) for t in ("fp32", "fp16", "bf16")
              for v in ("VEC", "scalar") for b in ("BN", "plain")}
    want_f |= {(t, "maxpool3s2_fwd_k<%s>" % b) for t in ("fp16", "bf16") for b in ("BN", "plain")}
    want_b = {(t, "maxpool_bwd_k<%s>" % v) for t in ("fp32", "fp16", "bf16")
              for v in ("VEC", "scalar")}
    want_b |= {(t, "maxpool3s2_bwd2_k<plain>") for t in ("fp16", "bf16")}
    assert fwd == want_f, want_f ^ fwd
    assert bwd == want_b, want_b ^ bwd
    # C = 520 with BN: off the stem specialisation
    assert R.fwd_kernel(BF16, 520, 3, 2, 1, bn=True) == "maxpool_fwd_k<VEC,BN>"
