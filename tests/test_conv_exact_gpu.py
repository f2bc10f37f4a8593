"""Exact-integer tests of the MFMA convolution and GEMM kernels on every tile plan
(csrc/hip/conv_igemm.hip conv_tap_k / conv3h_k / the weight-gradient kernels and their
reductions, stem_conv.hip, gemm4w.hip, wgrad4w.hip).

Inputs are small integers (tests/conv_ref.py), so every product and partial sum is exact
in fp32 and the kernel's output must equal the float64 reference rounded once to the
output type BIT FOR BIT - whatever the tiling, ring depth, tile order, split count or
accumulation order.  Every comparison is ``torch.equal`` over the whole tensor; nothing is
masked out and no case is excluded.  Each case names the plan it is there for and asserts
through the launchers' own host query (conv.tap_plan / wgrad_splits / wgrad_tap_tile) that
this is the plan it ran, so a moved threshold fails here instead of silently dropping
coverage.  The tables and the ``make_*`` builders are device-agnostic:
tests/test_conv_ref_cpu.py runs them on the CPU to check conv_ref's conditions.

Contracts met on the way (read off the kernels, compared with them exactly):
* conv_wgrad / splitk_reduce / wgrad4w with ``out=`` and accumulate: ONE rounding of
  fp32(out_prev) + sum (wgrad_reduce_one_k, wgrad_reduce2_k) - no double rounding found;
* stem_wgrad returns the packed [64, 8 (r), 8 (s), 4 (c)] gradient; lanes r = 7, s = 7 and
  c = 3 belong to no filter element and are dropped by StemConvFunction exactly as here.
"""
import os
import zlib

import pytest
import torch

import conv_ref as cr
from test_conv_halo_gpu import SHAPES as _HALO_SHAPES

# test_conv_halo_gpu.py's shapes, plus one: on all of those the cost model (conv3h_cfg)
# prefers 64-wide tiles at 256 pixels - one round of workgroups either way - so the
# 256 x 128 instantiation never ran in that test.  68 pixel tiles x 8 > 512 workgroups
# make the 128-wide tile the cheaper one (test_halo_table_reaches_every_conv3h_plan).
HALO_SHAPES = list(_HALO_SHAPES) + [(22, 64, 28, 28, 512)]
# shape -> conv3h_k's tile width under the switches (halo mode, pixel tile) = (1, 256),
# (1, 224), (64, 256); None: the shape keeps conv_tap_k there (224-pixel tiles exist for the
# 128-wide kernel only)
HALO_BN = {
    (2, 128, 28, 28, 128): (64, 128, 64),
    (2, 256, 14, 14, 256): (64, 128, 64),
    (4, 512, 7, 7, 512): (64, 128, 64),
    (3, 64, 9, 11, 128): (64, 128, 64),
    (5, 128, 5, 3, 256): (64, 128, 64),
    (1, 64, 56, 56, 128): (64, 128, 64),
    (2, 192, 13, 17, 128): (64, 128, 64),
    (2, 64, 56, 56, 64): (64, None, 64),
    (2, 128, 20, 20, 192): (64, None, 64),
    (22, 64, 28, 28, 512): (128, 128, 64),
}
HALO_SWITCHES = [(1, 256), (1, 224), (64, 256)]

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)
CL = torch.channels_last
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16


def _C():
    from apex_example_amd import _native
    return _native.require()


def _seed(name):
    return zlib.crc32(str(name).encode()) & 0x7FFFFFFF


@pytest.fixture
def sw():
    """The conv A/B switches; every one is put back to its load-time value afterwards
    (apex_example_amd/_native.py reads the same environment variables)."""
    cv = _C().conv
    halo = cv.halo_enabled()
    yield cv
    cv.set_halo(halo)
    cv.set_halo_mtile(int(os.environ.get("APEX_AMD_CONV_HALO_BM", "0")))
    cv.set_nfast(int(os.environ.get("APEX_AMD_CONV_NFAST", "1")))
    cv.set_halo_nfast(int(os.environ.get("APEX_AMD_CONV_HALO_NFAST", "0")))
    cv.set_1x1_gemm4w(int(os.environ.get("APEX_AMD_CONV_1X1_G4W", "0")))
    cv.set_bnbwd_early(1)


def _rows(t):
    """[N, C, H, W] -> float64 [M, C] in raster (NHWC) order."""
    return t.double().permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _tile_sums(rows, bm):
    """float64 [C, ceil(M / bm)]: sums over consecutive runs of bm rows."""
    m, c = rows.shape
    t = (m + bm - 1) // bm
    pad = rows.new_zeros(t * bm, c)
    pad[:m] = rows
    return pad.view(t, bm, c).sum(1).t().contiguous()


def _assert_slab(slab, y, shift, bm):
    """The statistics slab [2][C][tiles] of the stored y: per-tile sums of (y - shift) and
    its square, exact; its width is the plan's M tile."""
    v = _rows(y)
    if shift is not None:
        v = v - shift.double()
    assert slab.shape == (2, y.shape[1], (v.shape[0] + bm - 1) // bm), (slab.shape, bm)
    assert torch.equal(slab[0].double(), _tile_sums(v, bm))
    assert torch.equal(slab[1].double(), _tile_sums(v * v, bm))


# ================================================================ a. conv_tap_k forward
# (id, N, Cin, H, W, Cout, ksize, stride, (BM, BN, BK, NB, folded at the default tile order))
FWD = [
    # 1x1 with one 64-channel K-tile: no ring (NB 1)
    ("nb1_below_one_tile", 1, 64, 5, 3, 128, 1, 1, (128, 128, 64, 1, False)),
    ("nb1_partial_grid6", 3, 64, 9, 11, 256, 1, 1, (128, 128, 64, 1, True)),
    ("nb1_image_1x1", 1, 64, 1, 1, 128, 1, 1, (128, 128, 64, 1, False)),
    ("nb1_image_1xW_grid3", 2, 64, 1, 7, 384, 1, 1, (128, 128, 64, 1, True)),
    # 128-wide tiles, 64-deep K-tiles on a 2-deep ring (grid < 1024)
    ("bk64_below_one_tile", 1, 128, 5, 3, 128, 1, 1, (128, 128, 64, 2, False)),
    ("bk64_3x3_partial", 3, 64, 9, 11, 128, 3, 1, (128, 128, 64, 2, False)),
    ("bk64_k256_grid8", 2, 256, 14, 14, 256, 1, 1, (128, 128, 64, 2, True)),
    ("bk64_3x3_image_1x1", 3, 128, 1, 1, 128, 3, 1, (128, 128, 64, 2, False)),
    ("bk64_3x3_image_1xW", 2, 64, 1, 9, 256, 3, 1, (128, 128, 64, 2, True)),
    ("bk64_3x3_grid9", 3, 64, 9, 11, 384, 3, 1, (128, 128, 64, 2, True)),
    # 128-wide tiles, 32-deep K-tiles on a 3-deep ring (grid >= 1024)
    ("bk32_1x1_256_tiles_last_partial", 1, 128, 181, 181, 512, 1, 1, (128, 128, 32, 3, True)),
    ("bk32_3x3_512_tiles", 1, 64, 255, 257, 256, 3, 1, (128, 128, 32, 3, True)),
    # 4 N tiles over >= 1024 M tiles keep M fastest (the unfolded exception)
    ("unfolded_1024_tiles", 1, 128, 362, 362, 512, 1, 1, (128, 128, 32, 3, False)),
    # 64-wide tiles
    ("w64_c64_3x3", 2, 64, 9, 11, 64, 3, 1, (128, 64, 32, 3, False)),
    ("w64_c192_1x1_grid9", 3, 128, 9, 11, 192, 1, 1, (128, 64, 32, 3, True)),
    ("w64_c64_cin64_below_one_tile", 1, 64, 5, 3, 64, 1, 1, (128, 64, 32, 3, False)),
    ("w64_c192_3x3_image_1xW", 1, 64, 1, 5, 192, 3, 1, (128, 64, 32, 3, True)),
    ("w64_c64_3x3_image_1x1", 3, 64, 1, 1, 64, 3, 1, (128, 64, 32, 3, False)),
    ("w64_c192_1x1_image_1x1", 1, 128, 1, 1, 192, 1, 1, (128, 64, 32, 3, True)),
    # stride 2 on odd H, W
    ("s2_3x3_odd", 2, 64, 9, 11, 128, 3, 2, (128, 128, 64, 2, False)),
    ("s2_1x1_odd_w64", 2, 128, 9, 11, 64, 1, 2, (128, 64, 32, 3, False)),
    ("s2_1x1_nb1", 3, 64, 9, 11, 128, 1, 2, (128, 128, 64, 1, False)),
    ("s2_3x3_w64_grid15", 5, 64, 19, 21, 192, 3, 2, (128, 64, 32, 3, True)),
]


def make_fwd(case, device):
    """(x, w, float64 reference) of a forward table row; conditions asserted."""
    name, n, ci, h, w, co, k, st = case[:8]
    g = cr.gen(_seed(name), device)
    x = cr.act(n, ci, h, w, g)
    wt = cr.weight(co, ci, k, g)
    ref = cr.conv_fwd(x, wt, st)
    cr.check_output(ref, extra=2.0, shift=torch.full((1,), 2.0))
    return x, wt, ref


def _folded(nfast, mtiles, ntiles):
    return ntiles > 1 and (nfast == 2 or (nfast == 1 and not (ntiles == 4 and mtiles >= 1024)))


@pytest.mark.parametrize("case", FWD, ids=[c[0] for c in FWD])
def test_conv_tap_forward_exact(case, sw):
    name, n, ci, h, w, co, k, st, plan = case
    bm, bn, bk, nb, folded = plan
    x, wt, ref = make_fwd(case, dev)
    want = cr.rounded(ref, BF)
    m = ref.shape[0] * ref.shape[2] * ref.shape[3]
    g = cr.gen(_seed(name) + 1, dev)
    shift = cr.ints((co,), g, F32)
    sw.set_halo(0)
    outs = []
    for nfast in (1, 0, 2):
        sw.set_nfast(nfast)
        got = sw.tap_plan("fwd", n, h, w, ci, co, k, st)
        fold = _folded(nfast, (m + bm - 1) // bm, co // bn)
        assert got == ("conv_tap_k", bm, bn, bk, nb, False, fold), (nfast, got)
        if nfast == 1:
            assert fold == folded, "the table names another tile order"
        y = sw.conv_fwd(x, wt, st)
        assert torch.equal(y, want), (nfast, float((y.double() - ref).abs().max()))
        y1, slab1 = sw.conv_fwd_stats(x, wt, st, shift)
        y0, slab0 = sw.conv_fwd_stats(x, wt, st, None)
        assert torch.equal(y1, want) and torch.equal(y0, want)
        _assert_slab(slab1, want, shift, bm)
        _assert_slab(slab0, want, None, bm)
        if k == 1 and st == 1 and sw.recompute_1x1_ok(m, ci, co):
            _, only = sw.conv1x1_stats_only(x, wt, shift)
            assert torch.equal(only, slab1), "stats-only launch differs from the plain slab"
        outs.append((y, slab1, slab0))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], o))


# ================================================================ b. data gradients
# stride-2 data gradient in one launch over the 4 parity classes.
# (id, N, C of dY, Ho, Wo, C of dX, ksize, (BM, BN, BK, NB, folded)); dX is [N, C, 2 Ho, 2 Wo]
DGRAD_S2 = [
    ("d3_3x5_w64", 1, 64, 3, 5, 64, 3, (128, 64, 32, 3, False)),
    ("d3_two_tiles", 3, 128, 7, 9, 128, 3, (128, 128, 64, 2, False)),
    ("d3_folded", 3, 64, 3, 5, 256, 3, (128, 128, 64, 2, True)),
    ("d3_w64_c192", 2, 128, 5, 7, 192, 3, (128, 64, 32, 3, True)),
    ("d1_3x5", 2, 64, 3, 5, 128, 1, (128, 128, 64, 2, False)),
    ("d1_w64_c192", 3, 128, 7, 9, 192, 1, (128, 64, 32, 3, True)),
    ("d3_grid_1024", 1, 64, 181, 181, 128, 3, (128, 128, 32, 3, False)),
    ("d1_grid_1024", 1, 128, 181, 181, 128, 1, (128, 128, 32, 3, False)),
]


def make_dgrad(case, device):
    """(dy, forward filter w [C_dY, C_dX, k, k], float64 dX) of a DGRAD_S2 row."""
    name, n, cdy, ho, wo, cdx, k = case[:7]
    g = cr.gen(_seed(name), device)
    dy = cr.act(n, cdy, ho, wo, g)
    wt = cr.weight(cdy, cdx, k, g, col_dim=1)
    ref = cr.conv_dgrad(dy, wt, 2 * ho, 2 * wo, 2)
    cr.check_output(ref)
    return dy, wt, ref


@pytest.mark.parametrize("case", DGRAD_S2, ids=[c[0] for c in DGRAD_S2])
def test_dgrad_stride2_exact(case, sw):
    name, n, cdy, ho, wo, cdx, k, plan = case
    bm, bn, bk, nb, folded = plan
    dy, wt, ref = make_dgrad(case, dev)
    want = cr.rounded(ref, BF)
    wprep = sw.rot_weight(wt) if k == 3 else sw.transpose_weight(wt)
    mt = (n * ho * wo + bm - 1) // bm
    if "grid_1024" in name:
        assert 4 * mt * (cdx // bn) >= 1024
    outs = []
    for nfast in (1, 0, 2):
        sw.set_nfast(nfast)
        got = sw.tap_plan("dgrad_s2", n, 2 * ho, 2 * wo, cdx, cdy, k, 2)
        fold = _folded(nfast, mt, cdx // bn)
        assert got == ("conv_tap_k", bm, bn, bk, nb, False, fold), (nfast, got)
        if nfast == 1:
            assert fold == folded
        dx = sw.conv_dgrad_s2(dy, wprep, 2 * ho, 2 * wo)
        assert torch.equal(dx, want), (nfast, float((dx.double() - ref).abs().max()))
        outs.append(dx)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


DGRAD_S1 = (2, 64, 128, 9, 11)      # (N, Cin, Cout, H, W) of the forward conv


def make_dgrad_s1(device):
    """(dy, forward filter, float64 dX) of the stride-1 3x3 data-gradient case."""
    n, ci, co, h, w = DGRAD_S1
    g = cr.gen(_seed("dgrad_s1"), device)
    dy = cr.act(n, co, h, w, g)
    wt = cr.weight(co, ci, 3, g, col_dim=1)
    ref = cr.conv_dgrad(dy, wt, h, w, 1)
    cr.check_output(ref)
    return dy, wt, ref


@pytest.mark.parametrize("halo", [0, 1])
def test_dgrad_stride1_through_rot_weight_exact(halo, sw):
    """The stride-1 3x3 data gradient is conv_fwd of dY with the rotated filter."""
    n, ci, co, h, w = DGRAD_S1
    dy, wt, ref = make_dgrad_s1(dev)
    sw.set_halo(halo)
    assert sw.tap_plan("fwd", n, h, w, co, ci, 3, 1)[0] == ("conv3h_k" if halo else "conv_tap_k")
    dx = sw.conv_fwd(dy, sw.rot_weight(wt), 1)
    assert torch.equal(dx, cr.rounded(ref, BF))
    # the batched layout kernel writes the same filters
    prep = sw.prep_weights([wt])
    assert torch.equal(prep[0], sw.rot_weight(wt))


# ================================================================ d. BN-backward epilogue
def make_bn_operands(case, ref, device):
    """Integer BN operands for which the epilogue's arithmetic stays exact: x and the
    residual in [-2, 2], integer mean and bias, invstd and weight powers of two (so is
    their product); (xbn, add, mean, invstd, bn_w, bn_b, float64 keep mask of relu_mode 2)."""
    name = case[0]
    n, co, h, w = ref.shape
    g = cr.gen(_seed(name) + 7, device)
    xbn = cr.act(n, co, h, w, g)
    add = cr.act(n, co, h, w, g)
    mean = cr.ints((co,), g, F32)
    bn_b = cr.ints((co,), g, F32)
    invstd = torch.pow(2.0, torch.randint(-2, 2, (co,), generator=g, device=g.device).float())
    bn_w = torch.pow(2.0, torch.randint(-1, 3, (co,), generator=g, device=g.device).float())
    sc = (invstd * bn_w).double().view(1, -1, 1, 1)
    pre = xbn.double() * sc + (bn_b.double() - mean.double() * sc.view(-1)).view(1, -1, 1, 1)
    cr.check_output(ref, extra=2.0)
    # sum(g * (x - mean)) over up to 256 rows
    assert 256 * (float(ref.abs().max()) + 2) * 4 < cr.LIM_ACC
    return xbn, add, mean, invstd, bn_w, bn_b, pre > 0


def _assert_bnbwd(cv, dy, wt, ref, ops, bm):
    """g and the slab of conv_fwd_bnbwd for relu_mode 0 / 2, with and without a residual."""
    xbn, add, mean, invstd, bn_w, bn_b, keep = ops
    xm = _rows(xbn) - mean.double()
    res = []
    for mode in (0, 2):
        for a in (None, add):
            o = ref if a is None else ref + a.double()
            want = cr.rounded(o if mode == 0 else torch.where(keep, o, torch.zeros_like(o)), BF)
            g, slab = cv.conv_fwd_bnbwd(dy, wt, a, xbn, None, mean, invstd, bn_w, bn_b, mode)
            assert torch.equal(g, want), (mode, a is not None)
            gr = _rows(want)
            assert slab.shape == (2, ref.shape[1], (gr.shape[0] + bm - 1) // bm), (slab.shape, bm)
            assert torch.equal(slab[0].double(), _tile_sums(gr, bm)), (mode, a is not None)
            assert torch.equal(slab[1].double(), _tile_sums(gr * xm, bm)), (mode, a is not None)
            res += [g, slab]
    return res


# (id, N, C of dY, H, W, C of g, ksize, 1, (BM, BN, BK, NB, folded), early with the switch on)
BNBWD = [
    ("bm64_k64_partial", 1, 64, 224, 225, 128, 1, 1, (64, 128, 32, 3, False), True),
    ("bm64_k128_folded", 1, 128, 224, 224, 256, 1, 1, (64, 128, 32, 3, True), True),
    ("bm64_k192", 1, 192, 224, 225, 128, 1, 1, (64, 128, 32, 3, False), False),
    ("bm128_k256", 1, 256, 224, 225, 128, 1, 1, (128, 128, 64, 2, False), False),
    ("bm128_below_50176", 1, 64, 223, 225, 128, 1, 1, (128, 128, 64, 1, False), False),
    ("bm128_small", 3, 128, 9, 11, 128, 1, 1, (128, 128, 64, 2, False), False),
    ("bm128_w64", 3, 128, 9, 11, 192, 1, 1, (128, 64, 32, 3, True), False),
    ("bm128_3x3_tap", 3, 64, 9, 11, 128, 3, 1, (128, 128, 64, 2, False), False),
]


@pytest.mark.parametrize("case", BNBWD, ids=[c[0] for c in BNBWD])
def test_bnbwd_epilogue_conv_tap_exact(case, sw):
    name, n, ci, h, w, co, k, _, plan, early = case
    bm, bn, bk, nb, folded = plan
    dy, wt, ref = make_fwd(case[:9], dev)
    ops = make_bn_operands(case, ref, dev)
    sw.set_halo(0)
    runs = []
    for on in (1, 0):
        sw.set_bnbwd_early(on)
        got = sw.tap_plan("bnbwd", n, h, w, ci, co, k, 1)
        assert got == ("conv_tap_k", bm, bn, bk, nb, bool(on) and early, folded), (on, got)
        runs.append(_assert_bnbwd(sw, dy, wt, ref, ops, bm))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


ADD_S2 = ("bnbwd_add_s2", 2, 128, 10, 12, 128, 1, 1, None)


def make_add_s2(device):
    """(dy, w, BN operands, compact residual, float64 conv + residual on the even pixels)."""
    dy, wt, ref = make_fwd(ADD_S2, device)
    ops = make_bn_operands(ADD_S2, ref, device)
    g = cr.gen(_seed("add_s2"), device)
    add = cr.act(2, 128, 5, 6, g)
    o = ref.clone()
    o[:, :, ::2, ::2] += add.double()
    cr.check_output(o)
    return dy, wt, ops, add, o


def test_bnbwd_epilogue_stride2_residual_exact(sw):
    """relu_mode 0 with the COMPACT residual of a stride-2 1x1 conv (even pixels only)."""
    dy, wt, (xbn, _, mean, invstd, bn_w, bn_b, _), add, o = make_add_s2(dev)
    want = cr.rounded(o, BF)
    got, slab = sw.conv_fwd_bnbwd(dy, wt, add, xbn, None, mean, invstd, bn_w, bn_b, 0, True)
    assert torch.equal(got, want)
    gr = _rows(want)
    assert torch.equal(slab[0].double(), _tile_sums(gr, 128))
    assert torch.equal(slab[1].double(), _tile_sums(gr * (_rows(xbn) - mean.double()), 128))


_DGRAD3 = [c for c in DGRAD_S2 if c[6] == 3]


@pytest.mark.parametrize("case", _DGRAD3, ids=[c[0] for c in _DGRAD3])
def test_dgrad_stride2_bnbwd_epilogue_exact(case, sw):
    """conv_dgrad_s2_bnbwd (3x3): g = mask * dX exact for relu_mode 0 and 2, and the slab
    [2][C][4 classes x M tiles] holds each parity class's per-tile sums of g and g (x - mean)
    (class z = 2 ph + pw owns the pixels (2a + ph, 2b + pw), rows in (n, a, b) order)."""
    name, n, cdy, ho, wo, cdx, k, plan = case
    bm, bn, bk, nb, folded = plan
    dy, wt, ref = make_dgrad(case, dev)
    xbn, _, mean, invstd, bn_w, bn_b, keep = make_bn_operands(case, ref, dev)
    assert sw.tap_plan("dgrad_s2_bnbwd", n, 2 * ho, 2 * wo, cdx, cdy, 3, 2) == (
        "conv_tap_k", bm, bn, bk, nb, False, folded)
    wrot = sw.rot_weight(wt)
    xm = xbn.double() - mean.double().view(1, -1, 1, 1)
    for mode in (0, 2):
        want = cr.rounded(ref if mode == 0 else torch.where(keep, ref, torch.zeros_like(ref)), BF)
        g, slab = sw.conv_dgrad_s2_bnbwd(dy, wrot, 2 * ho, 2 * wo, xbn, None, mean, invstd,
                                         bn_w, bn_b, mode)
        assert torch.equal(g, want), mode
        s0, s1 = [], []
        for ph in (0, 1):
            for pw in (0, 1):
                gz = want.double()[:, :, ph::2, pw::2]
                s0.append(_tile_sums(_rows(gz), bm))
                s1.append(_tile_sums(_rows(gz * xm[:, :, ph::2, pw::2]), bm))
        assert slab.shape == (2, cdx, 4 * ((n * ho * wo + bm - 1) // bm)), slab.shape
        assert torch.equal(slab[0].double(), torch.cat(s0, 1)), mode
        assert torch.equal(slab[1].double(), torch.cat(s1, 1)), mode


# ================================================================ c. conv3h_k (halo)
def test_halo_table_reaches_every_conv3h_plan(sw):
    """Host query only: the shapes x switches below run all three conv3h_k instantiations."""
    assert set(HALO_BN) == set(HALO_SHAPES)
    seen = {(bm, bn) for row in HALO_BN.values()
            for (_, bm), bn in zip(HALO_SWITCHES, row) if bn is not None}
    assert seen == {(256, 128), (224, 128), (256, 64)}, seen
    for (n, ci, h, w, co), row in HALO_BN.items():
        for (mode, bm), bn in zip(HALO_SWITCHES, row):
            sw.set_halo_mtile(bm)
            sw.set_halo(mode)
            p = sw.tap_plan("fwd", n, h, w, ci, co, 3, 1)
            assert p[:3] == (("conv3h_k", bm, bn) if bn else ("conv_tap_k", 128, p[2])), p


@pytest.mark.parametrize("mode,bm", HALO_SWITCHES)
@pytest.mark.parametrize("shape", HALO_SHAPES)
def test_conv3h_exact(shape, mode, bm, sw):
    n, ci, h, w, co = shape
    want_bn = HALO_BN[shape][HALO_SWITCHES.index((mode, bm))]
    case = ("halo", n, ci, h, w, co, 3, 1, None)
    x, wt, ref = make_fwd(case, dev)
    want = cr.rounded(ref, BF)
    ops = make_bn_operands(case, ref, dev)
    g = cr.gen(_seed(shape), dev)
    shift = cr.ints((co,), g, F32)
    m = n * h * w

    sw.set_halo(0)
    tap = [sw.conv_fwd(x, wt, 1), *sw.conv_fwd_stats(x, wt, 1, shift)]
    assert sw.tap_plan("fwd", n, h, w, ci, co, 3, 1)[0] == "conv_tap_k"
    assert torch.equal(tap[0], want) and torch.equal(tap[1], want)
    _assert_slab(tap[2], want, shift, 128)

    sw.set_halo_mtile(bm)
    sw.set_halo(mode)
    halo = want_bn is not None
    runs = []
    for nf in (0, 1):
        sw.set_halo_nfast(nf)
        p = sw.tap_plan("fwd", n, h, w, ci, co, 3, 1)
        pb = sw.tap_plan("bnbwd", n, h, w, ci, co, 3, 1)
        if halo:
            assert p[:6] == ("conv3h_k", bm, want_bn, 32, 3, False), p
            assert p[6] == (nf == 1 and co // want_bn > 1)
            assert pb == p
        else:
            assert p[0] == "conv_tap_k" and p[1] == 128, p
        tile = p[1]
        y = sw.conv_fwd(x, wt, 1)
        y1, slab = sw.conv_fwd_stats(x, wt, 1, shift)
        # exact, hence bitwise the per-tap kernel's output as well
        assert torch.equal(y, want) and torch.equal(y1, want) and torch.equal(y, tap[0])
        _assert_slab(slab, want, shift, tile)
        assert slab.shape[2] == (m + tile - 1) // tile
        runs.append([y, slab] + _assert_bnbwd(sw, x, wt, ref, ops, tile))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ================================================================ e. weight gradients
# per-tap kernel: (algo, Cin, Cout, ksize, stride, (N, H, W, S) with S <= 16: single-pass
# reduce, (N, H, W, S) with S > 16: two-stage) - S as conv.wgrad_splits chooses it
WGRAD_TAP = [
    (0, 128, 128, 3, 1, (3, 13, 15, 3), (7, 29, 31, 20)),
    (0, 128, 128, 3, 2, (5, 21, 19, 2), (12, 57, 59, 24)),
    (0, 128, 128, 1, 1, (3, 13, 15, 3), (7, 29, 31, 25)),
    (0, 128, 128, 1, 2, (5, 21, 19, 2), (9, 45, 47, 20)),
    (2, 128, 128, 3, 1, (2, 9, 11, 2), (7, 29, 31, 18)),
    (2, 128, 128, 3, 2, (5, 21, 19, 5), (12, 57, 59, 22)),
    (2, 128, 128, 1, 1, (2, 9, 11, 2), (7, 29, 31, 50)),
    (2, 128, 128, 1, 2, (5, 21, 19, 5), (8, 37, 35, 22)),
    (3, 128, 128, 3, 1, (3, 13, 15, 3), (8, 37, 35, 18)),
    (3, 128, 128, 3, 2, (5, 21, 19, 2), (16, 61, 63, 21)),
    (3, 128, 128, 1, 1, (3, 13, 15, 3), (7, 29, 31, 25)),
    (3, 128, 128, 1, 2, (5, 21, 19, 2), (9, 45, 47, 20)),
    (5, 128, 128, 3, 1, (2, 9, 11, 2), (7, 29, 31, 18)),
    (5, 128, 128, 3, 2, (5, 21, 19, 5), (12, 57, 59, 22)),
    (5, 128, 128, 1, 1, (2, 9, 11, 2), (7, 29, 31, 50)),
    (5, 128, 128, 1, 2, (5, 21, 19, 5), (8, 37, 35, 22)),
    (0, 64, 128, 3, 1, (5, 21, 19, 4), (8, 37, 35, 17)),
    (0, 64, 128, 3, 2, (7, 29, 31, 4), (12, 57, 59, 17)),
    (0, 64, 128, 1, 1, (5, 21, 19, 4), (8, 37, 35, 21)),
    (0, 64, 128, 1, 2, (7, 29, 31, 4), (12, 57, 59, 21)),
    (2, 64, 128, 3, 1, (3, 13, 15, 3), (8, 37, 35, 18)),
    (2, 64, 128, 3, 2, (5, 21, 19, 2), (16, 61, 63, 21)),
    (2, 64, 128, 1, 1, (3, 13, 15, 3), (7, 29, 31, 25)),
    (2, 64, 128, 1, 2, (5, 21, 19, 2), (9, 45, 47, 20)),
    # (64 -> 128 has 18 workgroups per split on this plan and the cost model stops at 14
    # splits; 64 -> 64, 9 per split, goes further: that pair carries the two-stage case)
    (3, 64, 128, 3, 1, (5, 21, 19, 4), None),
    (3, 64, 128, 3, 2, (7, 29, 31, 4), None),
    (3, 64, 64, 3, 1, (5, 21, 19, 4), (8, 55, 57, 28)),
    (3, 64, 64, 3, 2, (7, 29, 31, 4), (32, 55, 57, 26)),
    (3, 64, 128, 1, 1, (5, 21, 19, 4), (8, 37, 35, 21)),
    (3, 64, 128, 1, 2, (7, 29, 31, 4), (12, 57, 59, 21)),
    (5, 64, 128, 3, 1, (5, 21, 19, 4), (8, 37, 35, 17)),
    (5, 64, 128, 3, 2, (7, 29, 31, 4), (12, 57, 59, 17)),
    (5, 64, 128, 1, 1, (5, 21, 19, 4), (8, 37, 35, 21)),
    (5, 64, 128, 1, 2, (7, 29, 31, 4), (12, 57, 59, 21)),
]
WGRAD_TILE = {  # (algo, all channels % 128) -> (BM, BN, BK, NB) of wg_tap_cfg
    (0, True): (128, 128, 64, 2), (2, True): (128, 128, 32, 4), (3, True): (128, 128, 64, 3),
    (5, True): (128, 128, 32, 3), (0, False): (64, 64, 128, 2), (2, False): (64, 64, 64, 3),
    (3, False): (64, 64, 128, 3), (5, False): (64, 64, 128, 2),
}
# strip kernels (3x3 stride 1, W <= 56): (algo, Cin, Cout, N, H, W, S)
WGRAD_STRIP = [
    (1, 64, 64, 2, 56, 56, 12),       # W = 56
    (1, 64, 64, 3, 4, 1, 1),          # W = 1
    (1, 64, 192, 2, 8, 8, 1),
    (1, 64, 64, 8, 30, 30, 15),       # 8 K-tiles per split, 15 per image: ranges cross images
    (1, 64, 64, 10, 30, 30, 18),      # two-stage reduce
    (1, 128, 64, 3, 14, 56, 4),
    (4, 64, 64, 2, 56, 56, 2),        # W = 56
    (4, 64, 64, 3, 4, 1, 3),          # W = 1
    (4, 64, 64, 2, 1, 1, 2),
    (4, 256, 256, 20, 5, 7, 16),      # one K-tile per image, two per split: boundary inside
    (4, 128, 128, 70, 5, 7, 64),      # two-stage reduce, boundaries inside the ranges
    (4, 64, 64, 20, 9, 9, 20),        # two-stage reduce, whole images
    (4, 128, 64, 3, 14, 56, 3),
]


def wgrad_cases():
    """(id, algo, Cin, Cout, ksize, stride, N, H, W, S) of every weight-gradient case."""
    for algo, ci, co, k, st, small, big in WGRAD_TAP:
        for tag, shp in (("one_pass", small), ("two_stage", big)):
            if shp is not None:
                n, h, w, s = shp
                yield ("tap%d_%dx%d_k%ds%d_%s" % (algo, ci, co, k, st, tag), algo, ci, co, k, st,
                       n, h, w, s)
    for algo, ci, co, n, h, w, s in WGRAD_STRIP:
        yield ("strip%d_%dx%d_n%d_%dx%d" % (algo, ci, co, n, h, w), algo, ci, co, 3, 1, n, h, w, s)


def make_wgrad(case, device):
    """(dy, x, float64 dW) of a weight-gradient case; conditions asserted."""
    name, algo, ci, co, k, st, n, h, w, s = case
    g = cr.gen(_seed((ci, co, k, st, n, h, w)), device)
    x = cr.act(n, ci, h, w, g)
    dy = cr.thin_dy(n, co, (h - 1) // st + 1, (w - 1) // st + 1, g)
    ref = cr.conv_wgrad(dy, x, k, st)
    cr.check_wgrad(dy, x, ref)
    assert float(ref.abs().max()) + 512 < cr.LIM_ACC       # + the accumulation target
    return dy, x, ref


_WG = list(wgrad_cases())


@pytest.mark.parametrize("case", _WG, ids=[c[0] for c in _WG])
def test_conv_wgrad_exact(case):
    name, algo, ci, co, k, st, n, h, w, s = case
    cv = _C().conv
    assert cv.wgrad_splits(n, h, w, ci, co, k, st, algo) == s, "the table names another split"
    if algo not in (1, 4):
        assert (s > 16) == ("two_stage" in name)
        tile = WGRAD_TILE[(algo, ci % 128 == 0 and co % 128 == 0)]
        assert cv.wgrad_tap_tile(ci, co, algo) == tile
    dy, x, ref = make_wgrad(case, dev)
    g = cr.gen(_seed(name) + 3, dev)
    for dt in (F32, BF):
        got = cv.conv_wgrad(dy, x, dt, algo, st, k)
        assert got.shape == ref.shape and got.dtype == dt
        assert torch.equal(got, cr.rounded(ref, dt)), (dt, float((got.double() - ref).abs().max()))
        # accumulate: ONE rounding of out_prev + sum (exact in fp32: integers)
        prev = torch.randint(-300, 301, ref.shape, generator=g, device=dev).to(dt)
        prev = prev.contiguous(memory_format=CL)
        acc = prev.clone(memory_format=torch.preserve_format)
        r = cv.conv_wgrad(dy, x, dt, algo, st, k, out=acc, accumulate=True)
        assert r.data_ptr() == acc.data_ptr()
        assert torch.equal(acc, cr.rounded(prev.double() + ref, dt)), dt
        # overwrite: whatever the target held (NaN) is gone
        over = torch.full_like(prev, float("nan"))
        cv.conv_wgrad(dy, x, dt, algo, st, k, out=over, accumulate=False)
        assert torch.equal(over, cr.rounded(ref, dt)), dt


@pytest.mark.parametrize("S", [1, 11, 16, 17, 37])
def test_splitk_reduce_exact(S):
    cv = _C().conv
    g = cr.gen(100 + S, dev)
    part = torch.randint(-1000, 1001, (S, 96, 40), generator=g, device=dev).float()
    ref = part.double().sum(0)
    for dt in (F32, BF):
        assert torch.equal(cv.splitk_reduce(part, dt), ref.to(dt))
        prev = torch.randint(-300, 301, (96, 40), generator=g, device=dev).to(dt)
        acc = prev.clone()
        cv.splitk_reduce(part, dt, acc, True)
        assert torch.equal(acc, (prev.double() + ref).to(dt))
        over = torch.full_like(prev, float("nan"))
        cv.splitk_reduce(part, dt, over, False)
        assert torch.equal(over, ref.to(dt))


# ================================================================ f. stem 7x7 / 2
# (N, H, W).  Output-row widths Wo = 16, 125, 1, 18, 50, 80, 4 reach every 16-pixel block
# count of stem_fwd_k (1, 8, 1, 2, 4, 7, 1) and every 32-pixel k-step count of stem_wgrad_k
# (1, 4, 1, 1, 2, 3, 1); N * H / 2 = 32, 18, 1, 15, 3, 2 rows fill the 8 waves of a workgroup
# exactly, partly or hardly; 2079 rows are more than the forward grid's 2048 waves: 2 rows
# per wave and 5 per weight-gradient workgroup (416 splits, two-stage reduce), and with 231
# rows per image both kernels' row runs cross image boundaries
STEM = [(2, 32, 32), (2, 18, 250), (1, 2, 2), (3, 10, 36), (1, 6, 100), (1, 4, 160),
        (9, 462, 8)]
# shape -> (statistics slab columns = waves of the forward grid, output rows per wave)
STEM_SLAB = {(2, 32, 32): (32, 1), (2, 18, 250): (24, 1), (1, 2, 2): (8, 1),
             (3, 10, 36): (16, 1), (1, 6, 100): (8, 1), (1, 4, 160): (8, 1),
             (9, 462, 8): (2048, 2)}


def make_stem(shape, device):
    """(x, w, dy, shift, float64 y, float64 dW) of a stem case."""
    n, h, w = shape
    g = cr.gen(_seed(shape), device)
    x = cr.act(n, 3, h, w, g)
    wt = cr.weight(64, 3, 7, g)
    dy = cr.thin_dy(n, 64, h // 2, w // 2, g)
    shift = cr.ints((64,), g, F32)
    ref = cr.conv_fwd(x, wt, 2, 3)
    cr.check_output(ref, extra=2.0)
    # integers: |v| <= v^2, so the whole channel's sum of squares bounds every partial sum
    v = ref.abs() + 2
    assert float((v * v).sum((0, 2, 3)).max()) < cr.LIM_ACC
    dw = cr.conv_wgrad(dy, x, 7, 2, 3)
    cr.check_wgrad(dy, x, dw)
    return x, wt, dy, shift, ref, dw


@pytest.mark.parametrize("shape", STEM)
def test_stem_exact(shape):
    from apex_example_amd.ops.conv import _pack_stem_weight
    cv = _C().conv
    n, h, w = shape
    x, wt, dy, shift, ref, dw = make_stem(shape, dev)
    rows = n * (h // 2)
    if shape == (3, 10, 36):
        assert rows % 8 != 0, "rows are to leave the last workgroup's waves partly idle"
    want = cr.rounded(ref, BF)
    xp = cv.stem_pad(x)
    wk = _pack_stem_weight(wt)                          # zeros in the lanes c = 3 and s = 7
    y = cv.stem_fwd(xp, wk)
    assert torch.equal(y, want), float((y.double() - ref).abs().max())
    cols, rpw = STEM_SLAB[shape]
    wo = w // 2
    for sh in (shift, None):
        y1, slab = cv.stem_fwd_stats(xp, wk, sh)
        assert torch.equal(y1, want)
        assert slab.shape == (2, 64, cols), slab.shape
        # column s = wave s = output rows [s * rpw, (s + 1) * rpw) in (n, ho) order; the
        # waves past the last row write zeros
        v = _rows(want) if sh is None else _rows(want) - sh.double()
        for k, q in enumerate((v, v * v)):
            per_wave = _tile_sums(q.reshape(rows, wo, 64).sum(1), rpw)
            exp = per_wave.new_zeros(64, cols)
            exp[:, :per_wave.shape[1]] = per_wave
            assert torch.equal(slab[k].double(), exp), (k, sh is not None)
    S = cv.stem_wgrad_splits(n, h)
    assert (S > 16) == (rows > 16)
    part = cv.stem_wgrad(xp, dy)
    got = part.view(64, 8, 8, 4)[:, :7, :7, :3].permute(0, 3, 1, 2)
    assert torch.equal(got.double(), dw)


# ================================================================ g. gemm4w / wgrad4w
G4W_M = [1, 255, 257, 1000]
G4W_K = [64, 1088]
# (T, M, N, S): T / S = 64 rows per split (one K-tile) for S = 1, 2, 4, and a longer one
W4W = [(64, 256, 256, 1), (128, 256, 512, 2), (256, 512, 256, 4), (2048, 256, 512, 4)]


def make_gemm(m, n, k, dtype, device):
    g = cr.gen(_seed(("gemm", m, n, k)), device)
    a = cr.ints((m, k), g, dtype)
    b = cr.thin_ints((n, k), k, 0, g, dtype)
    ref = cr.abt(a, b)
    cr.check_output(ref)
    return a, b, ref


def make_w4w(t, m, n, device, dtype=BF):
    g = cr.gen(_seed(("w4w", t, m, n)), device)
    dy = cr.thin_ints((t, m), t, 1, g, dtype)
    x = cr.ints((t, n), g, dtype)
    ref = cr.atb(dy, x)
    assert float(dy.double().abs().sum(0).max()) * 2 + 512 < cr.LIM_ACC
    return dy, x, ref


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("k", G4W_K)
@pytest.mark.parametrize("m", G4W_M)
def test_gemm4w_exact(m, k, dtype):
    dn = _C().dense
    a, b, ref = make_gemm(m, 512, k, dtype, dev)
    assert dn.gemm4w_ok(a, b)
    c, = dn.gemm4w(a, b)
    assert c.dtype == dtype and torch.equal(c, ref.to(dtype))


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("tmns", W4W)
def test_wgrad4w_exact(tmns, dtype):
    dn = _C().dense
    t, m, n, s = tmns
    dy, x, ref = make_w4w(t, m, n, dev, dtype)
    assert dn.wgrad4w_ok(dy, x, s)
    g = cr.gen(_seed(tmns) + 1, dev)
    for dt in ((F32, BF) if dtype == BF else (F32,)):
        w = dn.wgrad4w(dy, x, s, dt)
        assert torch.equal(w, ref.to(dt))
        prev = torch.randint(-300, 301, (m, n), generator=g, device=dev).to(dt)
        acc = prev.clone()
        dn.wgrad4w(dy, x, s, dt, out=acc, accumulate=True)
        assert torch.equal(acc, (prev.double() + ref).to(dt))
        over = torch.full_like(prev, float("nan"))
        dn.wgrad4w(dy, x, s, dt, out=over, accumulate=False)
        assert torch.equal(over, ref.to(dt))
        wb, db = dn.wgrad4w_bias(dy, x, s, dt, bias_dtype=F32)
        assert torch.equal(wb, ref.to(dt))
        assert torch.equal(db.double(), dy.double().sum(0))


# stride-1 1x1 forwards routed to gemm4w (statistics epilogue, EPI 3): (N, Cin, H, W, Cout)
G4W_CONV = [(2, 64, 30, 17, 256), (1, 1024, 9, 9, 256), (2, 128, 14, 14, 512), (1, 64, 1, 1, 256)]


@pytest.mark.parametrize("shape", G4W_CONV)
def test_conv1x1_on_gemm4w_exact(shape, sw):
    n, ci, h, w, co = shape
    x, wt, ref = make_fwd(("g4w", n, ci, h, w, co, 1, 1, None), dev)
    want = cr.rounded(ref, BF)
    g = cr.gen(_seed(shape), dev)
    shift = cr.ints((co,), g, F32)
    sw.set_1x1_gemm4w(0)
    own = sw.conv_fwd(x, wt, 1)
    assert sw.tap_plan("fwd", n, h, w, ci, co, 1, 1)[0] == "conv_tap_k"
    sw.set_1x1_gemm4w(2)
    assert sw.tap_plan("fwd", n, h, w, ci, co, 1, 1)[:3] == ("gemm4w", 256, 256)
    y = sw.conv_fwd(x, wt, 1)
    assert torch.equal(y, want) and torch.equal(y, own)
    for sh in (shift, None):
        y1, slab = sw.conv_fwd_stats(x, wt, 1, sh)
        assert torch.equal(y1, want)
        _assert_slab(slab, want, sh, 256)
