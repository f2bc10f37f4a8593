"""The float64 pooling references of tests/pool_ref.py are right (no GPU needed): they
agree with torch's max_pool2d in float64 and its autograd on tie-free, tied and special
(-inf / NaN / signed zero) inputs over every geometry the kernels are held to, the fused
stem backward agrees with autograd through max_pool2d(relu(batch_norm)), the float32
emulation of each documented algorithm stays below the bound, the BN pooling inputs leave
at least 99 % of the windows decided, the grid-stride shapes exceed the launch caps, and
each deliberately wrong variant misses the reference - which is how we know that
tests/test_pool_gpu.py would notice."""
import pytest
import torch
import torch.nn.functional as F

import pool_ref as R
from pool_ref import BF16, F16, F32, F64

GEOMS = R.geometries()
CS = [1, 5, 8]


def _eq(a, b, what):
    assert a.shape == b.shape, what
    assert torch.equal(a.isnan(), b.isnan()), what + ": NaN positions"
    assert torch.equal(a.nan_to_num(nan=7.0), b.nan_to_num(nan=7.0)), what


def _torch_pool(x64, dy, k, s, p):
    xd = x64.clone().requires_grad_(True)
    y = F.max_pool2d(xd, k, s, p)
    y.backward(dy.to(F64))
    return y.detach(), xd.grad


@pytest.mark.parametrize("geom", GEOMS, ids=R.geom_id)
def test_ref_matches_torch(geom):
    k, s, p, (H, W) = geom
    for C in CS:
        shape = (2, C, H, W)
        for maker in ("tie_free", "tied", "special"):
            x = {"tie_free": lambda: R.tie_free(shape, k, 1), "tied": lambda: R.tied(shape, 2),
                 "special": lambda: R.special(shape, k, 3)}[maker]()
            y, tap = R.ref_maxpool_fwd(x, k, s, p)
            dy = R.rand_dy(y.shape, 4)
            dx = R.ref_maxpool_bwd(dy, tap, H, W, k, s, p)
            # ATen's CPU kernel starts from the first in-bounds element and replaces on
            # (v > max) || isnan(v): with ONE NaN per tensor its routing is the reference's
            # stated rule on every input here, -inf windows and the NaN window included
            ty, tdx = _torch_pool(x.to(F64), dy, k, s, p)
            _eq(y, ty, "%s C=%d y" % (maker, C))
            _eq(dx.v, tdx, "%s C=%d dx" % (maker, C))
            # every gradient arrives somewhere
            assert float((dx.v.sum() - dy.to(F64).sum()).abs()) < 1e-9
            assert int(tap.max()) < k * k and int(tap.min()) >= 0


def test_special_covers_border_and_interior():
    """The -inf blocks make all--inf windows both where tap 0 is padding and where it is
    not, and the zero row has a window whose first maximum is -0."""
    x = R.special((2, 8, 9, 11), 3, 3)
    y, tap = R.ref_maxpool_fwd(x, 3, 2, 1)
    allinf = y == float("-inf")
    assert bool(allinf[0, 0, 0, 0]) and int(tap[0, 0, 0, 0]) == 4      # first in-bounds tap
    assert bool(allinf[:, :, 1:, 1:].any())                            # interior: tap 0
    assert bool((tap[allinf] == 0).any()) and bool((tap[allinf] != 0).any())
    assert bool(y.isnan().any())
    assert bool(((y == 0) & torch.signbit(y)).any())


@pytest.mark.parametrize("hw", [(8, 10), (9, 11), (7, 6), (1, 1), (2, 2)])
def test_bwd_bn_matches_autograd(hw):
    H, W = hw
    shape = (2, 8, H, W)
    inp = R.zero_channel(R.exact_ints(shape, 3, 2, 1, 5))
    x, dy = inp["x"].to(BF16), inp["dy"].to(BF16)
    mean, invstd, w, b = (inp[n] for n in ("mean", "invstd", "w", "b"))
    y, tap, pre = R.ref_maxpool_fwd(x, 3, 2, 1, bn=(mean, invstd, w, b))
    out = R.ref_maxpool_bwd_bn(dy, tap, x, mean, invstd, w, b)
    xd = x.to(F64).requires_grad_(True)
    cs = (1, -1, 1, 1)
    o = (xd - mean.to(F64).view(cs)) * invstd.to(F64).view(cs) * w.to(F64).view(cs) \
        + b.to(F64).view(cs)
    r = torch.relu(o)
    o.retain_grad()
    r.retain_grad()
    yt = F.max_pool2d(r, 3, 2, 1)
    yt.backward(dy.to(F64))
    _eq(y, yt.detach(), "y")
    _eq(pre.v, r.detach(), "pre")
    _eq(out["dx"].v, r.grad, "dx")
    d = o.grad
    _eq(out["sum_dy"].v, d.sum((0, 2, 3)), "sum_dy")
    _eq(out["sum_dy_xmu"].v, (d * (xd.detach() - mean.to(F64).view(cs))).sum((0, 2, 3)),
        "sum_dy_xmu")
    assert float(out["sum_dy"].v[0]) == 0.0        # the channel at exactly zero


def test_gap_matches_autograd():
    torch.manual_seed(0)
    dy = torch.randn(3, 5).to(BF16)
    x = torch.zeros(3, 5, 4, 7, dtype=F64, requires_grad=True)
    x.mean((2, 3)).backward(dy.to(F64))
    torch.testing.assert_close(R.ref_gap_bwd(dy, 4, 7)["dx"].v, x.grad, rtol=1e-14, atol=0)


# ------------------------------------------------------------ the float32 emulation
def _bn_case(shape, dtype, seed, exact):
    if exact:
        inp = R.zero_channel(R.exact_ints(shape, 3, 2, 1, seed))
        x, dy = inp["x"].to(dtype), inp["dy"].to(dtype)
        bn = tuple(inp[n] for n in ("mean", "invstd", "w", "b"))
    else:
        x = R.bn_x(shape, 3, seed).to(dtype)
        bn = R.bn_params(shape[1], seed)
        dy = R.rand_dy((shape[0], shape[1], R.out_size(shape[2], 3, 2, 1),
                        R.out_size(shape[3], 3, 2, 1)), seed).to(dtype)
    return x, dy, bn


def test_emulation_ratio():
    torch.manual_seed(0)
    worst = {"dx": 0.0, "sum_dy": 0.0, "sum_dy_xmu": 0.0, "gap": 0.0}
    for k, s, p, (H, W) in GEOMS:
        for C in (5, 8):
            shape = (2, C, H, W)
            for x in (R.tie_free(shape, k, 1), R.tied(shape, 2), R.special(shape, k, 3)):
                _, tap = R.ref_maxpool_fwd(x, k, s, p)
                for dt in (F32, F16, BF16):
                    dy = R.rand_dy(tap.shape, 4).to(dt)
                    r = R.emulation_ratio(
                        lambda d, work: {"dx": R.ref_maxpool_bwd(d, tap, H, W, k, s, p, work)}, dy)
                    worst["dx"] = max(worst["dx"], r["dx"])
    for hw in [(8, 10), (9, 11), (31, 30)]:
        for dt in (F16, BF16):
            for exact in (False, True):
                shape = (3, 64, hw[0], hw[1])
                x, dy, bn = _bn_case(shape, dt, 6, exact)
                assert not bool(R.bnr_ambiguous(x, *bn).any()) or exact
                _, tap, _ = R.ref_maxpool_fwd(x, 3, 2, 1, bn=bn)
                stored = R.ref_maxpool_bwd(dy, tap, hw[0], hw[1], 3, 2, 1).v.to(dt)

                def fn(d, work):
                    o = R.ref_maxpool_bwd_bn(d, tap, x, *bn, dx_stored=stored, work=work)
                    return {n: o[n] for n in ("sum_dy", "sum_dy_xmu")}
                r = R.emulation_ratio(fn, dy)
                for n in r:
                    worst[n] = max(worst[n], r[n])
    for dt in (F32, F16, BF16):
        dy = torch.randn(3, 12).to(dt)
        r = R.emulation_ratio(lambda d, work: R.ref_gap_bwd(d, 5, 3, work), dy)
        worst["gap"] = max(worst["gap"], r["dx"])
    print("worst emulation ratios:", {n: round(v, 3) for n, v in worst.items()})
    assert all(v < 1.0 for v in worst.values()), worst


# ------------------------------------------------------------ conditions of the GPU file
@pytest.mark.parametrize("geom", GEOMS, ids=R.geom_id)
def test_bn_inputs_are_decided(geom):
    """>= 99 % of the windows of the BN pooling inputs have a tap that no correct
    evaluation can change, and no ReLU condition of the stem backward is ambiguous."""
    k, s, p, (H, W) = geom
    for C in R.CHANNELS + [520]:
        for dt in (F32, F16, BF16):
            x = R.bn_x((2, C, H, W), k, 7).to(dt)
            bn = R.bn_params(C, 7)
            _, tap, pre = R.ref_maxpool_fwd(x, k, s, p, bn=bn)
            share = float(R.decided(pre, tap, dt, k, s, p).double().mean())
            assert share >= 0.99, (C, dt, share)
            assert not bool(R.bnr_ambiguous(x, *bn).any())


def test_kernel_selection_mirror():
    assert R.fwd_kernel(BF16, 64, 3, 2, 1) == "maxpool3s2_fwd_k<plain>"
    assert R.fwd_kernel(F16, 64, 3, 2, 1, bn=True) == "maxpool3s2_fwd_k<BN>"
    assert R.fwd_kernel(BF16, 520, 3, 2, 1, bn=True) == "maxpool_fwd_k<VEC,BN>"
    assert R.fwd_kernel(F32, 64, 3, 2, 1) == "maxpool_fwd_k<VEC,plain>"
    assert R.fwd_kernel(BF16, 64, 3, 2, 1, aligned=False, bn=True) == "maxpool_fwd_k<scalar,BN>"
    assert R.fwd_kernel(BF16, 5, 3, 2, 1) == "maxpool_fwd_k<scalar,plain>"
    assert R.bwd_kernel(F16, 8, 3, 2, 1) == "maxpool3s2_bwd2_k<plain>"
    assert R.bwd_kernel(F16, 8, 3, 1, 1) == "maxpool_bwd_k<VEC>"
    assert R.bwd_kernel(F16, 8, 3, 2, 1, aligned=False) == "maxpool_bwd_k<scalar>"


def test_grid_stride_shapes_exceed_the_caps():
    cap = R.GRID_CAP * R.THREADS
    for name, c in R.BIG.items():
        assert c["items"] > c["cap"], name
        assert c["items"] < 1.02 * c["cap"], name      # the smallest such shape, roughly
    assert R.BIG["generic"]["cap"] == cap and R.BIG["bnr"]["cap"] == R.BNR_GRID_CAP * R.THREADS
    N, C, H, W = R.BIG["bnr"]["shape"]
    assert C == 64 and H % 2 == 1 and R.bnr_grid(N, H, W) == R.BNR_GRID_CAP


# ------------------------------------------------------------ wrong variants must fail
def _fails(got, ref, dtype=BF16):
    return R.worst_ratio(got.to(dtype), ref) > 1.0


def test_wrong_last_max_fails():
    x = R.tied((2, 8, 9, 11), 2)
    _, tap = R.ref_maxpool_fwd(x, 3, 2, 1)
    _, bad = R.ref_maxpool_fwd(x, 3, 2, 1, rule="last")
    assert float((tap != bad).double().mean()) > 0.5
    dy = R.rand_dy(tap.shape, 4).to(BF16)
    ref = R.ref_maxpool_bwd(dy, tap, 9, 11, 3, 2, 1)
    assert _fails(R.ref_maxpool_bwd(dy, bad, 9, 11, 3, 2, 1).v, ref)
    # and the tie-free input cannot tell them apart: the tied one is what is needed
    xf = R.tie_free((2, 8, 9, 11), 3, 1)
    assert torch.equal(R.ref_maxpool_fwd(xf, 3, 2, 1)[1], R.ref_maxpool_fwd(xf, 3, 2, 1, rule="last")[1])


def test_wrong_relu_ge_fails():
    shape = (2, 64, 9, 11)
    x, dy, bn = _bn_case(shape, BF16, 5, True)
    _, tap, _ = R.ref_maxpool_fwd(x, 3, 2, 1, bn=bn)
    good = R.ref_maxpool_bwd_bn(dy, tap, x, *bn)
    bad = R.ref_maxpool_bwd_bn(dy, tap, x, *bn, relu_ge=True)
    assert not torch.equal(good["cond"], bad["cond"])
    # the windows of the zero channel are all ties at 0: their gradients reach tap-0 inputs,
    # which >= lets through
    assert float(good["sum_dy"].v[0]) == 0.0
    assert not torch.equal(bad["sum_dy_xmu"].v, good["sum_dy_xmu"].v) \
        or not torch.equal(bad["sum_dy"].v, good["sum_dy"].v)
    assert _fails(bad["sum_dy"].v, good["sum_dy"], F32)


def test_wrong_missing_window_fails():
    x = R.tie_free((2, 8, 9, 11), 3, 1)
    _, tap = R.ref_maxpool_fwd(x, 3, 2, 1)
    for dy, equal_only in ((R.rand_dy(tap.shape, 4).to(BF16), False),
                           (R.exact_ints((2, 8, 9, 11), 3, 2, 1, 5)["dy"], True)):
        ref = R.ref_maxpool_bwd(dy, tap, 9, 11, 3, 2, 1)
        bad = R.ref_maxpool_bwd(dy, tap, 9, 11, 3, 2, 1, skip=(1, 1))
        assert not torch.equal(bad.v, ref.v)
        if not equal_only:
            assert _fails(bad.v, ref)


def test_wrong_unrounded_dx_in_sums_fails():
    shape = (2, 64, 9, 11)
    x, dy, bn = _bn_case(shape, BF16, 6, False)
    _, tap, _ = R.ref_maxpool_fwd(x, 3, 2, 1, bn=bn)
    good = R.ref_maxpool_bwd_bn(dy, tap, x, *bn)
    bad = R.ref_maxpool_bwd_bn(dy, tap, x, *bn, round_dx=False)
    assert _fails(bad["sum_dy_xmu"].v, good["sum_dy_xmu"], F32)


def test_wrong_inf_window_tap_out_of_bounds_fails():
    x = R.special((2, 8, 9, 11), 3, 3)
    y, tap = R.ref_maxpool_fwd(x, 3, 2, 1)
    yb, bad = R.ref_maxpool_fwd(x, 3, 2, 1, init="zero")
    _eq(y, yb, "y")                                    # y cannot tell
    assert not torch.equal(tap, bad)                   # the saved index can
    dy = R.exact_ints((2, 8, 9, 11), 3, 2, 1, 5)["dy"]
    good = R.ref_maxpool_bwd(dy, tap, 9, 11, 3, 2, 1)
    lost = R.ref_maxpool_bwd(dy, bad, 9, 11, 3, 2, 1)
    assert not torch.equal(good.v, lost.v)             # and so can the gradient:
    assert float(good.v.sum()) == float(dy.sum())      # the border windows' share is
    assert float(lost.v.sum()) != float(dy.sum())      # dropped
