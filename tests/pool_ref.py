"""float64 references of the channels-last pooling kernels (csrc/hip/pool.hip), shared by
tests/test_pool_ref_cpu.py (the references are right; deliberately wrong variants miss
them) and tests/test_pool_gpu.py (the kernels match them).  Same scheme as
tests/optim_ref.py, norm_ref.py and bn_ref.py, whose ``Val``, ``bound``, ``assert_within``,
``worst_ratio``, ``emulation_ratio``, ``K``, ``EPS32`` and ``vsum`` are used as they are.

Every ``ref_*`` function takes the tensors AS STORED (fp32 / fp16 / bf16), shaped
[N, C, H, W] whatever their memory format (on any device), and upcasts to float64.

  max forward   output size (H + 2p - k)//s + 1; the window's in-bounds taps are scanned in
                (kh, kw) order; the FIRST maximum wins; a NaN wins over any number and the
                first NaN stays; tap = kh*k + kw.  A window with no tap greater than -inf
                keeps the first IN-BOUNDS tap (the gradient of such a window goes to a real
                input, as ATen routes it).  Nothing is rounded: y is one of the inputs.
  with bn       the window values are relu((x - mean)*invstd*w + b) rounded to x's type
                before the comparison (bn_ref.ref_apply: its value, and the error magnitude
                of the kernels' o = x*sc + sh form); the float64 values before that rounding
                are returned too.  A value whose o is negative by more than its bound is
                EXACTLY 0 in any evaluation and carries e = 0.
  max backward  dx[h, w] = sum of dy over the covering windows whose tap points at (h, w).
                An input is covered by at most ceil(k/s)^2 windows, the kernel adds them
                one by one into an fp32 accumulator that starts at 0 (the first addition is
                exact): a chain of ceil(k/s)^2 - 1 additions, e = chain * sum|dy|.
  stem backward with the BatchNorm sums (maxpool3s2_bwd2_k<T, true>, k, s, p = 3, 2, 1)
                dx as above;  d = T(dx) * [(x*sc + sh) > 0] with sc = fl(invstd*w),
                sh = fl(b - fl(mean*sc)) as chan_affine forms them in fp32;
                sum_dy = sum d;  sum_dy_xmu = sum d*(x - mean)  per channel.
  gap backward  dy / (H*W); the kernel multiplies by fl(1 / HW): 2 roundings, e = 2|v|.

Chain of the stem backward's sums (``bnr_chain``), read off maxpool3s2_bwd2_k: the grid is
``bnr_grid`` = min(ceil(total/256), 16384, 2048) blocks over total = N*ceil(H/2)*ceil(W/2)*8
items; a thread runs ceil(total / (grid*256)) iterations and adds the 4 pixels of its 2x2
block serially into s1 / s2 in each; the lanes that share a channel group are combined by 3
xor-shuffle levels (8, 16, 32); the 4 wave totals are added serially in LDS; the consumer
(bn.slab_reduce_grad) adds the ``grid`` slab columns with bn_ref.slab_chain(grid):

                chain = 4*iterations + 3 + 4 + slab_chain(grid)

(4.2 million elements per channel at the largest case below give 4*2 + 7 + 15 = 30.)

ReLU condition.  fl(x*sc + sh) > 0 (one fma) has the sign of the exact x*sc + sh, which
float64 decides exactly for 16-bit x; what no reference can decide is an element whose
x*sc + sh is within a few roundings of sh of zero (the compiler may contract
b - mean*sc into one fma).  ``bnr_ambiguous`` marks those; the random inputs are drawn so
that there is none (asserted), and the exactly representable inputs of ``exact_ints``
(where sc, sh and the fma are exact) probe the condition AT zero.

Taps with bn.  Two window values closer than their bounds may be ordered either way by a
correct kernel.  ``decided`` marks the windows where every other tap is farther than the
bounds from the maximum, or where both values are exact (e = 0: a tie, or not, in any
evaluation); there the tap and y must match exactly.  Elsewhere the GPU test accepts
another tap only if the reference value there is within the bound of the reference maximum
and the kernel's y is that value within the same bound.

K.  The sums are plain additions: the float32 evaluation in any order stays within
0.5*eps32*S.  Measured on the CPU (tests/test_pool_ref_cpu.py::test_emulation_ratio asserts
< 1; worst over every input maker and geometry): max backward dx 0.19, stem sums sum_dy
0.01, sum_dy_xmu 0.02, gap backward 0.46.  Measured on an MI355X
(tests/test_pool_gpu.py, fp32 storage or fp32 sums): dx 0.06, sum_dy 0.00, sum_dy_xmu 0.01,
gap 0.09, BN forward y 0.07; with 16-bit outputs the ratio is that of the final rounding
to the storage type, just under 1.
"""
import torch
import torch.nn.functional as F

import bn_ref
from optim_ref import (EPS32, K, Val, assert_within, bound, emulation_ratio,  # noqa: F401
                       worst_ratio)
from norm_ref import vsum

F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64

# launch constants of csrc/hip/pool.hip
THREADS = 256            # kPoolThreads
GRID_CAP = 16384         # pool_grid
BNR_GRID_CAP = 2048      # maxpool_bwd_bn_grid
BN_MAX_C = 512           # kPoolBNMaxC


def _cdiv(a, b):
    return -(-int(a) // int(b))


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def pool_grid(items):
    return max(min(_cdiv(items, THREADS), GRID_CAP), 1)


def bnr_items(N, H, W):
    return N * _cdiv(H, 2) * _cdiv(W, 2) * 8


def bnr_grid(N, H, W):
    return min(pool_grid(bnr_items(N, H, W)), BNR_GRID_CAP)


def bnr_chain(N, H, W):
    g = bnr_grid(N, H, W)
    return float(4 * _cdiv(bnr_items(N, H, W), g * THREADS) + 3 + 4 + bn_ref.slab_chain(g))


def stem_geometry(k, s, p):
    return (k, s, p) == (3, 2, 1)


def fwd_kernel(dtype, C, k, s, p, aligned=True, bn=False):
    """The kernel maxpool2d_nhwc_fwd launches (its dispatch conditions)."""
    vec = C % 8 == 0 and aligned
    if dtype != F32 and vec and stem_geometry(k, s, p) and (not bn or C <= BN_MAX_C):
        return "maxpool3s2_fwd_k<%s>" % ("BN" if bn else "plain")
    return "maxpool_fwd_k<%s,%s>" % ("VEC" if vec else "scalar", "BN" if bn else "plain")


def bwd_kernel(dtype, C, k, s, p, aligned=True):
    vec = C % 8 == 0 and aligned
    if dtype != F32 and vec and stem_geometry(k, s, p):
        return "maxpool3s2_bwd2_k<plain>"
    return "maxpool_bwd_k<%s>" % ("VEC" if vec else "scalar")


# --------------------------------------------------------------------------- references
def _windows(X, k, s, p, fill):
    """(tap, values [N, C, OH, OW], in-bounds [1, 1, OH, OW]) in scan order."""
    H, W = X.shape[2], X.shape[3]
    OH, OW = out_size(H, k, s, p), out_size(W, k, s, p)
    Xp = F.pad(X, (p, p, p, p), value=fill)
    ok = F.pad(torch.ones(1, 1, H, W, dtype=torch.bool, device=X.device), (p, p, p, p),
               value=False)
    for kh in range(k):
        for kw in range(k):
            sl = (slice(None), slice(None), slice(kh, kh + (OH - 1) * s + 1, s),
                  slice(kw, kw + (OW - 1) * s + 1, s))
            yield kh * k + kw, Xp[sl], ok[sl]


def _scan(X, k, s, p, rule="first", init="in_bounds"):
    N, C, H, W = X.shape
    OH, OW = out_size(H, k, s, p), out_size(W, k, s, p)
    assert OH > 0 and OW > 0
    best = torch.full((N, C, OH, OW), float("-inf"), dtype=X.dtype, device=X.device)
    arg = torch.full((N, C, OH, OW), -1 if init == "in_bounds" else 0, dtype=torch.int64,
                     device=X.device)
    for tap, v, ok in _windows(X, k, s, p, 0.0):
        gt = (v >= best) if rule == "last" else (v > best)
        take = ok & (gt | (v.isnan() & ~best.isnan()) | (arg < 0))
        best = torch.where(take, v, best)
        arg = torch.where(take, torch.full_like(arg, tap), arg)
    assert bool((arg >= 0).all())
    return best, arg


def ref_maxpool_fwd(x, k, s, p, bn=None, rule="first", init="in_bounds"):
    """-> (y float64, tap int64), both [N, C, OH, OW]; with ``bn`` = (mean, invstd, w, b)
    (fp32 [C]; w / b may be None) also the float64 BN + ReLU values before the rounding to
    x's type, a Val shaped like x.  ``rule`` = "last" and ``init`` = "zero" (a window without
    a tap above -inf keeps tap 0, in bounds or not) are the WRONG variants the CPU file
    shows to fail."""
    if bn is None:
        return _scan(x.detach().to(F64), k, s, p, rule, init)
    mean, invstd, w, b = bn
    fw = bn_ref.ref_apply(x, mean, invstd, w, b, None, True)
    o, pre = fw["o"], fw["y"]
    exact0 = o.v < -bound(o, x.dtype)
    pre = Val(pre.v, torch.where(exact0, torch.zeros_like(pre.e), pre.e))
    y, tap = _scan(pre.v.to(x.dtype).to(F64), k, s, p, rule, init)
    return y, tap, pre


def at_tap(t, tap, k, s, p, fill=0.0):
    """t [N, C, H, W] read at each window's ``tap`` -> [N, C, OH, OW] (``fill`` where the
    tap is out of bounds)."""
    out = torch.full(tap.shape, fill, dtype=t.dtype, device=t.device)
    for i, v, ok in _windows(t, k, s, p, fill):
        out = torch.where((tap == i) & ok, v, out)
    return out


def decided(pre, tap, dtype, k, s, p):
    """Windows whose tap no correct evaluation can change (see the module docstring)."""
    big = float("inf")
    mv, me = at_tap(pre.v, tap, k, s, p), at_tap(pre.e, tap, k, s, p)
    mb = bound(Val(mv, me), dtype)
    out = torch.ones(tap.shape, dtype=torch.bool, device=tap.device)
    ev = _windows(pre.e, k, s, p, 0.0)
    for (i, v, ok), (_, e, _) in zip(_windows(pre.v, k, s, p, -big), ev):
        far = (mv - v).abs() > mb + bound(Val(v.clamp_min(-1e300), e), dtype)
        exact = (me == 0) & (e == 0)
        out &= far | exact | ~ok | (tap == i)
    return out


def ref_maxpool_bwd(dy, tap, H, W, k, s, p, work=F64, skip=None):
    """-> dx [N, C, H, W] as a Val.  A tap that points out of bounds drops its gradient (as
    the kernels' gather does).  ``skip`` = (a, b): the WRONG variant that omits the windows
    (i + a, j + b) of each 2x2 input block (stem geometry)."""
    DY = dy.detach().to(work)
    N, C, OH, OW = DY.shape
    acc = torch.zeros(N, C, H + 2 * p + k, W + 2 * p + k, dtype=work, device=DY.device)
    mag = torch.zeros_like(acc)
    zero = torch.zeros_like(DY)
    for kh in range(k):
        for kw in range(k):
            m = tap == kh * k + kw
            if skip is not None:
                # window (oh, ow) is (i + a, j + b) of the block of input (2*oh - 1 + kh, ...)
                a = 1 if kh == 0 else 0
                b = 1 if kw == 0 else 0
                if (a, b) == tuple(skip):
                    continue
            c = torch.where(m, DY, zero)
            sl = (slice(None), slice(None), slice(kh, kh + (OH - 1) * s + 1, s),
                  slice(kw, kw + (OW - 1) * s + 1, s))
            acc[sl] += c
            mag[sl] += c.abs()
    chain = float(_cdiv(k, s) ** 2 - 1)
    crop = (slice(None), slice(None), slice(p, p + H), slice(p, p + W))
    return Val(acc[crop].contiguous(), chain * mag[crop].contiguous())


def chan_affine32(mean, invstd, w, b):
    """sc, sh as bn_common.h chan_affine forms them in fp32 (two roundings for sh)."""
    sc = invstd.to(F32) * (w.to(F32) if w is not None else 1.0)
    sh = (b.to(F32) if b is not None else torch.zeros_like(sc)) - mean.to(F32) * sc
    return sc, sh


def _chan(t, work=F64):
    return t.detach().to(work).reshape(1, -1, 1, 1)


def bnr_ambiguous(x, mean, invstd, w, b):
    """Elements whose ReLU condition (x*sc + sh > 0) depends on how sh was rounded."""
    sc, sh = chan_affine32(mean, invstd, w, b)
    X = x.detach().to(F64)
    o = X * _chan(sc) + _chan(sh)
    mag = (X * _chan(sc)).abs() + _chan(sh).abs() + (_chan(mean) * _chan(sc)).abs()
    return o.abs() <= 4 * EPS32 * mag


def ref_maxpool_bwd_bn(dy, tap, x, mean, invstd, w, b, dx_stored=None, relu_ge=False,
                       round_dx=True, work=F64):
    """The fused stem backward (3x3 / stride 2 / pad 1).  ``dx_stored``: what the device
    stored (checked against "dx" separately), so that its rounding is not charged twice;
    without it dx is rounded to x's type here.  ``relu_ge`` (>= in the ReLU condition) and
    ``round_dx`` = False (the sums formed from the unrounded dx) are WRONG variants.
    -> dx [N, C, H, W], sum_dy, sum_dy_xmu [C] (Vals), cond (bool like x)."""
    N, C, H, W = x.shape
    dx = ref_maxpool_bwd(dy, tap, H, W, 3, 2, 1, work)
    if dx_stored is not None:
        g = dx_stored.detach().to(work)
    else:
        g = dx.v.to(x.dtype).to(work) if round_dx else dx.v
    sc, sh = chan_affine32(mean, invstd, w, b)
    o = x.detach().to(F64) * _chan(sc) + _chan(sh)
    cond = (o >= 0) if relu_ge else (o > 0)
    D = Val(bn_ref._cl(g * cond.to(work), work))
    xm = Val(bn_ref._cl(x, work)) - Val(mean.detach().to(work).reshape(-1, 1))
    chain = bnr_chain(N, H, W)
    return {"dx": dx, "sum_dy": vsum(D, 1, chain), "sum_dy_xmu": vsum(D * xm, 1, chain),
            "cond": cond}


def ref_gap_bwd(dy, H, W, work=F64):
    """dy [N, C] -> {"dx": Val [N, C, H, W]} = dy / (H*W), as reciprocal-then-multiply."""
    DY = dy.detach().to(work).reshape(dy.shape[0], dy.shape[1], 1, 1)
    inv = torch.ones((), dtype=work, device=DY.device) / float(H * W)
    v = (DY * inv).expand(-1, -1, H, W).contiguous()
    return {"dx": Val(v, 2 * v.abs())}


# --------------------------------------------------------------------------- inputs
def _gen(seed, device="cpu"):
    return torch.Generator(device=device).manual_seed(1000003 * seed + 12345)


def tie_free(shape, k, seed=0, device="cpu"):
    """No two equal values inside any k x k window: the value at (h, w) is a per-(n, c)
    random permutation of the k*k residue pairs (h % k, w % k), which a window covers once
    each.  Integers 0 .. k*k - 1 (fp32), exact in every storage type for k <= 15."""
    N, C, H, W = shape
    g = _gen(seed, device)
    perm = torch.argsort(torch.rand(N * C, k * k, generator=g, device=device), dim=1).float()
    res = ((torch.arange(H, device=device) % k).view(H, 1) * k
           + (torch.arange(W, device=device) % k).view(1, W)).view(1, H * W)
    return torch.gather(perm, 1, res.expand(N * C, H * W)).view(N, C, H, W)


def tied(shape, seed=0, device="cpu"):
    """Values from a 3-value alphabet: most windows have ties."""
    g = _gen(seed + 1, device)
    return torch.randint(-1, 2, shape, generator=g, device=device).float()


def rand_dy(shape, seed=0, device="cpu"):
    return torch.randn(shape, generator=_gen(seed + 2, device), device=device)


def exact_ints(shape, k, s, p, seed=0, device="cpu", xmax=6, dmax=None):
    """Inputs with which every kernel result is exactly representable in bf16 / fp16: x,
    dy, mean and b small integers, invstd and w powers of two (|sc| in 1/4 .. 4, so the BN
    value is a multiple of 1/4 below 64), every dx (a sum of at most ceil(k/s)^2 values
    |dy| <= dmax) below 2^8, the channel sums below 2^24 (asserted by the users).
    -> dict x, dy, mean, invstd, w, b."""
    N, C, H, W = shape
    g = _gen(seed + 3, device)
    OH, OW = out_size(H, k, s, p), out_size(W, k, s, p)
    if dmax is None:
        dmax = max(1, 128 // _cdiv(k, s) ** 2)

    def ints(sh, lo, hi):
        return torch.randint(lo, hi + 1, sh, generator=g, device=device).float()
    x = ints(shape, -xmax, xmax)
    dy = ints((N, C, OH, OW), -dmax, dmax)
    mean, b = ints((C,), -2, 2), ints((C,), -3, 3)
    invstd = 2.0 ** ints((C,), -1, 1)
    w = 2.0 ** ints((C,), -1, 1) * (1 - 2 * (ints((C,), 0, 3) == 0).float())
    return {"x": x, "dy": dy, "mean": mean, "invstd": invstd, "w": w, "b": b}


def zero_channel(inp, c=0):
    """Channel ``c`` of an ``exact_ints`` set has x*sc + sh exactly 0 everywhere
    (x = mean, b = 0): ReLU lets nothing through at exactly zero."""
    inp["x"][:, c] = inp["mean"][c]
    inp["b"][c] = 0.0
    return inp


def special(shape, k, seed=0, device="cpu"):
    """Small integers with -inf blocks at the top-left corner (border windows whose only
    in-bounds taps are -inf), at the bottom-right corner and in the interior, one NaN, and
    a patch of alternating +0 / -0 (a tie whose FIRST element's sign must come out)."""
    N, C, H, W = shape
    x = torch.randint(-4, 5, shape, generator=_gen(seed + 4, device), device=device).float()
    ninf = float("-inf")
    kb = min(k + 1, H), min(k + 1, W)
    x[:, :, :kb[0], :kb[1]] = ninf
    if H > 2 * k + 2 and W > 2 * k + 2:
        x[:, :, H // 2:H // 2 + k + 1, W // 2:W // 2 + k + 1] = ninf
        x[:, :, H - k:, W - k:] = ninf
    hz = min(H - 1, kb[0] + 1)
    sign = 1 - 2 * (torch.arange(W, device=device) % 2).float()
    x[:, :, hz, :] = 0.0 * sign                    # +0, -0, +0, ...
    if H > 1 and W > 1:
        x[0, 0, H - 1, W // 2] = float("nan")
    x[N - 1, C - 1] = ninf                         # one whole plane: every window
    return x


def bn_params(C, seed=0, device="cpu"):
    """Non-exact BatchNorm operands (fp32 [C]): mean, invstd, w (some negative), b."""
    g = _gen(seed + 5, device)
    mean = torch.randn(C, generator=g, device=device) * 0.5
    invstd = torch.rand(C, generator=g, device=device) + 0.5
    w = torch.rand(C, generator=g, device=device) + 0.5
    if C >= 3:
        w[C // 2] = -w[C // 2]
    b = torch.randn(C, generator=g, device=device) * 0.5 + 0.75
    return mean, invstd, w, b


def bn_x(shape, k, seed=0, device="cpu"):
    """The BN pooling input: tie-free steps of 1/2 around 0 (exact in every storage type),
    so that two taps of a window differ by at least |sc| / 2 after the affine."""
    return (tie_free(shape, k, seed, device) - float(k * k // 2)) * 0.5


def place(t, dtype, device, offset=0):
    """A [N, C, H, W] tensor on ``device`` in ``dtype``, channels-last, ``offset`` elements
    into its storage (offset 1: a misaligned view the vector kernels must refuse)."""
    N, C, H, W = t.shape
    buf = torch.empty(t.numel() + offset, dtype=dtype, device=device)
    v = buf[offset:].view(N, H, W, C).permute(0, 3, 1, 2)
    v.copy_(t.to(device))
    assert v.is_contiguous(memory_format=torch.channels_last) or C == 1 or H * W == 1
    return v


# (k, s, p, [(H, W), ...]) walked by both test files
GEOMETRIES = [
    (3, 2, 1, [(8, 10), (9, 11), (7, 6), (1, 1), (2, 2)]),
    (2, 2, 0, [(7, 8)]),
    (3, 1, 1, [(6, 5)]),
    (1, 1, 0, [(3, 4)]),
    (2, 3, 0, [(8, 7)]),      # stride > kernel: inputs without a window
    (5, 2, 2, [(9, 8)]),
    (7, 3, 3, [(11, 13)]),
    (15, 2, 7, [(16, 16)]),
]
CHANNELS = [1, 5, 8, 24, 64]


def geometries():
    return [(k, s, p, hw) for k, s, p, hws in GEOMETRIES for hw in hws]


def geom_id(g):
    return "k%ds%dp%d-%dx%d" % (g[0], g[1], g[2], g[3][0], g[3][1])


def _big(shape, k, s, p, per, cap):
    N, C, H, W = shape
    fwd = N * out_size(H, k, s, p) * out_size(W, k, s, p) * (C // per)
    blk = N * _cdiv(H, 2) * _cdiv(W, 2) * (C // per)
    return dict(shape=shape, k=k, s=s, p=p, cap=cap, fwd_items=fwd, bwd_items=N * H * W * (C // per),
                blk_items=blk)


# The smallest shapes whose work items exceed the grid caps, so that the grid-stride loops
# run a second time: generic scalar forward / backward (one item per element), the stem
# forward (one per 8 channels of an output) and plain stem backward (one per 2x2 block),
# the stem backward with the BatchNorm sums (C = 64, odd H) and the scalar gap backward.
_CAP = GRID_CAP * THREADS
BIG = {
    "generic": _big((1, 5, 917, 917), 3, 1, 1, 1, _CAP),
    "stem": _big((1, 8, 4098, 4098), 3, 2, 1, 8, _CAP),
    "bnr": _big((2, 64, 363, 362), 3, 2, 1, 8, BNR_GRID_CAP * THREADS),
    "gap": dict(shape=(2, 5, 648, 648), cap=_CAP, items=2 * 5 * 648 * 648),
}
BIG["generic"]["items"] = min(BIG["generic"]["fwd_items"], BIG["generic"]["bwd_items"])
BIG["stem"]["items"] = min(BIG["stem"]["fwd_items"], BIG["stem"]["blk_items"])
BIG["bnr"]["items"] = bnr_items(2, 363, 362)
