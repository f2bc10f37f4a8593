"""float64 references and exact-integer generators for the MFMA convolution and GEMM
kernels (csrc/hip/conv_igemm.hip, stem_conv.hip, gemm4w.hip, wgrad4w.hip), shared by
tests/test_conv_ref_cpu.py (the references equal F.conv2d and its autograd in fp64; the
generators meet the conditions below on every GPU shape) and tests/test_conv_exact_gpu.py
(the kernels equal the references BIT FOR BIT).

Why exact.  These kernels are sums of products accumulated in fp32.  With small-integer
inputs every product and every partial sum is an integer below 2^24, which fp32 holds
exactly, so the result does not depend on the tiling, the ring depth, the split count or
the order of accumulation: the kernel's output must equal the float64 reference rounded
ONCE to the output type.  One missing, doubled or misplaced term anywhere changes an
integer and fails ``torch.equal``; no tolerance exists to be tuned.

References (plain torch in float64, no F.conv2d, so they run in fp64 on either device).
A convolution is the sum over its taps (r, s) of a matmul of the shifted, strided slice of
the zero-padded input with that tap's [Cout, Cin] matrix:

  conv_fwd    y[n, :, i, j]    = sum_rs W[:, :, r, s] . xpad[n, :, i*st + r, j*st + s]
  conv_dgrad  dxpad[n, :, i*st + r, j*st + s] += W[:, :, r, s]^T . dy[n, :, i, j]
  conv_wgrad  dW[:, :, r, s]   = sum_nij dy[n, :, i, j] (x) xpad[n, :, i*st + r, j*st + s]
  abt / atb   A . B^T and A^T . B

Tensors are [N, C, H, W] whatever their memory format; results are float64 [N, C, H, W]
(contiguous in channels-last order) or [Cout, Cin, k, k].

Generators.  ``ints``: integers uniform in [-2, 2] (x, dy of the data path, A).
``thin_ints(shape, K, col_dim)``: the same, each kept with probability min(1, 48 / K) - K
being the reduction length - so an output is a sum of ~48 non-zero products whatever K is
and stays small; then every "column" (every index of the tensor with ``col_dim`` removed:
a (ci, r, s) of a weight over its Cout, a pixel of a weight-gradient dy over its
channels) that came out all zero gets one non-zero at a random place, so that no element
of the OTHER operand is invisible in the result.  (Thinning alone leaves ~1.3 % of the
weight columns empty at Cout = 64 - 128.)

Conditions, asserted on the REFERENCE by ``check_*`` for every case (they are what makes
the comparison exact, not tolerances):

  max |y| <= 128                        every output is an integer bf16 and fp16 hold
                                        (integers up to 256 / 2048), and so is y + add
  tile statistics < 2^24                sum and sum of squares of (y - shift) over any run
                                        of up to 256 rows (bounded by 256 * max^2)
  weight-gradient partials < 2^24       bounded by sum_p |dy[p, co]| * max|x| per channel,
                                        which bounds every partial sum of every split
"""
import torch

LIM_Y = 128
LIM_ACC = 1 << 24


def gen(seed, device="cpu"):
    return torch.Generator(device=device).manual_seed(seed)


def ints(shape, g, dtype=torch.bfloat16):
    """Integers uniform in [-2, 2], generated on g's device."""
    return torch.randint(-2, 3, tuple(shape), generator=g, device=g.device).to(dtype)


def thin_ints(shape, K, col_dim, g, dtype=torch.bfloat16):
    """``ints`` kept with probability min(1, 48 / K); every column over ``col_dim`` then has
    at least one non-zero (see the module docstring)."""
    shape = tuple(shape)
    dev = g.device
    v = torch.randint(-2, 3, shape, generator=g, device=dev)
    keep = torch.rand(shape, generator=g, device=dev) < min(1.0, 48.0 / K)
    v = v * keep
    empty = (v != 0).sum(col_dim, keepdim=True) == 0
    n = shape[col_dim]
    where = torch.randint(0, n, empty.shape, generator=g, device=dev)
    val = torch.randint(0, 4, empty.shape, generator=g, device=dev)
    val = torch.where(val < 2, val - 2, val - 1)                 # -2, -1, 1, 2
    idx = torch.arange(n, device=dev).view([n if d == col_dim else 1 for d in range(len(shape))])
    v = torch.where(empty & (idx == where), val, v)
    return v.to(dtype)


def weight(co, ci, k, g, dtype=torch.bfloat16, col_dim=0):
    """Thinned integer filter [co, ci, k, k] (channels-last).  col_dim 0: for a forward conv
    (K = ci*k*k, every (ci, r, s) column used by some co); col_dim 1: for a data gradient
    (K = co*k*k, every (co, r, s) used by some ci)."""
    K = (ci if col_dim == 0 else co) * k * k
    w = thin_ints((co, ci, k, k), K, col_dim, g, dtype)
    return w.contiguous(memory_format=torch.channels_last)


def act(n, c, h, w, g, dtype=torch.bfloat16):
    """Integer activation [n, c, h, w] (channels-last)."""
    return ints((n, c, h, w), g, dtype).contiguous(memory_format=torch.channels_last)


def thin_dy(n, c, h, w, g, dtype=torch.bfloat16):
    """Thinned integer dy of a weight gradient (K = n*h*w pixels), every pixel used."""
    t = thin_ints((n, c, h, w), n * h * w, 1, g, dtype)
    return t.contiguous(memory_format=torch.channels_last)


# ---------------------------------------------------------------- references
def _rows(t):
    """[N, C, H, W] -> float64 [N, H, W, C]."""
    return t.detach().double().permute(0, 2, 3, 1)


def _pad_rows(x, pad):
    n, h, w, c = x.shape
    xp = x.new_zeros(n, h + 2 * pad, w + 2 * pad, c)
    xp[:, pad:pad + h, pad:pad + w] = x
    return xp


def out_size(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


def _tap(xp, r, s, ho, wo, stride):
    return xp[:, r:r + stride * (ho - 1) + 1:stride, s:s + stride * (wo - 1) + 1:stride]


def conv_fwd(x, w, stride=1, pad=None):
    k = w.shape[2]
    pad = k // 2 if pad is None else pad
    xr, wd = _rows(x), w.detach().double()
    n, h, wid, _ = xr.shape
    ho, wo = out_size(h, k, stride, pad), out_size(wid, k, stride, pad)
    xp = _pad_rows(xr, pad)
    y = xr.new_zeros(n, ho, wo, w.shape[0])
    for r in range(k):
        for s in range(k):
            y += _tap(xp, r, s, ho, wo, stride) @ wd[:, :, r, s].t()
    return y.permute(0, 3, 1, 2)


def conv_dgrad(dy, w, h, wid, stride=1, pad=None):
    k = w.shape[2]
    pad = k // 2 if pad is None else pad
    dr, wd = _rows(dy), w.detach().double()
    n, ho, wo, _ = dr.shape
    dxp = dr.new_zeros(n, h + 2 * pad, wid + 2 * pad, w.shape[1])
    for r in range(k):
        for s in range(k):
            _tap(dxp, r, s, ho, wo, stride).add_(dr @ wd[:, :, r, s])
    return dxp[:, pad:pad + h, pad:pad + wid].permute(0, 3, 1, 2)


def conv_wgrad(dy, x, k, stride=1, pad=None):
    pad = k // 2 if pad is None else pad
    dr, xr = _rows(dy), _rows(x)
    n, ho, wo, co = dr.shape
    ci = xr.shape[3]
    xp = _pad_rows(xr, pad)
    dw = dr.new_zeros(co, ci, k, k)
    d2 = dr.reshape(-1, co).t()
    for r in range(k):
        for s in range(k):
            dw[:, :, r, s] = d2 @ _tap(xp, r, s, ho, wo, stride).reshape(-1, ci)
    return dw


def abt(a, b):
    return a.detach().double() @ b.detach().double().t()


def atb(a, b):
    return a.detach().double().t() @ b.detach().double()


def slab_sums(y, shift=None):
    """Per-channel (sum, sum of squares) of y - shift over all pixels: float64 [2, C]."""
    v = y.detach().double()
    if shift is not None:
        v = v - shift.detach().double().view(1, -1, 1, 1)
    return torch.stack([v.sum((0, 2, 3)), (v * v).sum((0, 2, 3))])


# ---------------------------------------------------------------- conditions
def check_output(y, extra=0.0, shift=None):
    """max |y| (+ extra, e.g. a residual's largest value) <= 128 and every statistic over a
    run of up to 256 rows below 2^24; y is a float64 reference."""
    m = float(y.abs().max()) if y.numel() else 0.0
    assert m + extra <= LIM_Y, (m, extra)
    assert torch.equal(y, y.round()), "reference is not integral"
    s = 0.0 if shift is None else float(shift.abs().max())
    assert 256 * (m + extra + s) ** 2 < LIM_ACC, (m, extra, s)
    return m


def check_wgrad(dy, x, dw=None):
    """Every partial sum of every split of dW stays below 2^24: bounded per output channel
    by sum_p |dy[p, co]| * max |x|."""
    b = float(dy.detach().double().abs().sum((0, 2, 3)).max()) * float(x.detach().double().abs().max())
    assert b < LIM_ACC, b
    if dw is not None:
        assert torch.equal(dw, dw.round())
    return b


def rounded(ref, dtype):
    """The float64 reference rounded ONCE to the output type (round to nearest even)."""
    return ref.to(dtype)
