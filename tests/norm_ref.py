"""float64 references of the LayerNorm / RMSNorm kernels (csrc/hip/layer_norm.hip) and of
the fused residual join, shared by tests/test_norm_ref_cpu.py (the references are right),
tests/test_layer_norm_gpu.py (the kernels match them) and tests/test_layer_norm_cpu.py
(the extension's CPU branch matches them).

Every ``ref_*`` function takes the tensors AS STORED (fp32 / fp16 / bf16), upcasts to
float64 and applies the formulas written from the math, over rows of ``n2`` elements:

  forward   mu = mean(x) (0 for RMS);  var = mean((x - mu)^2) (two passes);
            iv = rsqrt(var + eps);  y = (x - mu) * iv * gamma + beta
  backward  mu, iv recomputed here (a wrong saved statistic shows in dx too);
            xh = (x - mu) * iv;  dg = dy * gamma;
            dx = (dg - mean(dg) - xh * mean(dg * xh)) * iv   (no mean(dg) term for RMS);
            dgamma = sum_rows(dy * xh);  dbeta = sum_rows(dy)
  join      s = x + keep * h * scale (scale = float32(1 / (1 - p)), keep GIVEN), rounded once
            to x's type; y, mean, invvar = LayerNorm of s AS STORED;
            ds = LN'(dy) + ds_ext;  dh = keep * ds * scale;  dhsum = sum_rows(dh AS STORED)

Results are ``optim_ref.Val`` objects: the float64 value ``v`` and the running first-order
error magnitude ``e`` = S.  An output stored in type T must satisfy ``optim_ref.bound``:

    |got - ref| <= u_T*|ref| + tiny_T + K*eps32*S

Reductions.  ``vsum(val, dim, chain)`` has value v.sum(dim) and error
e.sum(dim) + chain * |v|.sum(dim): the SUM OF MAGNITUDES, so that a cancelling sum
(sum(x - mu), mean(dg)) is not under-budgeted.  ``chain`` is the longest run of dependent
fp32 additions on the way to one result, read off layer_norm.hip:

  row sums (mean, variance, mean(dg), mean(dg*xh)) - ``row_chain(n2)``
    fast     a lane adds its 8*VPT values serially (VPT = ceil(n2 / 512) 16-byte groups of 8
             columns), then wave_sum: 6 xor-shuffle levels          -> 8*ceil(n2/512) + 6
    generic  a thread adds ceil(n2 / 256) values, wave_sum (6), then block_sum adds the 4
             wave totals serially (4)                               -> ceil(n2/256) + 10
  column sums (dgamma, dbeta, dhsum) - ``col_chain(n1, n2)``
    fast     ln_bwd_fast: blocks = min(ceil(n1/4), 1024), a wave walks
             ceil(n1 / (4*blocks)) rows adding into registers; the LDS combine adds the 4
             waves serially (4); ln_bwd_colsum: a row lane adds its ceil(blocks / 32)
             partial rows (the four-deep unrolled loop is shallower, never deeper), then a
             5-level LDS tree over the 32 row lanes
                                   -> ceil(n1/(4*blocks)) + 4 + ceil(blocks/32) + 5
    generic  ln_bwd_colpart_generic: parts = min(ceil(n1/32), 512), ceil(n1 / parts) rows
             added serially; then ln_bwd_colsum as above
                                   -> ceil(n1/parts) + ceil(parts/32) + 5
  Each is the LARGER of the two paths (the fast one exists for n2 % 8 == 0, n2 <= 2048
  only; a misaligned pointer sends any width down the generic one), as a function of the
  shape: (n1, n2) = (5, 64) has 14 / 11, (32772, 64) has 14 / 86.

Variance.  d = x - mu carries the error of mu to first order (e_d = e_mu + |d|): y, xh, dx
pay for it, as they must - a mean that is off by delta shifts every y by delta * iv.  The
variance does NOT: sum((d - delta)^2) = sum(d^2) + n*delta^2 exactly, because sum(d) = 0
at the true mean of the stored row.  So the variance is budgeted from d with its own
rounding alone (e = |d|) plus the second-order term delta^2 <= (0.5*eps32*e_mu)^2, entered
as eps32 * e_mu^2 in S (so that K*eps32*S holds 4K times that square: its own margin,
independent of K).  Without this the offset-row inputs (|mu| / sigma = 1e5) would get a
variance budget as large as the variance and a one-pass E[x^2] - mu^2 kernel would pass.

rsqrt.  rsqrtf enters with 2 ulp (as powf does in optim_ref) plus its first-order term
e_a * r / (2*a).

K.  With S defined this way the same formulas evaluated in float32 in the same order stay
within 0.5*eps32*S to first order.  The kernels differ in order (a multiplication by
1/n2 rounded once instead of a division, fmaf in the sums and in y, gamma applied before
or after the row means) with at most about twice the roundings on any path, and rsqrtf has
up to 2 ulp: 0.5 * 2 * 2 = 2, and K = 4 keeps the float32 emulation under HALF the bound.
Measured on the CPU against the reference alone (never on a kernel or on the extension):
worst |ref32 - ref64| / (eps32 * S) over every shape, operator and storage type of
tests/test_layer_norm_gpu.py, eps in 1e-5 / 1e-12 / 0.1, the offset, constant and zero
rows (tests/test_norm_ref_cpu.py::test_k_measured asserts these stay <= K/2):

    layer_norm  y 0.46  mean 0.12  invvar 0.15  dx 0.14  dgamma 0.07  dbeta 0.11
    rms_norm    y 0.18  mean 0.00  invvar 0.15  dx 0.22  dgamma 0.08  dbeta 0.11
    join        s 0.48  y 0.43  mean 0.01  invvar 0.13  ds 0.17  dh 0.18  dgamma 0.03
                dbeta 0.00  dhsum 0.00

(Just under 0.50 is the final rounding of an elementwise output whose last term dominates;
the reductions sit far below it because torch's float32 sums are pairwise while S budgets
the kernels' serial chains.)  K = 4 therefore leaves the emulation at one eighth of the
bound.  The extension's CPU branch (csrc/torch/norm_ops.cpp) IS this emulation - float32
ATen elementwise operations and reductions in the order of the formulas above - so it adds
nothing to K; measured the same way on its fp32 outputs (tests/test_layer_norm_cpu.py's
shapes, the three eps): y 0.40, mean 0.04, invvar 0.11, dx 0.15, dgamma 0.05, dbeta 0.05.
"""
import torch

from optim_ref import (EPS32, Val, assert_within, bound, emulation_ratio, f32,  # noqa: F401
                       worst_ratio)

K = 4.0
FAST_MAX_N2 = 2048


def _cdiv(a, b):
    return -(-int(a) // int(b))


def fast_width(n2):
    """Widths the one-row-per-wave kernels take (given 16-byte aligned pointers)."""
    return n2 % 8 == 0 and n2 <= FAST_MAX_N2


def row_chain(n2):
    """Longest chain of dependent fp32 additions in a sum over one row (see above)."""
    generic = _cdiv(n2, 256) + 6 + 4
    fast = 8 * _cdiv(n2, 512) + 6 if fast_width(n2) else 0
    return float(max(generic, fast))


def col_chain(n1, n2):
    """Longest chain of dependent fp32 additions in a sum over the rows of one column."""
    n1 = max(int(n1), 1)
    parts = min(_cdiv(n1, 32), 512)
    generic = _cdiv(n1, parts) + _cdiv(parts, 32) + 5
    fast = 0
    if fast_width(n2):
        blocks = min(_cdiv(n1, 4), 1024)
        fast = _cdiv(n1, 4 * blocks) + 4 + _cdiv(blocks, 32) + 5
    return float(max(generic, fast))


def vsum(val, dim, chain, keepdim=False):
    """Sum along ``dim`` as a chain / tree of fp32 additions ``chain`` deep."""
    v = val.v.sum(dim, keepdim=keepdim)
    return Val(v, val.e.sum(dim, keepdim=keepdim) + chain * val.v.abs().sum(dim, keepdim=keepdim))


def vrsqrt(a):
    """1 / sqrt(a), a > 0: first-order term of the argument's error plus 2 ulp (rsqrtf)."""
    r = a.v.rsqrt()
    return Val(r, a.e * r / (2 * a.v) + 2 * r)


def _leaf(t, work):
    return Val(t.detach().to(work))


def _rows(t, n2, work):
    return _leaf(t, work).v.reshape(-1, n2)


def _stats(x, n2, eps, rms, work):
    """-> X - mu (with the error of mu), mu, iv; all [n1, n2] / [n1, 1] Vals."""
    X = Val(_rows(x, n2, work))
    chain = row_chain(n2)
    if rms:
        mu = Val(torch.zeros(X.v.shape[0], 1, dtype=work))
        D = Dvar = X
    else:
        mu = vsum(X, 1, chain, keepdim=True) / float(n2)
        D = X - mu
        Dvar = Val(D.v, D.v.abs())   # the variance sees mu's error to second order only
    var = vsum(Dvar * Dvar, 1, chain, keepdim=True) / float(n2)
    var = Val(var.v, var.e + EPS32 * mu.e * mu.e)
    iv = vrsqrt(var + f32(eps))
    return D, mu, iv


def _params(t, n2, work):
    return None if t is None else Val(_rows(t, n2, work))


def _shaped(val, shape):
    return Val(val.v.reshape(shape), val.e.reshape(shape))


def ref_forward(x, gamma, beta, n2, eps, rms, work=torch.float64):
    """-> {"y": like x, "mean": [n1], "invvar": [n1]}; gamma / beta may be None."""
    D, mu, iv = _stats(x, n2, eps, rms, work)
    y = D * iv
    G, B = _params(gamma, n2, work), _params(beta, n2, work)
    if G is not None:
        y = y * G
    if B is not None:
        y = y + B
    return {"y": _shaped(y, x.shape), "mean": _shaped(mu, (-1,)), "invvar": _shaped(iv, (-1,))}


def ref_backward(dy, x, gamma, n2, eps, rms, work=torch.float64):
    """-> {"dx": like x, "dgamma": [n2], "dbeta": [n2]} (reshape to the parameter's shape
    with ``_shaped`` / ``.reshape``); gamma may be None (dg = dy)."""
    D, _, iv = _stats(x, n2, eps, rms, work)
    DY = Val(_rows(dy, n2, work))
    G = _params(gamma, n2, work)
    xh = D * iv
    dg = DY if G is None else DY * G
    chain = row_chain(n2)
    m2 = vsum(dg * xh, 1, chain, keepdim=True) / float(n2)
    if rms:
        t = dg - xh * m2
    else:
        t = dg - vsum(dg, 1, chain, keepdim=True) / float(n2) - xh * m2
    cc = col_chain(DY.v.shape[0], n2)
    return {"dx": _shaped(t * iv, x.shape), "dgamma": vsum(DY * xh, 0, cc),
            "dbeta": vsum(DY, 0, cc)}


def join_scale(p):
    """The dropout scale as the kernels receive it."""
    return f32(1.0 / (1.0 - float(p)))


def _masked(val, keep):
    return Val(val.v * keep, val.e * keep)


def ref_join_forward(x, h, keep, p, gamma, beta, n2, eps, s_stored=None, work=torch.float64):
    """``keep``: 0 / 1 tensor like x.  The LayerNorm runs on ``s_stored`` (what the device
    stored, checked against "s" separately); without it s is rounded to x's type here.
    -> s, y, mean, invvar."""
    keep = keep.detach().to(work).reshape(x.shape)
    S = _leaf(x, work) + _masked(_leaf(h, work) * join_scale(p), keep)
    s_in = s_stored if s_stored is not None else S.v.to(x.dtype)
    out = ref_forward(s_in, gamma, beta, n2, eps, False, work)
    out["s"] = S
    return out


def ref_join_backward(dy, ds_ext, s, keep, p, gamma, n2, eps, h_dtype=None, dh_stored=None,
                      work=torch.float64):
    """``s``: the stored LayerNorm input.  dy / ds_ext may be None (an unused output).
    dhsum sums ``dh_stored`` (what the device stored, checked against "dh" separately), or
    dh rounded to ``h_dtype`` here.  -> ds, dh, dgamma, dbeta, dhsum."""
    keep = keep.detach().to(work).reshape(s.shape)
    r = ref_backward(torch.zeros_like(s) if dy is None else dy, s, gamma, n2, eps, False, work)
    ds = r["dx"] if ds_ext is None else r["dx"] + _leaf(ds_ext, work)
    dh = _masked(ds * join_scale(p), keep)
    dh_in = dh_stored if dh_stored is not None else dh.v.to(h_dtype or s.dtype)
    n1 = s.numel() // n2
    dhsum = vsum(Val(_rows(dh_in, n2, work)), 0, col_chain(n1, n2))
    return {"ds": ds, "dh": dh, "dgamma": r["dgamma"], "dbeta": r["dbeta"], "dhsum": dhsum}


def one_pass_forward(x, n2, eps, work=torch.float32):
    """What a one-pass E[x^2] - mu^2 LayerNorm computes in ``work`` precision (plain
    tensors): the conditioning inputs are only worth something if THIS lands outside the
    bound.  -> mean [n1], invvar [n1]."""
    X = _rows(x, n2, work)
    mu = X.mean(1)
    var = (X * X).mean(1) - mu * mu
    return mu, (var + f32(eps)).rsqrt()


# --------------------------------------------------------------------------- test cases
# Shared by the CPU measurement of K and the GPU comparison, so that K is measured on
# exactly the shapes and inputs the kernels are held to.
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16

FAST_N2 = [8, 64, 504, 512, 520, 1024, 1032, 1536, 1544, 2048]
FAST_N1 = [1, 3, 5]
FAST_GRIDS = [(130, 64), (520, 64), (4100, 64), (32772, 8), (32772, 64)]
GENERIC_N2 = [1, 7, 15, 777, 998, 2056, 4100]
GENERIC_N1 = [1, 33]
GENERIC_CAP = [(16400, 7)]


def shapes():
    """Every (n1, n2) of the shape sweep: each lane-edge / generic width at each of its
    row counts, and the grid shapes."""
    out = [(n1, n2) for n2 in FAST_N2 for n1 in FAST_N1] + FAST_GRIDS
    out += [(n1, n2) for n2 in GENERIC_N2 for n1 in GENERIC_N1] + GENERIC_CAP
    return out


# operator = (rms, affine); parameter type None = x's own
OPERATORS = [(False, True), (False, False), (True, True), (True, False)]
TYPE_COMBOS = [(F32, None), (F16, None), (BF16, None), (F16, F32), (BF16, F32)]
COMBO_SHAPES = [(5, 1032), (33, 777)]   # one fast, one generic


def make_inputs(n1, n2, dtype, wdtype=None, seed=0, kind="randn", shape=None):
    """Seeded CPU inputs: x, dy (drawn in fp32, rounded to the type the kernel reads),
    gamma, beta (in ``wdtype`` or x's type)."""
    g = torch.Generator().manual_seed(seed * 1000003 + n1 * 131 + n2)
    shape = tuple(shape) if shape is not None else (n1, n2)
    r = torch.randn(shape, generator=g, dtype=torch.float32)
    if kind == "randn":
        x = r * 2 + 0.5
    elif kind == "offset1000":
        x = 1000 + 0.01 * r
    elif kind == "offset8":
        x = 8 + 0.25 * r
    elif kind == "const":
        x = torch.full(shape, 0.5)
    elif kind == "zero":
        x = torch.zeros(shape)
    else:
        raise ValueError(kind)
    dy = torch.randn(shape, generator=g, dtype=torch.float32)
    gamma = torch.randn(n2, generator=g, dtype=torch.float32) * 0.5 + 1.0
    beta = torch.randn(n2, generator=g, dtype=torch.float32)
    wd = wdtype or dtype
    return x.to(dtype), dy.to(dtype), gamma.to(wd), beta.to(wd)


def conditioning_cases():
    """(kind, dtype, n2) of the offset / constant / zero rows (n1 = 16 each)."""
    out = []
    for n2 in (1024, 777):
        out.append(("offset1000", F32, n2))
        out.append(("offset8", BF16, n2))
        for dt in (F32, BF16):
            out.append(("const", dt, n2))
            out.append(("zero", dt, n2))
    return out


COND_N1 = 16
JOIN_SHAPES = [(3, 8), (4100, 8), (3, 520), (4100, 520), (3, 2048), (4100, 2048)]
JOIN_P = [0.0, 0.1, 0.9]


def make_join_inputs(n1, n2, dtype, wdtype, p, seed=0):
    """x, h, keep (a seeded stand-in mask of density 1 - p), dy, ds_ext, gamma, beta."""
    x, dy, gamma, beta = make_inputs(n1, n2, dtype, wdtype, seed=seed + 17)
    g = torch.Generator().manual_seed(seed * 7919 + n1 + n2)
    h = torch.randn(n1, n2, generator=g, dtype=torch.float32).to(dtype)
    de = torch.randn(n1, n2, generator=g, dtype=torch.float32).to(dtype)
    keep = (torch.rand(n1, n2, generator=g) >= p).to(torch.float32)
    return x, h, keep, dy, de, gamma, beta
