"""float64 references of the BatchNorm kernels (csrc/hip/batch_norm.hip, bn_nhwc.hip,
csrc/include/bn_common.h), shared by tests/test_bn_ref_cpu.py (the references are right;
the extension's CPU branches match them) and tests/test_batch_norm_gpu.py (the kernels
match them).  Same scheme as tests/optim_ref.py and tests/norm_ref.py, whose ``Val``,
``bound``, ``assert_within``, ``worst_ratio``, ``emulation_ratio``, ``vsum`` and ``vrsqrt``
are used as they are.

Every ``ref_*`` function takes the tensors AS STORED (fp32 / fp16 / bf16), shaped
[N, C, *] whatever their memory format, upcasts to float64 and applies the formulas
written from the math, per channel over the n = N * prod(*) elements of the channel:

  stats     mean = sum(x)/n;  var = sum((x - mean)^2)/n (biased);  invstd = rsqrt(var + eps)
            running_mean' = (1 - m)*running_mean + m*mean
            running_var'  = (1 - m)*running_var  + m*var*(n > 1 ? n/(n-1) : 1)
  combine   N = sum_i n_i;  mean = sum_i n_i*mean_i / N;
            var = sum_i n_i*(var_i + (mean_i - mean)^2) / N  (the plain pooled formulas);
            invstd, 1/N, running stats with var*N/(N-1) for N > 1
  apply     o = (x - mean)*invstd*w + b (+ z);  mask = o > 0;  y = relu?(o)
            (mean / invstd GIVEN: the statistics of x from ``ref_stats`` or any others)
  backward  d = dy*mask (mask GIVEN);  sum_dy = sum(d);  sum_dy_xmu = sum(d*(x - mean));
            dgamma = sum_dy_xmu*invstd;  dbeta = sum_dy;  xhat = (x - mean)*invstd;
            dx = (d - mean(d) - xhat*mean(d*xhat))*invstd*w;  dz = d
            ``sum_scale`` form (SyncBN): the two sums leave multiplied by the device scalar
            (1/global count) and dx takes them as the means; accumulate form: dgamma / dbeta
            are ADDED to the stored gw / gb
  slab      the finalize formulas above on sum_s slab[0|1][c][s]

Results are ``optim_ref.Val`` objects: the float64 value ``v`` and the running first-order
error magnitude ``e`` = S.  An output stored in type T must satisfy ``optim_ref.bound``:

    |got - ref| <= u_T*|ref| + tiny_T + K*eps32*S

Reductions.  ``vsum(val, dim, chain)`` has error e.sum + chain * |v|.sum, ``chain`` being
the longest run of dependent fp32 additions an element passes through on the way to the
result, read off the kernels:

  NHWC reductions (stats_k, reduce_k) - ``nhwc_chain(M, C, tuning)``
    a thread adds ceil(per / rows_iter) rows serially (per = ceil(M / splits) rows of its
    split; the U-unrolled loop adds its rows in order and a clamped slot adds an exact 0);
    block_slab_write adds the rows_iter row groups of the block serially in LDS
    (rows_iter - 1); the finalize's slab_sum adds ceil(splits / 256) slab rows per thread,
    6 xor-shuffle levels and the 4 wave totals serially
                     -> ceil(per/rows_iter) + rows_iter - 1 + ceil(splits/256) + 10
    the LARGER of the scalar and the vector geometry (ngeom(C, vec)) where both can run.
  NCHW reductions (stats_nchw, reduce_nchw) - ``nchw_chain(N, C, HW)``
    a thread adds ceil(ceil(L/splits) / 256) elements (scalar) or 8 * ceil(ceil(L/8/splits)
    / 256) (vector), L = N*HW; block_sum: 6 shuffle levels + 4 waves; then slab_sum
                     -> max(scalar, vector) + 10 + ceil(splits/256) + 10
  slab finalizes (slab_t_sum<CH>, TPC = 256 / slab_ch(S) threads per channel) -
    ``slab_chain(S)``: 8 chains of ceil(S / (8*TPC)) values, a tail of up to 7 more on chain
    0, the 3-level tree over the 8 chains and the log2(TPC)-level LDS tree
                     -> ceil(S/(8*TPC)) + 7 + 3 + log2(TPC)
  combine: ``world`` terms added in order -> world.  The kernel merges the ranks one
    by one (Chan et al., amd_dev.h welford_combine): mean += delta * n_b/n with
    delta = mean_b - mean rounds delta and the product at the size of |delta|, where the
    pooled sum pays only n_b/N of it - a one-element rank far from the rest costs
    eps32*|delta| either way round.  So e_mean carries 2*|delta_i| per merge step on top
    of the pooled formula's own magnitude (the variance, which sees the mean's error to
    second order only, does not).

Variance.  The budget is that of the documented algorithm (batch_norm.hip's header):
fp32 sums of d = x - k and d^2, k = the channel's first element (or the slab's shift),
finished in DOUBLE (m = s1/n, var = s2/n - m^2, mean = k + m, rounded to fp32 once).
So  e_mean = e_s1/n + |mean|  and  e_var = e_s2/n + 2|m|*e_s1/n + eps32*(e_s1/n)^2 + |var|
with e_s1 = (1 + chain)*sum|d|, e_s2 = (3 + chain)*sum d^2: S is written from sum(x - k)
and sum((x - k)^2) with that k and nothing else.  A two-pass kernel (k = mean) has a
smaller error and passes too; an unshifted one-pass E[x^2] - mean^2 in fp32
(``one_pass_stats``) does not: at mean/sigma = 1e5 its variance is off by hundreds of
sigma^2 (tests/test_bn_ref_cpu.py::test_one_pass_fails).  The algorithm's known cost is an
unlucky shift: with the channel's first element an outlier D = 100 sigma from the mean
("outlier_first") |m| ~ D and s2/n ~ D^2, so e_var ~ 3*chain*D^2: a variance budget of
K*eps32*3*chain*D^2, i.e. relative to the variance 1.4e-6*chain*D^2/var instead of about
1e-7*chain - 9 % for 700 rows of sigma = 2 behind a first element at 200 (chain 98, var 61
including the outlier's own D^2/n).  That is stated here, not hidden; such a channel is
still held to it, and its mean (budget K*eps32*chain*D, there 0.5 % of sigma) stays sharp.

Elementwise passes.  The values are those of the formulas above; the error magnitude of o
is the larger of the formula's own and that of the kernels' documented form
o = x*sc + sh, sc = invstd*w, sh = b - mean*sc (bn_common.h chan_affine), which rounds sh
at the magnitude of mean*sc: with statistics given exactly (e = 0) the formula's S would
vanish at x = mean while no evaluation of x*sc + sh can.  With the statistics of x the
two agree (e_mean >= |mean|, the rounding of the saved fp32 mean).  dx likewise pays for
e_mean through xhat; the kernels' dx = dy*k1 + x*k2 + k3 rounds k3 at |k2*mean|, which is
that same term.

ReLU.  o is discontinuous in the mask at 0, so ``make_inputs`` keeps every ReLU input off
it: an element is AMBIGUOUS if |o_ref| <= bound(o_ref) for the storage type, and the
generator nudges z (or, without a residual, x - and recomputes; the bias where o does not
depend on x: one element per channel, a zero weight) until there is none, asserting that
it converged.  Then the mask, y > 0 and the backward's d are all determined
and compared everywhere; nothing is excluded.

K.  As in norm_ref: the same formulas in float32 stay within 0.5*eps32*S to first order,
the kernels differ in order (fmaf, sc / sh / k1..k3 formed per channel) with at most
about twice the roundings, rsqrtf has up to 2 ulp: K = 4 keeps the float32 emulation under
half the bound.  Measured on the CPU against the reference alone (never on a kernel or
the extension): worst |ref32 - ref64| / (eps32 * S) over every case of
tests/test_batch_norm_gpu.py in fp32 / fp16 / bf16 storage
(tests/test_bn_ref_cpu.py::test_k_measured asserts these stay <= K/2):

    stats     mean 0.35  var 0.11  invstd 0.14  running_mean 0.33  running_var 0.34
    apply     o 0.33  y 0.33
    backward  sum_dy 0.05  sum_dy_xmu 0.31  dgamma 0.29  dbeta 0.05  dx 0.27  dz 0.00
    combine   mean 0.15  var 0.20  invstd 0.19  inv_total 0.19  running_mean 0.33
              running_var 0.26
    slab      mean 0.32  var 0.10  invstd 0.11  running_mean 0.32  running_var 0.22
              sum_dy 0.06  sum_dy_xmu 0.06  dgamma 0.32  dbeta 0.24

(All below 0.5: an output's single final rounding against S >= its own magnitude; the sums
sit far below because torch's float32 sums are pairwise while S budgets serial chains.)
K = 4 therefore leaves the emulation at a tenth of the bound.
"""
import math
from collections import namedtuple

import torch

from optim_ref import (EPS32, Val, assert_within, bound, emulation_ratio, f32,  # noqa: F401
                       worst_ratio)
from norm_ref import vrsqrt, vsum

K = 4.0
F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
THREADS = 256

# BNTuning defaults of csrc/include/bn_common.h, in bn.get_tuning()'s order
TUNING_KEYS = ("red_rpt", "red_cap", "red_min", "elem_rpt", "elem_cap", "elem_min")
DEFAULT_TUNING = dict(red_rpt=32, red_cap=1024, red_min=512, elem_rpt=8, elem_cap=16384,
                      elem_min=0)


def tuning(**kw):
    """The default tuning with ``kw`` changed (elem_rpt = 0: the per-shape rule)."""
    t = dict(DEFAULT_TUNING)
    t.update(kw)
    return t


def _cdiv(a, b):
    return -(-int(a) // int(b))


# --------------------------------------------------------------------------- geometry
# Pure-Python mirrors of the launchers' sizing (bn_nhwc.hip, batch_norm.hip, bn_common.h):
# they let the case lists state which condition each shape reaches and feed the chains.
NGeom = namedtuple("NGeom", "ctile rows_iter cblocks cv")


def ngeom(C, vec):
    cv = C // 8 if vec else C
    ctile = max(min(cv, 64), 1)
    return NGeom(ctile, THREADS // ctile, max(_cdiv(cv, ctile), 1), cv)


def _sized(M, g, rpt, floor_total, cap_total):
    want = _cdiv(M, g.rows_iter * rpt)
    floor_b = floor_total // g.cblocks
    max_by_rows = M // (g.rows_iter * 2)
    if want < floor_b:
        want = min(floor_b, max_by_rows)
    want = min(want, max(cap_total // g.cblocks, 1))
    return max(want, 1)


def reduce_splits(M, g, t=DEFAULT_TUNING):
    return _sized(M, g, t["red_rpt"], t["red_min"], t["red_cap"])


def elem_rpt_for(M, g, nbytes, t=DEFAULT_TUNING):
    if t["elem_rpt"] != 0:
        return t["elem_rpt"]
    if nbytes > 256 << 20:
        return 8
    r = 32
    while r > 8:
        if _cdiv(M, g.rows_iter * r) * g.cblocks >= 384:
            return r
        r >>= 1
    return 8


def elem_blocks(M, g, nbytes, t=DEFAULT_TUNING):
    return _sized(M, g, elem_rpt_for(M, g, nbytes, t), t["elem_min"], t["elem_cap"])


def nchw_splits(N, C, HW):
    want = min(_cdiv(2048, C), _cdiv(N * HW, 2048))
    return max(want, 1)


def elem_grid(items):
    return max(min(_cdiv(items, THREADS), 8192), 1)


def fin_ch(C):
    return 8 if C >= 1024 else 4 if C >= 512 else 2 if C >= 256 else 1


def slab_ch(S):
    ch = 1
    while ch < 32 and S * ch * 2 <= THREADS * 16:
        ch *= 2
    return ch


def u2_straddle(rows, rows_iter):
    """A pair (r, r + rows_iter) of the U = 2 loops over ``rows`` rows whose first row is
    valid and whose second is past the end (clamped)."""
    return any(r < rows <= r + rows_iter
               for base in range(0, rows, 2 * rows_iter) for r in range(base, base + rows_iter))


def view(shape, channels_last):
    """norm_ops.cpp bn_view: (cl, outer, C, inner).  ``channels_last``: a 4-D tensor stored
    in that memory format; HW = 1 (2-D included) always takes the NHWC kernels."""
    N, C = shape[0], shape[1]
    HW = 1
    for s in shape[2:]:
        HW *= s
    if HW == 1:
        return True, N, C, 1
    if channels_last:
        assert len(shape) == 4
        return True, N * HW, C, 1
    return False, N, C, HW


def slab_sum_chain(splits):
    return _cdiv(splits, THREADS) + 6 + 4


def nhwc_chain(M, C, t=DEFAULT_TUNING):
    out = 0
    for vec in ((False, True) if C % 8 == 0 else (False,)):
        g = ngeom(C, vec)
        s = reduce_splits(M, g, t)
        out = max(out, _cdiv(_cdiv(M, s), g.rows_iter) + g.rows_iter - 1 + slab_sum_chain(s))
    return float(out)


def nchw_chain(N, C, HW):
    L = N * HW
    s = nchw_splits(N, C, HW)
    per_thread = _cdiv(_cdiv(L, s), THREADS)
    if HW % 8 == 0:
        per_thread = max(per_thread, 8 * _cdiv(_cdiv(L // 8, s), THREADS))
    return float(per_thread + 10 + slab_sum_chain(s))


def red_chain(shape, channels_last, t=DEFAULT_TUNING):
    cl, outer, C, inner = view(shape, channels_last)
    return nhwc_chain(outer, C, t) if cl else nchw_chain(outer, C, inner)


def slab_chain(S):
    tpc = THREADS // slab_ch(S)
    return float(_cdiv(S, 8 * tpc) + 7 + 3 + int(math.log2(tpc)))


# --------------------------------------------------------------------------- helpers
def _cl(t, work):
    """[N, C, *] as stored -> [C, n] in ``work``."""
    return t.detach().to(work).movedim(1, 0).reshape(t.shape[1], -1)


def _back(val, shape):
    """[C, n] Val -> [N, C, *]."""
    def f(a):
        return a.reshape((shape[1], shape[0]) + tuple(shape[2:])).movedim(0, 1).contiguous()
    return Val(f(val.v), f(val.e))


def _asval(t, work):
    if isinstance(t, Val):
        return Val(t.v.detach().to(work), t.e.detach().to(work))
    return Val(t.detach().to(work))


def _col(val):
    return Val(val.v.reshape(-1, 1), val.e.reshape(-1, 1))


def _flat(val):
    return Val(val.v.reshape(-1), val.e.reshape(-1))


def _param(t, work):
    return None if t is None else Val(t.detach().to(work).reshape(-1, 1))


def _finish(s1, s2, k, n, eps, momentum, running_mean, running_var, work):
    """The stats finalize: fp32 shifted sums (Vals in ``work``) finished in double."""
    m_v, m_e = s1.v.to(F64) / n, s1.e.to(F64) / n
    q_v, q_e = s2.v.to(F64) / n, s2.e.to(F64) / n
    mean_v = k.to(F64) + m_v
    var_v = (q_v - m_v * m_v).clamp_min(0.0)
    mean = Val(mean_v.to(work), (m_e + mean_v.abs()).to(work))
    var = Val(var_v.to(work),
              (q_e + 2 * m_v.abs() * m_e + EPS32 * m_e * m_e + var_v.abs()).to(work))
    out = {"mean": mean, "var": var, "invstd": vrsqrt(var + f32(eps)),
           "running_mean": None, "running_var": None}
    if running_mean is not None:
        mom = f32(momentum)
        keep = mean.const(1.0) - mom
        f = float(n) / float(n - 1) if n > 1 else 1.0
        unb = Val((var_v * f).to(work), var.e * f)   # formed in double, rounded once
        out["running_mean"] = _asval(running_mean, work) * keep + mean * mom
        out["running_var"] = _asval(running_var, work) * keep + unb * mom
    return out


# --------------------------------------------------------------------------- references
def ref_stats(x, eps, chain, momentum=0.0, running_mean=None, running_var=None, work=F64):
    """-> mean, var (biased), invstd, running_mean, running_var (None without the stored
    ones; one momentum step from them), all [C]; count (int)."""
    X = _cl(x, work)
    n = X.shape[1]
    k = X[:, 0].clone()
    D = Val(X) - Val(k.reshape(-1, 1))
    s1 = vsum(D, 1, chain)
    s2 = vsum(D * D, 1, chain)
    return _finish(s1, s2, k, n, eps, momentum, running_mean, running_var, work)


def ref_slab_stats(slab, count, shift, eps, momentum=0.0, running_mean=None, running_var=None,
                   work=F64):
    """``slab``: fp32 [2][C][S] per-tile sums of (x - shift), (x - shift)^2."""
    S = slab.shape[2]
    chain = slab_chain(S)
    P = Val(slab.detach().to(work))
    s1 = vsum(Val(P.v[0]), 1, chain)
    s2 = vsum(Val(P.v[1]), 1, chain)
    k = shift.detach().to(work) if shift is not None else torch.zeros(slab.shape[1], dtype=work)
    return _finish(s1, s2, k, int(count), eps, momentum, running_mean, running_var, work)


def ref_slab_reduce(slab, invstd, sum_scale=None, gw0=None, gb0=None, work=F64):
    """``slab``: fp32 [2][C][S] per-tile (sum d, sum d*(x - mean)); invstd given."""
    chain = slab_chain(slab.shape[2])
    P = slab.detach().to(work)
    s1, s2 = vsum(Val(P[0]), 1, chain), vsum(Val(P[1]), 1, chain)
    iv = _asval(invstd, work)
    dg, db = s2 * iv, s1
    if gw0 is not None:
        dg, db = dg + _asval(gw0, work), db + _asval(gb0, work)
    if sum_scale is not None:
        s1, s2 = s1 * f32(sum_scale), s2 * f32(sum_scale)
    return {"sum_dy": s1, "sum_dy_xmu": s2, "dgamma": dg, "dbeta": db}


def ref_combine(means, vars_, counts, eps, momentum=0.0, running_mean=None, running_var=None,
                work=F64):
    """means / vars_: [world, C] (biased variances), counts: [world].
    -> mean, var, invstd [C], inv_total [1], running_mean, running_var."""
    M = Val(means.detach().to(work).reshape(-1, means.shape[-1]))
    V = Val(vars_.detach().to(work).reshape(M.v.shape))
    n = Val(counts.detach().to(work).reshape(-1, 1))
    world = M.v.shape[0]
    chain = float(world)
    N = vsum(n, 0, chain)
    mean = vsum(M * n, 0, chain) / N
    dm = M - Val(mean.v.reshape(1, -1), mean.e.reshape(1, -1))
    M2 = vsum((V + dm * dm) * n, 0, chain)
    var = M2 / N
    # the kernel merges rank by rank (welford_combine): each step rounds delta and
    # delta * n_b/n at the size of delta = mean_b - (running mean); see the docstring
    run, cnt, extra = torch.zeros_like(mean.v), 0.0, torch.zeros_like(mean.v)
    for i in range(world):
        delta = M.v[i] - run
        cnt += float(n.v[i])
        run = run + delta * (float(n.v[i]) / cnt)
        extra = extra + 2 * delta.abs()
    mean = Val(mean.v, mean.e + extra)
    out = {"mean": mean, "var": var, "invstd": vrsqrt(var + f32(eps)),
           "inv_total": N.const(1.0) / N, "running_mean": None, "running_var": None}
    if running_mean is not None:
        mom = f32(momentum)
        keep = mean.const(1.0) - mom
        unb = M2 / (N - 1.0) if float(N.v) > 1 else var
        out["running_mean"] = _asval(running_mean, work) * keep + mean * mom
        out["running_var"] = _asval(running_var, work) * keep + unb * mom
    return out


def ref_apply(x, mean, invstd, weight, bias, z, relu, work=F64):
    """mean / invstd: [C] tensors (exact) or Vals (e.g. ``ref_stats``' own).
    -> "o" (before the ReLU), "y", both Vals like x, and "mask" = o > 0 (bool like x)."""
    X = Val(_cl(x, work))
    mu, iv = _col(_asval(mean, work)), _col(_asval(invstd, work))
    W, B = _param(weight, work), _param(bias, work)
    Z = None if z is None else Val(_cl(z, work))
    o = (X - mu) * iv
    sc = iv
    if W is not None:
        o, sc = o * W, iv * W
    sh = (B if B is not None else Val(torch.zeros_like(mu.v))) - mu * sc
    oa = X * sc + sh          # the kernels' form: its error magnitude only
    if B is not None:
        o = o + B
    if Z is not None:
        o, oa = o + Z, oa + Z
    o = _back(Val(o.v, torch.maximum(o.e, oa.e)), x.shape)
    mask = o.v > 0
    # |relu(a) - relu(b)| <= |a - b|: y keeps o's error magnitude on both sides of zero
    y = Val(o.v.clamp_min(0.0), o.e) if relu else o
    return {"o": o, "y": y, "mask": mask}


def ref_backward(dy, x, mask, mean, invstd, weight, chain, sum_scale=None, gw0=None, gb0=None,
                 work=F64):
    """``mask``: bool like x (None: no ReLU).  mean / invstd as in ``ref_apply``.
    ``sum_scale``: the sums leave multiplied by it and dx uses them as the means.
    gw0 / gb0: stored gradients the accumulate form adds to.
    -> sum_dy, sum_dy_xmu, dgamma, dbeta [C]; dx, dz like x."""
    X = Val(_cl(x, work))
    d = _cl(dy, work)
    if mask is not None:
        d = d * _cl(mask, work)
    D = Val(d)
    n = X.v.shape[1]
    mu, iv = _col(_asval(mean, work)), _col(_asval(invstd, work))
    W = _param(weight, work)
    xm = X - mu
    s1 = vsum(D, 1, chain, keepdim=True)
    s2 = vsum(D * xm, 1, chain, keepdim=True)
    dg, db = s2 * iv, s1
    if gw0 is not None:
        dg, db = dg + _param(gw0, work), db + _param(gb0, work)
    if sum_scale is not None:
        s1, s2 = s1 * f32(sum_scale), s2 * f32(sum_scale)
        mdy, mdyx = s1, s2
    else:
        mdy, mdyx = s1 / float(n), s2 / float(n)
    g = iv if W is None else iv * W
    dx = (D - mdy - (xm * iv) * (mdyx * iv)) * g
    return {"sum_dy": _flat(s1), "sum_dy_xmu": _flat(s2), "dgamma": _flat(dg),
            "dbeta": _flat(db), "dx": _back(dx, x.shape), "dz": _back(D, x.shape)}


def one_pass_stats(x, eps, work=F32):
    """What an UNSHIFTED one-pass E[x^2] - mean^2 computes in ``work`` precision (plain
    tensors): the large-mean input is only worth something if THIS misses the bound.
    -> mean, var, invstd [C]."""
    X = _cl(x, work)
    mean = X.mean(1)
    var = ((X * X).mean(1) - mean * mean).clamp_min(0)
    return mean, var, (var + f32(eps)).rsqrt()


def ambiguous(o, dtype):
    """Elements whose ReLU condition the bound does not decide."""
    return o.v.abs() <= bound(o, dtype, K)


def mask_bytes(mask):
    """The ReLU bitmask of a [N, C, *] bool tensor as the NHWC apply writes it: uint8
    [M, C/8], byte [row][c/8], bit c & 7 (C % 8 == 0)."""
    C = mask.shape[1]
    m = mask.movedim(1, -1).reshape(-1, C // 8, 8).to(torch.int32)
    w = (1 << torch.arange(8, dtype=torch.int32)).reshape(1, 1, 8)
    return (m * w).sum(-1).to(torch.uint8)


# --------------------------------------------------------------------------- inputs
KINDS = ("randn", "large_mean", "outlier_first", "const", "allneg")
EPS = 1e-5
MOMENTUM = 0.1


def make_inputs(shape, dtype, wdtype, layout, kind="randn", relu=False, residual=False, seed=0,
                tune=None, affine=True):
    """Seeded CPU inputs for a [N, C, *] BatchNorm: dict of x, dy, z (None without
    ``residual``), weight, bias (None without ``affine``; in ``wdtype`` or x's type),
    running_mean, running_var (fp32).  ``layout``: "nhwc" (a 4-D tensor will be stored
    channels-last; 2-D is NHWC by nature) or "nchw" - it selects the summation chain of the
    ambiguity bound.  dy is drawn in fp32 and rounded to the type the kernel reads.
    With ``relu`` no element of o is ambiguous on return (asserted)."""
    shape = tuple(shape)
    C = shape[1]
    g = torch.Generator().manual_seed(seed * 1000003 + sum(shape) * 131 + C)
    r = torch.randn(shape, generator=g, dtype=F32)
    first = (0, slice(None)) + (0,) * (len(shape) - 2)
    if kind == "large_mean":
        x = 1000 + 0.01 * r if dtype == F32 else 8 + 0.25 * r     # mean/sigma = 1e5 in fp32
    else:
        x = r * 2 + 0.5
    if kind == "outlier_first":
        x[first] = 0.5 + 200.0                                    # 100 sigma
    if kind == "const":
        x[:, 0] = 0.5
    dy = torch.randn(shape, generator=g, dtype=F32)
    z = torch.randn(shape, generator=g, dtype=F32) if residual else None
    w = torch.rand(C, generator=g, dtype=F32) + 0.5
    b = torch.randn(C, generator=g, dtype=F32)
    if C >= 3:
        w[C - 1] = -w[C - 1]
        w[C // 2] = 0.0
    if C >= 16:
        w[5] = -w[5]
    if kind == "allneg":
        c = 1 % C
        w[c], b[c] = abs(float(w[c])) + 0.5, -100.0
    rm = torch.randn(C, generator=g, dtype=F32)
    rv = torch.rand(C, generator=g, dtype=F32) + 0.5
    wd = wdtype or dtype
    out = {"x": x.to(dtype), "dy": dy.to(dtype), "z": None if z is None else z.to(dtype),
           "weight": w.to(wd) if affine else None, "bias": b.to(wd) if affine else None,
           "running_mean": rm, "running_var": rv}
    if relu:
        _deambiguate(out, dtype, red_chain(shape, layout == "nhwc" and len(shape) == 4,
                                           tune or DEFAULT_TUNING))
    return out


def _deambiguate(inp, dtype, chain, rounds=8):
    """Move every ambiguous element of o off zero: through z where there is a residual,
    else through x (the statistics change, hence the rounds)."""
    for _ in range(rounds):
        st = ref_stats(inp["x"], EPS, chain)
        fw = ref_apply(inp["x"], st["mean"], st["invstd"], inp["weight"], inp["bias"],
                       inp["z"], True)
        amb = ambiguous(fw["o"], dtype)
        if not bool(amb.any()):
            return
        o = fw["o"]
        sign = torch.where(o.v < 0, -1.0, 1.0).to(F64)
        if inp["z"] is not None:
            t = inp["z"].to(F64)
            step = torch.maximum(4 * bound(o, dtype, K), t.abs() * 2.0 ** -5 + 2.0 ** -10)
            inp["z"] = torch.where(amb, t + sign * step, t).to(dtype)
        else:
            t = inp["x"].to(F64)
            cshape = (1, -1) + (1,) * (t.dim() - 2)
            if inp["weight"] is not None:
                ws = inp["weight"].to(F64).reshape(cshape)
                sign = sign * torch.where(ws < 0, -1.0, 1.0)
                # a channel whose o does not depend on x (one element per channel: xhat = 0;
                # a zero weight) is o = bias everywhere: move the bias instead
                dims = [0] + list(range(2, t.dim()))
                fixed = (ws.reshape(-1) == 0) | (t.numel() // t.shape[1] == 1)
                hit = amb.any(dims) & fixed
                if bool(hit.any()):
                    bt = inp["bias"].to(F64)
                    bstep = 4 * bound(o, dtype, K).amax(dims) + bt.abs() * 2.0 ** -5 + 2.0 ** -10
                    bsign = torch.where(bt < 0, -1.0, 1.0).to(F64)
                    inp["bias"] = torch.where(hit, bt + bsign * bstep, bt).to(inp["bias"].dtype)
            step = t.abs() * 2.0 ** -5 + 2.0 ** -6
            inp["x"] = torch.where(amb, t + sign * step, t).to(dtype)
    raise AssertionError("ambiguous ReLU elements remain after %d rounds" % rounds)


# --------------------------------------------------------------------------- case lists
# Shared by the CPU measurement of K / the geometry assertions and the GPU comparison.
# ``reaches``: names of the conditions (REACH below) the shape is in the list for.
Case = namedtuple("Case", "shape layout reaches offset tune")


def case(shape, layout, reaches, offset=0, tune=None):
    return Case(tuple(shape), layout, tuple(reaches.split()), offset, tune)


def rows_shape(M, C):
    """[M, C] rows as a 4-D channels-last [N, C, H, 1] where M has a small factor H > 1,
    else as the 2-D [M, C] itself."""
    for h in (2, 3, 5, 7):
        if M % h == 0 and M > h:
            return (M // h, C, h, 1)
    return (M, C)


def _n(M, C, reaches, **kw):
    return case(rows_shape(M, C), "nhwc", reaches, **kw)


NHWC_CASES = [
    # scalar path, C % 8 != 0
    _n(1, 3, "scalar m1 count1"), _n(2, 3, "scalar m2"), _n(3, 3, "scalar below_rows_iter"),
    _n(84, 3, "scalar rows_iter_minus1 idle_thread"), _n(86, 3, "scalar rows_iter_plus1 u2_tail"),
    _n(1003, 3, "scalar splits ragged_split"),
    _n(20, 12, "scalar rows_iter_minus1 idle_thread"), _n(22, 12, "scalar rows_iter_plus1"),
    _n(257, 12, "scalar splits ragged_split u2_tail"),
    _n(1, 20, "scalar m1 count1"), _n(11, 20, "scalar rows_iter_minus1"),
    _n(13, 20, "scalar rows_iter_plus1 u2_tail"), _n(100, 20, "scalar splits"),
    _n(3, 604, "scalar cblocks10 last_block_partial rows_iter_minus1 fin_ch4"),
    _n(5, 604, "scalar cblocks10 rows_iter_plus1 u2_tail"),
    _n(37, 604, "scalar cblocks10 splits ragged_split"),
    # C = 600 IS a multiple of 8 (75 lanes of 8: a second block with 11 lanes); its scalar
    # route - 10 channel blocks, the last with 24 of 64 lanes - is the misaligned one
    _n(5, 600, "vec cblocks last_block_partial u2_tail fin_ch4"),
    _n(37, 600, "vec cblocks last_block_partial splits ragged_split"),
    _n(5, 600, "misaligned cblocks10 last_block_partial", offset=1),
    _n(37, 600, "misaligned cblocks10 last_block_partial splits ragged_split", offset=1),
    # scalar path, misaligned pointer (a contiguous view one element into the storage)
    _n(5, 64, "misaligned rows_iter_plus1", offset=1), _n(130, 64, "misaligned splits", offset=1),
    # vector path
    _n(1, 8, "vec ctile1 m1 count1"), _n(255, 8, "vec ctile1 rows_iter_minus1"),
    _n(257, 8, "vec ctile1 rows_iter_plus1 u2_tail"), _n(1030, 8, "vec ctile1 splits"),
    _n(2, 24, "vec m2 idle_thread"), _n(84, 24, "vec rows_iter_minus1 idle_thread"),
    _n(86, 24, "vec rows_iter_plus1 u2_tail"), _n(702, 24, "vec splits ragged_split"),
    _n(7, 256, "vec rows_iter_minus1 fin_ch2"), _n(9, 256, "vec rows_iter_plus1 u2_tail"),
    _n(100, 256, "vec splits ragged_split fin_ch2"),
    _n(3, 512, "vec rows_iter_minus1 fin_ch4"), _n(5, 512, "vec rows_iter_plus1"),
    _n(64, 512, "vec splits fin_ch4"),
    _n(1, 520, "vec cblocks last_block_partial m1 count1"),
    _n(3, 520, "vec cblocks last_block_partial below_rows_iter"),
    _n(5, 520, "vec cblocks last_block_partial u2_tail"),
    _n(77, 520, "vec cblocks last_block_partial splits ragged_split fin_ch4"),
    _n(2, 1024, "vec cblocks m2 fin_ch8"), _n(45, 1024, "vec cblocks splits fin_ch8"),
    _n(3, 2048, "vec cblocks fin_ch8"),
    _n(1030, 2048, "vec cblocks splits empty_splits fin_ch8"),
]

NCHW_CASES = [
    case((4, 6, 7, 7), "nchw", "nchw hw_not8"),
    case((5, 16, 1, 1), "nchw", "hw1_is_nhwc vec"),
    case((5, 3, 1, 1), "nchw", "hw1_is_nhwc scalar"),
    case((3, 5, 8, 8), "nchw", "nchw nchw_vec"),
    case((3, 5, 8, 8), "nchw", "nchw nchw_misaligned", offset=1),
    case((5, 8, 24, 24), "nchw", "nchw nchw_vec nchw_splits split_off_sample"),
    case((5, 8, 23, 25), "nchw", "nchw hw_not8 nchw_splits split_off_sample"),
    case((4, 5, 10), "nchw", "nchw ndim3"),
    case((2, 3, 2, 3, 4), "nchw", "nchw ndim5 nchw_vec"),
    case((1, 2, 3, 3), "nchw", "nchw hw_not8"),
]
# more than 8192 * 256 scalar elements: the grid-stride loops run a second time
NCHW_BIG = case((2, 16, 257, 257), "nchw", "nchw hw_not8 nchw_splits grid_stride")

# loop edges through bn.set_tuning at small shapes
TUNED_CASES = [
    _n(700, 24, "vec one_split", tune=tuning(red_rpt=1, red_cap=1)),
    _n(257, 12, "scalar one_split", tune=tuning(red_rpt=1, red_cap=1)),
    _n(77, 520, "vec cblocks one_block_strides", tune=tuning(elem_cap=1)),
    _n(1003, 3, "scalar one_block_strides", tune=tuning(elem_cap=1)),
    _n(700, 24, "vec elem_auto", tune=tuning(elem_rpt=0)),
    _n(100, 256, "vec many_splits", tune=tuning(red_rpt=1, red_min=0)),
]

# types and options: one vector, one scalar NHWC shape and one NCHW shape
OPTION_CASES = [_n(77, 520, "vec cblocks"), _n(13, 20, "scalar"),
                case((4, 6, 7, 7), "nchw", "nchw hw_not8")]
TYPE_COMBOS = [(F32, F32), (F16, F32), (F16, F16), (BF16, F32), (BF16, BF16)]

# conditioning: (kind, dtype, case)
KIND_CASES = [(k, dt, c) for k in ("large_mean", "outlier_first", "const", "allneg")
              for dt in (F32, BF16)
              for c in (_n(700, 24, "vec splits"), _n(257, 12, "scalar splits"),
                        case((5, 8, 24, 24), "nchw", "nchw nchw_splits"))]

# ReLU modes: (relu, residual, want_mask)
MODES = {"none": (False, False, False), "relu": (True, False, False),
         "relu_z": (True, True, False), "relu_z_mask": (True, True, True)}

COMBINE_WORLDS = [(7,), (1, 30), (12, 1, 300)]      # counts per rank: a one-element rank
# slab_ch: 32 up to S = 128, then 16 / 8 / 4 / 2 per doubling, 1 above 2048 (200 and 1500 are
# here for 16 and 2); TPC = 8 threads per channel at 32: S = 1, 7 are below it, 64 is one
# pass of the unrolled loop with no tail, 65 adds a tail
SLAB_S = [1, 7, 64, 65, 128, 200, 300, 1024, 1500, 2049, 5000]
SLAB_C = [8, 64, 520]
FUSED_X2 = [(5, 520), (77, 520), (3, 2048), (45, 2048)]
MODULE_SHAPES = [(6, 20, 5, 3), (3, 520, 3, 2)]


def geom(c, esize=4):
    """What the launchers do with case ``c`` (default tuning unless the case has its own)."""
    t = c.tune or DEFAULT_TUNING
    cl, outer, C, inner = view(c.shape, c.layout == "nhwc" and len(c.shape) == 4)
    info = {"cl": cl, "M": outer, "C": C, "HW": inner, "ndim": len(c.shape),
            "elem_auto": t["elem_rpt"] == 0}
    if cl:
        vec = C % 8 == 0 and c.offset == 0
        g = ngeom(C, vec)
        s = reduce_splits(outer, g, t)
        per = _cdiv(outer, s)
        eb = elem_blocks(outer, g, outer * C * esize, t)
        info.update(vec=vec, g=g, splits=s, per=per, elem_blocks=eb, fin_ch=fin_ch(C),
                    elem_rpt=elem_rpt_for(outer, g, outer * C * esize, t))
    else:
        vec = inner % 8 == 0 and c.offset == 0
        s = nchw_splits(outer, C, inner)
        L = outer * inner
        info.update(vec=vec, splits=s, per=_cdiv(L // 8 if vec else L, s) * (8 if vec else 1),
                    items=outer * C * inner // (8 if vec else 1))
    return info


REACH = {
    "scalar": lambda i: i["cl"] and not i["vec"] and i["C"] % 8 != 0,
    "misaligned": lambda i: i["cl"] and not i["vec"] and i["C"] % 8 == 0,
    "vec": lambda i: i["cl"] and i["vec"],
    "ctile1": lambda i: i["g"].ctile == 1 and i["g"].rows_iter == 256,
    "idle_thread": lambda i: i["g"].ctile * i["g"].rows_iter < THREADS,
    "cblocks": lambda i: i["g"].cblocks > 1,
    "cblocks10": lambda i: i["g"].cblocks == 10 and i["g"].cv % i["g"].ctile != 0,
    "last_block_partial": lambda i: i["g"].cblocks > 1 and i["g"].cv % i["g"].ctile != 0,
    "fin_ch2": lambda i: i["fin_ch"] == 2,
    "fin_ch4": lambda i: i["fin_ch"] == 4,
    "fin_ch8": lambda i: i["fin_ch"] == 8,
    "m1": lambda i: i["M"] == 1,
    "count1": lambda i: i["M"] * i["HW"] == 1,
    "m2": lambda i: i["M"] == 2,
    "below_rows_iter": lambda i: i["M"] < i["g"].rows_iter,
    "rows_iter_minus1": lambda i: i["M"] == i["g"].rows_iter - 1,
    "rows_iter_plus1": lambda i: i["M"] == i["g"].rows_iter + 1,
    "u2_tail": lambda i: (u2_straddle(i["per"], i["g"].rows_iter)
                          and u2_straddle(i["M"], i["elem_blocks"] * i["g"].rows_iter)),
    "splits": lambda i: i["splits"] > 1,
    "ragged_split": lambda i: i["splits"] > 1 and i["M"] % i["splits"] != 0,
    "empty_splits": lambda i: (i["splits"] - 1) * i["per"] >= i["M"],
    "one_split": lambda i: i["splits"] == 1 and i["M"] > 2 * i["g"].rows_iter,
    "many_splits": lambda i: i["per"] <= i["g"].rows_iter,
    "one_block_strides": lambda i: (i["elem_blocks"] == 1
                                    and i["M"] > 2 * i["g"].rows_iter),
    "elem_auto": lambda i: i["elem_auto"] and i["elem_rpt"] in (8, 16, 32),
    "nchw": lambda i: not i["cl"],
    "hw1_is_nhwc": lambda i: i["cl"] and i["HW"] == 1 and i["ndim"] == 4,
    "hw_not8": lambda i: not i["cl"] and i["HW"] % 8 != 0 and not i["vec"],
    "nchw_vec": lambda i: not i["cl"] and i["vec"],
    "nchw_misaligned": lambda i: not i["cl"] and i["HW"] % 8 == 0 and not i["vec"],
    "nchw_splits": lambda i: not i["cl"] and i["splits"] > 1,
    "split_off_sample": lambda i: i["per"] % i["HW"] != 0,
    "ndim3": lambda i: i["ndim"] == 3,
    "ndim5": lambda i: i["ndim"] == 5,
    "grid_stride": lambda i: not i["vec"] and i["items"] > 8192 * THREADS,
}


def all_cases():
    return (NHWC_CASES + NCHW_CASES + [NCHW_BIG] + TUNED_CASES + OPTION_CASES
            + [c for _, _, c in KIND_CASES])


def slab_inputs(S, C, seed=0, with_shift=True, rows=2):
    """A synthetic statistics slab in the layout the conv epilogues write and the slab ops
    read (conv_igemm.hip: slab[(0|1)*C + c][s], i.e. fp32 [2][C][S] channel-major): per-tile
    sums a of (x - shift) over ``rows`` rows and a^2/rows + u >= their sums of squares
    (Cauchy-Schwarz keeps the variance non-negative).  -> slab, count, shift."""
    g = torch.Generator().manual_seed(seed * 7919 + S * 31 + C)
    a = torch.randn(C, S, generator=g, dtype=F32) * rows ** 0.5 + 0.3
    u = torch.rand(C, S, generator=g, dtype=F32) * rows
    slab = torch.stack([a, a * a / rows + u]).contiguous()
    shift = torch.randn(C, generator=g, dtype=F32) if with_shift else None
    return slab, S * rows, shift


def grad_slab_inputs(S, C, seed=0):
    """A synthetic backward slab [2][C][S] (sum d, sum d*(x - mean)) and an invstd."""
    g = torch.Generator().manual_seed(seed * 104729 + S * 17 + C)
    slab = torch.randn(2, C, S, generator=g, dtype=F32)
    return slab, torch.rand(C, generator=g, dtype=F32) + 0.5


def combine_inputs(counts, C, seed=0):
    """Per-rank batches of ``counts`` elements per channel -> (list of [n_i, C] fp32
    batches, means [world, C], biased vars [world, C], counts [world]) as gathered."""
    g = torch.Generator().manual_seed(seed * 15485863 + sum(counts) + C)
    xs = [torch.randn(n, C, generator=g, dtype=F32) * (1 + i) + 0.5 * i
          for i, n in enumerate(counts)]
    means = torch.stack([x.double().mean(0) for x in xs]).to(F32)
    vars_ = torch.stack([x.double().var(0, unbiased=False) for x in xs]).to(F32)
    return xs, means, vars_, torch.tensor([float(n) for n in counts], dtype=F32)


def ref_all(x, dy, z, weight, bias, running_mean, running_var, *, chain, relu, mask=None,
            work=F64):
    """Forward and backward of one training step from the reference's own statistics
    (``mask``: the float64 run's, given, so that an emulation shares it)."""
    st = ref_stats(x, EPS, chain, MOMENTUM, running_mean, running_var, work=work)
    fw = ref_apply(x, st["mean"], st["invstd"], weight, bias, z, relu, work=work)
    m = (fw["mask"] if mask is None else mask) if relu else None
    bw = ref_backward(dy, x, m, st["mean"], st["invstd"], weight, chain, work=work)
    out = {k: st[k] for k in ("mean", "var", "invstd", "running_mean", "running_var")}
    out.update(o=fw["o"], y=fw["y"], **bw)
    return out, fw["mask"]
