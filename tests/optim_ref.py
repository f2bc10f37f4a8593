"""One-step float64 references of the fused multi-tensor optimizers (csrc/hip/mt_optim.hip),
shared by tests/test_optim_ref_cpu.py (the references are right) and
tests/test_optim_kernels_gpu.py (the kernels match them).

Every ``ref_*`` function takes the tensors AS STORED (fp32 / fp16 / bf16) and the scalar
arguments as the kernels receive them (rounded to float32, ``f32``), upcasts to float64
and applies the documented update ONCE, written from the math:

  SGD       d = g*s (+ wd*p);  m = d (first run) | mu*m + (1-damp)*d;
            d = d + mu*m (nesterov) | m;  (+ wd*p after momentum);  p -= lr*d
  Adam      d = g*s (+ wd*p, mode 0);  m = b1*m + (1-b1)*d;  v = b2*v + (1-b2)*d^2;
            u = (m/bc1) / (sqrt(v/bc2) + eps) (+ wd*p, mode 1);  p -= lr*u
  LAMB      d = g*s/clip (+ wd*p, mode 0);  m = b1*m + b3*d;  v as Adam;  u as Adam, formed
            from m, v AS STORED in the parameter type (documented kernel behaviour);
            p -= lr * (||p|| / ||u||) * u   (plain lr without wd / nvlamb or for a zero norm)
  NovoGrad  v_t = ||g|| (seed) | sqrt(b2*v^2 + (1-b2)*||g||^2) | b2*v + (1-b2)*||g||_inf;
            d = g*s / (v/sqrt(bc2) + eps) (+ wd*p, mode 0);  m = b1*m + b3*d;
            p -= lr * (m/bc1 (+ wd*p, mode 1))
  Adagrad   d = g*s (+ wd*p, mode 0);  h += d^2;  p -= lr * (d/(sqrt(h)+eps) (+ wd*p, mode 1))

Nothing is rounded: results are ``Val`` objects holding the float64 value ``v`` and a
running first-order error magnitude ``e`` (below).  A multi-step test feeds each step from
what the device stored at the previous one, so storage rounding never accumulates.

Tolerance.  An output stored in type T must satisfy, elementwise,

    |got - ref| <= u_T*|ref| + tiny_T + K*eps32*S

with u_T = eps_T/2 (the one rounding to storage), tiny_T = smallest_normal_T * eps_T/2
(half a subnormal spacing) and S = ``Val.e``: the sum of the magnitudes of every
intermediate result the output depends on, propagated through the formula (running error
analysis: each operation adds |result|, a product adds |a|*e_b + |b|*e_a, a quotient and a
square root their first-order terms).  For p this is |p_new| + c*|lr*update| + ...; it also
carries the conditioning of 1 - beta^step, which no fp32 evaluation can avoid.

K.  With S defined this way the same formula evaluated in float32 in the same order is
bounded by 0.5*eps32*S to first order (u = eps32/2 per operation); powf enters with 2 ulp.
The kernels evaluate in a different order (fmaf, lr/bc1, rsqrtf(bc2), 1/(v/sqrt(bc2)+eps))
with at most about twice the operations on any path and intrinsics of up to 2 ulp, which
gives K = 0.5 * 2 * 2 = 2; K = 4 keeps the float32 emulation under HALF the bound with
room to spare.  Measured on the CPU against the reference alone (never on a kernel):
worst |ref32 - ref64| / (eps32 * S) over 2*10^5 random elements per optimizer, every
option and fp32 / fp16 / bf16 storage (tests/test_optim_ref_cpu.py::test_k_measured
asserts these stay <= K/2):

    sgd       p 0.50  m 0.49            adam      p 0.50  m 0.48  v 0.49
    lamb      p 0.50  m 0.49  v 0.49  ||p|| 0.03  ||u|| 0.10
    legacy    p 0.50  m 0.48  v 0.49  u 0.44
    novograd  p 0.50  m 0.49  v 0.08  adagrad   p 0.50  h 0.50

(0.50 is the final rounding of an output whose last term dominates - half an ulp against
S ~ |value|: the first-order bound is attained, never exceeded.)  K = 4 therefore leaves
the emulation at one eighth of the bound.
"""
import torch

EPS32 = torch.finfo(torch.float32).eps
K = 4.0
# longest chain of additions in a per-tensor sum of squares (32 fmaf per thread, an
# 8-level block tree, the per-chunk finalize): each adds one rounding of the running sum
NORM_CHAIN = 48.0


def f32(x):
    """A scalar argument as the kernels receive it: rounded to float32."""
    if isinstance(x, torch.Tensor):
        x = x.reshape(-1)[0].item()
    return float(torch.tensor(float(x), dtype=torch.float32))


class Val:
    """A float64 value ``v`` with ``e``, the first-order error magnitude (in units of
    eps32) of evaluating it in float32.  Stored inputs are exact (e = 0)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    def const(self, x):
        return Val(torch.as_tensor(float(x), dtype=self.v.dtype, device=self.v.device))

    def _c(self, o):
        return o if isinstance(o, Val) else self.const(o)

    def __add__(self, o):
        o = self._c(o)
        v = self.v + o.v
        return Val(v, self.e + o.e + v.abs())

    __radd__ = __add__

    def __sub__(self, o):
        o = self._c(o)
        v = self.v - o.v
        return Val(v, self.e + o.e + v.abs())

    def __rsub__(self, o):
        return self._c(o) - self

    def __mul__(self, o):
        o = self._c(o)
        v = self.v * o.v
        return Val(v, self.v.abs() * o.e + o.v.abs() * self.e + v.abs())

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._c(o)
        v = self.v / o.v
        return Val(v, self.e / o.v.abs() + v.abs() * o.e / o.v.abs() + v.abs())

    def __rtruediv__(self, o):
        return self._c(o) / self

    def sqrt(self):
        r = self.v.sqrt()
        inf = torch.full_like(r, float("inf"))
        # sqrt(0) of an exactly-zero argument is exact; of a cancelled one, unbounded here
        prop = torch.where(r > 0, self.e / (2 * r), torch.where(self.e > 0, inf, self.e))
        return Val(r, prop + r)

    def sumsq(self):
        """sum(x^2) as the norm kernels form it (a tree of fp32 additions)."""
        sq = self * self
        v = sq.v.sum()
        return Val(v, sq.e.sum() + NORM_CHAIN * v)


def _leaf(t, work):
    return Val(t.detach().to(work))


def _scale(P, scale, scale_inv):
    s = P.const(f32(scale))
    return P.const(1.0) / s if scale_inv else s


def _bias_corrections(P, on, beta1, beta2, step):
    """1 - beta^step (powf: 2 ulp), or 1 without bias correction."""
    if not on:
        return P.const(1.0), P.const(1.0)
    out = []
    for b in (beta1, beta2):
        pw = P.const(b).v ** int(step)
        out.append(P.const(1.0) - Val(pw, 2 * pw.abs()))
    return out


# --------------------------------------------------------------------------- SGD
def ref_sgd(g, p, m, *, wd, momentum, dampening, lr, nesterov, first_run, wd_after_momentum,
            scale=1.0, scale_inv=False, work=torch.float64):
    """-> {"p": Val, "m": Val or None (no momentum: the buffer is not touched)}."""
    wd, momentum, dampening, lr = f32(wd), f32(momentum), f32(dampening), f32(lr)
    G, P, M = _leaf(g, work), _leaf(p, work), _leaf(m, work)
    d = G * _scale(P, scale, scale_inv)
    if wd != 0 and not wd_after_momentum:
        d = d + P * wd
    Mn = None
    if momentum != 0:
        Mn = d if first_run else M * momentum + d * (P.const(1.0) - dampening)
        d = d + Mn * momentum if nesterov else Mn
    if wd != 0 and wd_after_momentum:
        d = d + P * wd
    return {"p": P - d * lr, "m": Mn}


# --------------------------------------------------------------------------- Adam
def ref_adam(g, p, m, v, *, lr, beta1, beta2, eps, step, mode, bias_correction, wd, scale=1.0,
             scale_inv=False, work=torch.float64):
    """``step`` is the number of this step (1 for the first).  mode 0: L2, 1: AdamW."""
    lr, beta1, beta2, eps, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd)
    G, P, M, V = (_leaf(t, work) for t in (g, p, m, v))
    one = P.const(1.0)
    d = G * _scale(P, scale, scale_inv)
    if mode == 0:
        d = d + P * wd
    Mn = M * beta1 + d * (one - beta1)
    Vn = V * beta2 + d * d * (one - beta2)
    bc1, bc2 = _bias_corrections(P, bias_correction, beta1, beta2, step)
    u = (Mn / bc1) / ((Vn / bc2).sqrt() + eps)
    if mode == 1:
        u = u + P * wd
    return {"p": P - u * lr, "m": Mn, "v": Vn}


# --------------------------------------------------------------------------- LAMB
def _clip(P, global_grad_norm, max_grad_norm, need_positive_max):
    gn, mx = f32(global_grad_norm), f32(max_grad_norm)
    if gn > mx and (mx > 0 or not need_positive_max):
        return P.const(gn) / mx
    return P.const(1.0)


def _trust_ratio(P, lr, pn, un, active):
    if active and float(pn.v) != 0.0 and float(un.v) != 0.0:
        return (pn / un) * lr
    return P.const(lr)


def ref_lamb(g, p, m, v, *, lr, beta1, beta2, eps, step, bias_correction, wd, grad_averaging,
             mode, global_grad_norm, max_grad_norm, use_nvlamb, scale=1.0, scale_inv=False,
             m_stored=None, v_stored=None, work=torch.float64):
    """One tensor.  The kernel forms u from m / v as stored in the parameter type: for a
    16-bit parameter pass what the device stored (``m_stored`` / ``v_stored``, checked
    against "m" / "v" separately); without them the float64 m / v are rounded here.
    -> p, m, v, pnorm (||p_old||), unorm (||u||)."""
    lr, beta1, beta2, eps, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd)
    G, P, M, V = (_leaf(t, work) for t in (g, p, m, v))
    one = P.const(1.0)
    d = G * (_scale(P, scale, scale_inv) / _clip(P, global_grad_norm, max_grad_norm, True))
    if mode == 0:
        d = d + P * wd
    beta3 = (one - beta1) if grad_averaging else one
    Mn = M * beta1 + d * beta3
    Vn = V * beta2 + d * d * (one - beta2)
    if p.dtype == torch.float32:
        Ms, Vs = Mn, Vn
    else:
        Ms = _leaf(m_stored if m_stored is not None else Mn.v.to(p.dtype), work)
        Vs = _leaf(v_stored if v_stored is not None else Vn.v.to(p.dtype), work)
    bc1, bc2 = _bias_corrections(P, bias_correction, beta1, beta2, step)
    u = (Ms / bc1) / ((Vs / bc2).sqrt() + eps)
    if mode == 1:
        u = u + P * wd
    pn, un = P.sumsq().sqrt(), u.sumsq().sqrt()
    ratio = _trust_ratio(P, lr, pn, un, use_nvlamb or wd != 0)
    return {"p": P - u * ratio, "m": Mn, "v": Vn, "pnorm": pn, "unorm": un}


def ref_lamb_legacy1(g, p, m, v, *, decay, step, beta1, beta2, eps, global_grad_norm,
                     max_grad_norm, work=torch.float64):
    """Legacy stage 1: Adam moments of the clipped grad, u = m^/(sqrt(v^)+eps) + decay*p.
    The bias corrections reach the kernel as float32 values computed on the host."""
    bc1, bc2 = f32(1.0 - float(beta1) ** int(step)), f32(1.0 - float(beta2) ** int(step))
    beta1, beta2, eps, decay = f32(beta1), f32(beta2), f32(eps), f32(decay)
    G, P, M, V = (_leaf(t, work) for t in (g, p, m, v))
    one = P.const(1.0)
    d = G / _clip(P, global_grad_norm, max_grad_norm, False)
    Mn = M * beta1 + d * (one - beta1)
    Vn = V * beta2 + d * d * (one - beta2)
    u = (Mn / bc1) / ((Vn / bc2).sqrt() + eps) + P * decay
    return {"m": Mn, "v": Vn, "u": u}


def ref_lamb_legacy2(p, u, *, param_norm, update_norm, lr, wd, use_nvlamb, work=torch.float64):
    """Legacy stage 2: p -= lr * (||p|| / ||u||) * u with the norms GIVEN (trust ratio 1 for a
    zero norm, plain lr without weight decay / nvlamb)."""
    lr, wd = f32(lr), f32(wd)
    P, U = _leaf(p, work), _leaf(u, work)
    pn, un = P.const(f32(param_norm)), P.const(f32(update_norm))
    ratio = _trust_ratio(P, lr, pn, un, use_nvlamb or wd != 0)
    return {"p": P - U * ratio}


# --------------------------------------------------------------------------- NovoGrad
def ref_novograd(g, p, m, *, v_old, grad_norm, first_step, lr, beta1, beta2, eps, step,
                 bias_correction, wd, grad_averaging, mode, norm_type, scale=1.0,
                 scale_inv=False, work=torch.float64):
    """One tensor; ``v_old`` / ``grad_norm`` are its entries of the per-tensor fp32 vectors
    (the norm of the UNSCALED grad).  first_step seeds v with the grad norm.
    -> p, m, v (0-dim)."""
    lr, beta1, beta2, eps, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd)
    G, P, M = (_leaf(t, work) for t in (g, p, m))
    one = P.const(1.0)
    gn, vo = P.const(f32(grad_norm)), P.const(f32(v_old))
    if first_step:
        vn = gn
    elif norm_type == 2:
        vn = (vo * vo * beta2 + gn * gn * (one - beta2)).sqrt()
    else:
        vn = vo * beta2 + gn * (one - beta2)
    bc1, bc2 = _bias_corrections(P, bias_correction, beta1, beta2, step)
    d = G * _scale(P, scale, scale_inv) / (vn / bc2.sqrt() + eps)
    if mode == 0:
        d = d + P * wd
    beta3 = (one - beta1) if grad_averaging else one
    Mn = M * beta1 + d * beta3
    u = Mn / bc1
    if mode == 1:
        u = u + P * wd
    return {"p": P - u * lr, "m": Mn, "v": vn}


# --------------------------------------------------------------------------- Adagrad
def ref_adagrad(g, p, h, *, lr, eps, mode, wd, scale=1.0, scale_inv=False, work=torch.float64):
    """mode 0: L2 (wd*p joins the grad), 1: decoupled (wd*p joins the update)."""
    lr, eps, wd = f32(lr), f32(eps), f32(wd)
    G, P, H = (_leaf(t, work) for t in (g, p, h))
    d = G * _scale(P, scale, scale_inv)
    if mode == 0:
        d = d + P * wd
    Hn = H + d * d
    u = d / (Hn.sqrt() + eps)
    if mode == 1:
        u = u + P * wd
    return {"p": P - u * lr, "h": Hn}


# --------------------------------------------------------------------------- tolerance
def bound(ref, dtype, k=K):
    """u_T*|ref| + tiny_T + k*eps32*S for an output stored in ``dtype``."""
    fi = torch.finfo(dtype)
    return (fi.eps / 2) * ref.v.abs() + fi.smallest_normal * fi.eps / 2 + k * EPS32 * ref.e


def worst_ratio(got, ref, k=K):
    """max |got - ref| / bound over the elements (0 for an empty tensor); inf if ``got``
    holds a non-finite value where the reference is finite."""
    if ref.v.numel() == 0:
        return 0.0
    g64 = got.detach().to(torch.float64)
    err = (g64 - ref.v.to(g64.device)).abs()
    r = err / bound(ref, got.dtype, k).to(g64.device)
    r = torch.where(torch.isfinite(g64), r, torch.full_like(r, float("inf")))
    return float(r.max())


def assert_within(got, ref, what, k=K):
    """``got`` (as stored by the code under test) is within the bound of ``ref``."""
    assert got.shape == ref.v.shape or ref.v.dim() == 0, (what, got.shape, ref.v.shape)
    r = worst_ratio(got, ref, k)
    print("%-40s worst |err| / bound = %.3f" % (what, r))
    assert r <= 1.0, "%s: |err| / bound = %g" % (what, r)


def emulation_ratio(fn, *tensors, **kw):
    """The K measurement: worst |fn in float32 - fn in float64| / (eps32 * S) per output
    (a bound with K = that value would just hold the float32 emulation)."""
    r64 = fn(*tensors, work=torch.float64, **kw)
    r32 = fn(*tensors, work=torch.float32, **kw)
    out = {}
    for name, a in r64.items():
        if a is None:
            continue
        err = (r32[name].v.to(torch.float64) - a.v).abs()
        ok = torch.isfinite(a.e) & (a.e > 0)
        r = torch.where(ok, err / (EPS32 * a.e), torch.zeros_like(err))
        assert bool((err[~ok & torch.isfinite(a.e)] == 0).all()), name
        out[name] = float(r.max()) if r.numel() else 0.0
    return out


# --------------------------------------------------------------------------- test cases
# The option sets both test files walk (every option of every optimizer at least once on
# and once off), and the norms the LAMB / NovoGrad calls take as inputs.
F32 = torch.float32
SGD_OPTS = [dict(momentum=0.0, nesterov=False, wd_after_momentum=False, dampening=0.0, wd=0.01),
            dict(momentum=0.9, nesterov=False, wd_after_momentum=False, dampening=0.0, wd=0.01),
            dict(momentum=0.9, nesterov=True, wd_after_momentum=False, dampening=0.0, wd=0.01),
            dict(momentum=0.9, nesterov=False, wd_after_momentum=True, dampening=0.0, wd=0.01),
            dict(momentum=0.9, nesterov=False, wd_after_momentum=False, dampening=0.1, wd=0.0)]


ADAM_OPTS = [dict(mode=m, bias_correction=b, wd=0.1) for m in (0, 1) for b in (True, False)]
BETAS = dict(beta1=0.9, beta2=0.99)


# max_grad_norm is given relative to the global grad norm: 0.5 clips, 2 does not, 0 is off
LAMB_OPTS = [
    dict(mode=1, grad_averaging=True, use_nvlamb=False, wd=0.01, bias_correction=True, clip=2.0),
    dict(mode=0, grad_averaging=True, use_nvlamb=False, wd=0.01, bias_correction=True, clip=0.5),
    dict(mode=1, grad_averaging=False, use_nvlamb=False, wd=0.0, bias_correction=False, clip=0.0),
    dict(mode=1, grad_averaging=True, use_nvlamb=True, wd=0.0, bias_correction=True, clip=0.5),
    dict(mode=0, grad_averaging=False, use_nvlamb=True, wd=0.01, bias_correction=True, clip=0.0),
    dict(mode=1, grad_averaging=True, use_nvlamb=False, wd=0.0, bias_correction=True, clip=2.0),
]


def global_norm(gs, gmul):
    return float(torch.cat([g.double().flatten() for g in gs]).norm()) / gmul


NOVO_OPTS = [
    dict(norm_type=2, mode=1, grad_averaging=True, bias_correction=True, wd=0.01),
    dict(norm_type=0, mode=1, grad_averaging=True, bias_correction=True, wd=0.01),
    dict(norm_type=2, mode=0, grad_averaging=False, bias_correction=True, wd=0.01),
    dict(norm_type=0, mode=0, grad_averaging=True, bias_correction=False, wd=0.01),
    dict(norm_type=2, mode=1, grad_averaging=False, bias_correction=False, wd=0.0),
]


def grad_norms(gs, gmul, norm_type):
    """Per-tensor norms of the UNSCALED grads, as the fp32 vector the op takes."""
    f = (lambda x: x.abs().max() if x.numel() else x.sum()) if norm_type == 0 else torch.norm
    return torch.stack([f(g.double().flatten()) / gmul for g in gs]).to(F32)
