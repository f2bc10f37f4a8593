"""The fused optimizer kernels (csrc/hip/mt_optim.hip) against the one-step float64
references of tests/optim_ref.py, at every dtype combination the dispatch can produce,
every option, device scalars, tile-edge sizes and misaligned pointers, with sentinel guard
bands around every tensor; skipped steps (noop flag) leave every output bitwise unchanged,
down to amp O2 runs whose overflow steps must be as if they never happened; unsupported
dtypes raise instead of launching nothing.  Tolerance and K: see optim_ref."""
import pytest
import torch
import torch.nn.functional as F

import optim_ref as R
from optim_ref import (ADAM_OPTS, BETAS, LAMB_OPTS, NOVO_OPTS, SGD_OPTS, global_norm,
                       grad_norms)

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
# where the indexing changes: the 8-element vector, the 2,048-element unroll stride, the
# 4,096-element half tile of Adam / LAMB, the 8,192-element tile; several tiles; nothing
SIZES = [1, 7, 8, 9, 2047, 2048, 2049, 4095, 4097, 8191, 8192, 8193, 16385, 3 * 8192 + 5, 0]
W4 = (24, 40, 3, 3)   # a channels_last weight: dense, not contiguous
SHAPES = [(n,) for n in SIZES] + [W4]
SENT = -1234.0        # guard bands
COPY_FILL = 7.0       # 16-bit copies before the kernel writes them
PADS = [16, 17]       # 17: every pointer misaligned (aligned == 0 in the tensor table)


def _amp_C():
    from apex_example_amd import amp_C

    return amp_C


def _mt():
    from apex_example_amd import _native

    return _native.require().mt


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _pmag(i):
    return 10.0 ** (i % 5 - 2)


def _gmag(i):
    return 10.0 ** ((2 * i) % 5 - 3)


def _dt(spec, i):
    """A dtype, or a tuple of dtypes the tensors take in turn (mixed-dtype lists)."""
    return spec[i % len(spec)] if isinstance(spec, tuple) else spec


class Pool:
    """Every tensor is the slice base[pad : pad + n] of its own sentinel-filled buffer."""

    def __init__(self, pad, shapes=SHAPES):
        self.pad, self.shapes, self.bases = pad, shapes, []

    def one(self, values, dtype):
        n, pad = values.numel(), self.pad
        base = torch.full((n + 2 * pad,), SENT, dtype=dtype, device=DEV)
        t = base[pad:pad + n]
        if values.dim() == 4:   # same memory, NHWC order
            s = values.shape
            t = t.view(s[0], s[2], s[3], s[1]).permute(0, 3, 1, 2)
        t.copy_(values)
        assert (t.data_ptr() % 16 == 0) == (pad % 8 == 0) or n == 0
        self.bases.append((base, n))
        return t

    def make(self, spec, seed, kind="randn", mag=_pmag, mul=1.0):
        g = torch.Generator().manual_seed(seed)
        out = []
        for i, shape in enumerate(self.shapes):
            x = torch.randn(shape, generator=g, dtype=F64) * (mag(i) * mul)
            if kind == "sq":
                x = x * x
            elif kind == "zero":
                x = x * 0
            elif kind == "fill":
                x = x * 0 + COPY_FILL
            out.append(self.one(x, _dt(spec, i)))
        return out

    def check_bands(self):
        bad = torch.zeros((), dtype=torch.bool, device=DEV)
        for base, n in self.bases:
            want = _bits(torch.full((self.pad,), SENT, dtype=base.dtype, device=DEV))
            bad |= (_bits(base[:self.pad]) != want).any()
            bad |= (_bits(base[self.pad + n:]) != want).any()
        assert not bool(bad), "a kernel wrote outside its tensor"


def _clone(ts):
    return [t.clone() for t in ts]


def _noop(v=0):
    return torch.full((1,), v, dtype=torch.int32, device=DEV)


def _scalars(dev):
    """(stored-grad multiplier, scale argument, scale_inv, lr argument) - as device tensors
    (loss scale 128 applied as its reciprocal) or as plain numbers."""
    if dev:
        return (128.0, torch.tensor([128.0], device=DEV), True,
                lambda lr: torch.tensor([lr], device=DEV))
    return 1.0, 1.0, False, lambda lr: lr


def _assert_copy(c, p):
    """The kernel stores the same fp32 registers twice: the copy is the stored p, cast."""
    assert torch.equal(_bits(c), _bits(p.to(c.dtype)))


# --------------------------------------------------------------------------- SGD
def _run_sgd(gt, pt, ct, o, pad, flag_mode="bool", dev=False, steps=3):
    amp_C, mt = _amp_C(), _mt()
    gmul, scale, inv, lr_of = _scalars(dev)
    pool = Pool(pad)
    p, m = pool.make(pt, 1), pool.make(pt, 2, kind="zero")
    c = pool.make(ct, 0, kind="fill") if ct is not None else None
    flag = _noop(0) if flag_mode == "flag" else None
    noop = _noop()
    for step in range(1, steps + 1):
        g = pool.make(gt, 10 + step, mag=_gmag, mul=gmul)
        p0, m0 = _clone(p), _clone(m)
        first = step == 1
        amp_C.multi_tensor_sgd(65536, noop, [g, p, m] + ([c] if c else []), o["wd"],
                               o["momentum"], o["dampening"], lr_of(0.05), o["nesterov"],
                               first if flag is None else False, o["wd_after_momentum"], scale,
                               scale_inv=inv, first_run_flag=flag)
        if flag is not None:
            mt.mark_step_done(flag, noop)
        for i in range(len(p)):
            r = R.ref_sgd(g[i], p0[i], m0[i], lr=0.05, first_run=first, scale=scale,
                          scale_inv=inv, **o)
            R.assert_within(p[i], r["p"], "sgd p[%d]" % i)
            if r["m"] is None:
                assert torch.equal(_bits(m[i]), _bits(m0[i]))
            else:
                R.assert_within(m[i], r["m"], "sgd m[%d]" % i)
            if c:
                _assert_copy(c[i], p[i])
        pool.check_bands()
    if flag is not None:
        assert flag.item() == 1


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("gt,pt", [(F32, F32), (F16, F16), (BF16, BF16), (BF16, F32), (F16, F32),
                                   ((F32, BF16), (F32, BF16))])
def test_sgd_depth3(gt, pt, pad):
    """Every (grad, param) pairing, and fp32 + bf16 params mixed in one call."""
    _run_sgd(gt, pt, None, SGD_OPTS[1], pad, steps=2)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("gt,ct", [(BF16, BF16), (F16, F16), (F32, BF16), (F32, F16)])
def test_sgd_depth4(gt, ct, pad):
    _run_sgd(gt, F32, ct, SGD_OPTS[2], pad, steps=2)


@pytest.mark.parametrize("gt,pt,ct", [(F32, F32, None), (BF16, F32, BF16), (F16, F16, None)])
@pytest.mark.parametrize("o", range(len(SGD_OPTS)))
def test_sgd_options(o, gt, pt, ct):
    _run_sgd(gt, pt, ct, SGD_OPTS[o], 16)
    if SGD_OPTS[o]["dampening"] != 0:   # the first run decided by the device flag
        _run_sgd(gt, pt, ct, SGD_OPTS[o], 16, flag_mode="flag")


def test_sgd_device_scalars():
    _run_sgd(BF16, F32, BF16, SGD_OPTS[4], 17, flag_mode="flag", dev=True)
    _run_sgd(F32, F32, None, SGD_OPTS[1], 16, dev=True)


def _pair_sets(pool_a, pool_b, gt, ct):
    """Set A [g16|32, p32, m32, c16] and set B [g32, p32, m32] with their StepPlans; the
    grads are read from the owners (A: the copies, B: the params)."""
    mt = _mt()
    pa, ma = pool_a.make(F32, 1), pool_a.make(F32, 2, mag=_gmag)
    ca = pool_a.make(ct, 0, kind="fill")
    pb, mb = pool_b.make(F32, 3), pool_b.make(F32, 4, mag=_gmag)
    return (pa, ma, ca, mt.StepPlan(ca, [pa, ma, ca])), (pb, mb, mt.StepPlan(pb, [pb, mb]))


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("gt,ct", [(BF16, BF16), (F16, F16)])
def test_sgd_pair(gt, ct, pad):
    """Two launch sets in ONE launch (StepPlan.sgd_pair), each with its own scale: both
    halves match the reference and the pair launch is what ran."""
    pool_a, pool_b = Pool(pad), Pool(pad, [(5,), (2049,), (0,), (8193,), (12, 8, 3, 3)])
    (pa, ma, ca, plan_a), (pb, mb, plan_b) = _pair_sets(pool_a, pool_b, gt, ct)
    o = SGD_OPTS[2]
    sa = torch.tensor([128.0], device=DEV)
    noop = _noop()
    for step in (1, 2):
        ga = pool_a.make(gt, 10 + step, mag=_gmag, mul=128.0)
        gb = pool_b.make(F32, 20 + step, mag=_gmag, mul=2.0)
        for owner, g in zip(ca + pb, ga + gb):
            owner.grad = g
        pa0, ma0, pb0, mb0 = _clone(pa), _clone(ma), _clone(pb), _clone(mb)
        took = plan_a.sgd_pair(plan_b, noop, o["wd"], o["momentum"], 0.0, 0.05, o["nesterov"],
                               o["wd_after_momentum"], 1.0, sa, True, 0.5, None, False)
        assert took is True
        for i in range(len(pa)):
            r = R.ref_sgd(ga[i], pa0[i], ma0[i], lr=0.05, first_run=False, scale=128.0,
                          scale_inv=True, **o)
            R.assert_within(pa[i], r["p"], "pair A p[%d]" % i)
            R.assert_within(ma[i], r["m"], "pair A m[%d]" % i)
            _assert_copy(ca[i], pa[i])
        for i in range(len(pb)):
            r = R.ref_sgd(gb[i], pb0[i], mb0[i], lr=0.05, first_run=False, scale=0.5, **o)
            R.assert_within(pb[i], r["p"], "pair B p[%d]" % i)
            R.assert_within(mb[i], r["m"], "pair B m[%d]" % i)
        pool_a.check_bands()
        pool_b.check_bands()


# --------------------------------------------------------------------------- Adam
GRID16 = [(F32, F32), (F16, F16), (BF16, BF16), (BF16, F32), (F16, F32)]
GRID_COPY = [(BF16, BF16), (F16, F16), (F32, BF16), (F32, F16)]
MIXED = ((F32, BF16), (F32, BF16))


def _run_adam(gt, pt, ct, o, pad, dev=False, steps=3, betas=BETAS):
    amp_C, mt = _amp_C(), _mt()
    gmul, scale, inv, lr_of = _scalars(dev)
    pool = Pool(pad)
    p, m = pool.make(pt, 1), pool.make(pt, 2, mag=_gmag)
    v = pool.make(pt, 3, kind="sq", mag=_gmag)
    c = pool.make(ct, 0, kind="fill") if ct is not None else None
    noop = _noop()
    step_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    for step in range(1, steps + 1):
        g = pool.make(gt, 10 + step, mag=_gmag, mul=gmul)
        p0, m0, v0 = _clone(p), _clone(m), _clone(v)
        amp_C.multi_tensor_adam(65536, noop, [g, p, m, v] + ([c] if c else []), lr_of(0.01),
                                betas["beta1"], betas["beta2"], 1e-8,
                                step_t if dev else step, o["mode"], o["bias_correction"],
                                o["wd"], scale=scale, scale_inv=inv)
        mt.advance_step(step_t, noop)
        for i in range(len(p)):
            r = R.ref_adam(g[i], p0[i], m0[i], v0[i], lr=0.01, eps=1e-8, step=step, scale=scale,
                           scale_inv=inv, **betas, **o)
            for name, got in (("p", p), ("m", m), ("v", v)):
                R.assert_within(got[i], r[name], "adam %s[%d]" % (name, i))
            if c:
                _assert_copy(c[i], p[i])
        pool.check_bands()
    assert step_t.item() == steps


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("gt,pt", GRID16 + [MIXED])
def test_adam_depth4(gt, pt, pad):
    _run_adam(gt, pt, None, ADAM_OPTS[0], pad, steps=2)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("gt,ct", GRID_COPY)
def test_adam_depth5(gt, ct, pad):
    _run_adam(gt, F32, ct, ADAM_OPTS[2], pad, steps=2)


@pytest.mark.parametrize("gt,pt,ct", [(F32, F32, None), (BF16, F32, BF16), (F16, F16, None)])
@pytest.mark.parametrize("o", range(len(ADAM_OPTS)))
def test_adam_options(o, gt, pt, ct):
    _run_adam(gt, pt, ct, ADAM_OPTS[o], 16)


def test_adam_device_scalars_and_default_betas():
    _run_adam(BF16, F32, BF16, ADAM_OPTS[0], 17, dev=True)
    _run_adam(F32, F32, None, ADAM_OPTS[2], 16, dev=True, betas=dict(beta1=0.9, beta2=0.999))


# --------------------------------------------------------------------------- LAMB
def _run_lamb(gt, pt, ct, o, pad, dev=False, steps=3, norm_as_tensor=True):
    amp_C = _amp_C()
    o = dict(o)
    clip = o.pop("clip")
    gmul, scale, inv, lr_of = _scalars(dev)
    pool = Pool(pad)
    p, m = pool.make(pt, 1), pool.make(pt, 2, mag=_gmag)
    v = pool.make(pt, 3, kind="sq", mag=_gmag)
    c = pool.make(ct, 0, kind="fill") if ct is not None else None
    noop = _noop()
    step_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    for step in range(1, steps + 1):
        g = pool.make(gt, 10 + step, mag=_gmag, mul=gmul)
        gn = torch.tensor([global_norm(g, gmul)], dtype=F32, device=DEV)
        mx = clip * float(gn)
        p0, m0, v0 = _clone(p), _clone(m), _clone(v)
        amp_C.multi_tensor_lamb(65536, noop, [g, p, m, v], lr_of(0.01), BETAS["beta1"],
                                BETAS["beta2"], 1e-6, step_t if dev else step,
                                o["bias_correction"], o["wd"], o["grad_averaging"], o["mode"],
                                gn if norm_as_tensor else float(gn), mx, o["use_nvlamb"],
                                model_copies=c, scale=scale, scale_inv=inv)
        _mt().advance_step(step_t, noop)
        for i in range(len(p)):
            r = R.ref_lamb(g[i], p0[i], m0[i], v0[i], lr=0.01, eps=1e-6, step=step,
                           global_grad_norm=gn, max_grad_norm=mx, scale=scale, scale_inv=inv,
                           m_stored=m[i], v_stored=v[i], **BETAS, **o)
            for name, got in (("p", p), ("m", m), ("v", v)):
                R.assert_within(got[i], r[name], "lamb %s[%d]" % (name, i))
            if c:
                _assert_copy(c[i], p[i])
        pool.check_bands()


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("gt,pt", GRID16 + [MIXED])
def test_lamb_depth4(gt, pt, pad):
    """With mixed lists the per-tensor norms must stay attached to their tensors across
    the dtype groups (every tensor has its own magnitude, so its own trust ratio)."""
    _run_lamb(gt, pt, None, LAMB_OPTS[0], pad, steps=2)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("gt,ct", GRID_COPY)
def test_lamb_depth5(gt, ct, pad):
    _run_lamb(gt, F32, ct, LAMB_OPTS[1], pad, steps=2)


@pytest.mark.parametrize("gt,pt,ct", [(F32, F32, None), (BF16, F32, BF16), (BF16, BF16, None)])
@pytest.mark.parametrize("o", range(len(LAMB_OPTS)))
def test_lamb_options(o, gt, pt, ct):
    _run_lamb(gt, pt, ct, LAMB_OPTS[o], 16, norm_as_tensor=(o % 2 == 0))


def test_lamb_device_scalars():
    _run_lamb(BF16, F32, BF16, LAMB_OPTS[1], 17, dev=True)
    _run_lamb(F32, F32, None, LAMB_OPTS[3], 16, dev=True)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("gt,pt", [(F32, F32), (BF16, BF16), (F16, F32)])
def test_lamb_legacy_stages(gt, pt, pad):
    """Legacy stage 1 (per-tensor decay, clip on and off) and stage 2 (given norms; a
    zero-norm tensor takes trust ratio 1)."""
    amp_C = _amp_C()
    noop = _noop()
    for clip in (0.5, 2.0):
        pool = Pool(pad)
        g, p = pool.make(gt, 11, mag=_gmag), pool.make(pt, 1)
        m, v = pool.make(pt, 2, mag=_gmag), pool.make(pt, 3, kind="sq", mag=_gmag)
        u = pool.make(pt, 0, kind="fill")
        p[3].zero_()
        decay = torch.tensor([0.01 * (i % 4) for i in range(len(p))], device=DEV)
        gn = global_norm(g, 1.0)
        p0, m0, v0 = _clone(p), _clone(m), _clone(v)
        amp_C.multi_tensor_lamb_stage1_cuda(65536, noop, [g, p, m, v, u], decay, 2, 0.9, 0.99,
                                            1e-6, torch.tensor(gn, device=DEV), clip * gn)
        for i in range(len(p)):
            r = R.ref_lamb_legacy1(g[i], p0[i], m0[i], v0[i], decay=decay[i], step=2, beta1=0.9,
                                   beta2=0.99, eps=1e-6, global_grad_norm=gn,
                                   max_grad_norm=clip * gn)
            for name, got in (("m", m), ("v", v), ("u", u)):
                R.assert_within(got[i], r[name], "legacy %s[%d]" % (name, i))
            assert torch.equal(_bits(p[i]), _bits(p0[i]))
        pn = torch.stack([x.double().norm() for x in p]).float()
        un = torch.stack([x.double().norm() for x in u]).float()
        assert pn[3].item() == 0.0
        u0 = _clone(u)
        amp_C.multi_tensor_lamb_stage2_cuda(65536, noop, [p, u], pn, un, 0.01, 0.01, False)
        for i in range(len(p)):
            r = R.ref_lamb_legacy2(p0[i], u0[i], param_norm=pn[i], update_norm=un[i], lr=0.01,
                                   wd=0.01, use_nvlamb=False)
            R.assert_within(p[i], r["p"], "legacy p[%d]" % i)
            assert torch.equal(_bits(u[i]), _bits(u0[i]))
        pool.check_bands()


# --------------------------------------------------------------------------- NovoGrad
def _run_novograd(gt, pt, o, pad, init_zero=False, dev=False, flag_mode="bool", steps=3):
    mt = _mt()
    gmul, scale, inv, lr_of = _scalars(dev)
    pool = Pool(pad)
    p, m = pool.make(pt, 1), pool.make(pt, 2, mag=_gmag)
    vvec = pool.one(torch.zeros(len(p), dtype=F64), F32)
    noop = _noop()
    flag = _noop(0) if flag_mode == "flag" else None
    step_t = torch.zeros(1, dtype=torch.int32, device=DEV)
    sv, st = (1.0, scale) if dev else (scale, None)
    for step in range(1, steps + 1):
        g = pool.make(gt, 10 + step, mag=_gmag, mul=gmul)
        gn = pool.one(grad_norms(g, gmul, o["norm_type"]).double(), F32)
        p0, m0, v0 = _clone(p), _clone(m), vvec.clone()
        first = step == 1 and not init_zero
        mt.novograd(noop, [g, p, m], vvec, gn, first if flag is None else False, flag, 0.01,
                    lr_of(0.01) if dev else None, BETAS["beta1"], BETAS["beta2"], 1e-8,
                    0 if dev else step, step_t if dev else None, o["bias_correction"], o["wd"],
                    o["grad_averaging"], o["mode"], o["norm_type"], sv, st, inv)
        mt.advance_step(step_t, noop)
        if flag is not None:
            mt.mark_step_done(flag, noop)
        for i in range(len(p)):
            r = R.ref_novograd(g[i], p0[i], m0[i], v_old=v0[i], grad_norm=gn[i],
                               first_step=first, lr=0.01, eps=1e-8, step=step, scale=scale,
                               scale_inv=inv, **BETAS, **o)
            R.assert_within(vvec[i], r["v"], "novograd v[%d]" % i)
            R.assert_within(p[i], r["p"], "novograd p[%d]" % i)
            R.assert_within(m[i], r["m"], "novograd m[%d]" % i)
        pool.check_bands()


STATE_GRID = [(F32, F32), (BF16, F32), (BF16, BF16), (F16, F16)]


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("gt,pt", STATE_GRID)
def test_novograd_types(gt, pt, pad):
    _run_novograd(gt, pt, NOVO_OPTS[0], pad, steps=2)


@pytest.mark.parametrize("gt,pt", [(F32, F32), (BF16, BF16)])
@pytest.mark.parametrize("o", range(len(NOVO_OPTS)))
def test_novograd_options(o, gt, pt):
    _run_novograd(gt, pt, NOVO_OPTS[o], 16)


def test_novograd_seed_init_zero_and_device_scalars():
    """First-step seed (host bool and device flag) against init_zero's blend from 0."""
    _run_novograd(BF16, F32, NOVO_OPTS[0], 16, init_zero=True)
    _run_novograd(BF16, F32, NOVO_OPTS[4], 16, flag_mode="flag")
    _run_novograd(BF16, F32, NOVO_OPTS[3], 17, dev=True, flag_mode="flag")
    _run_novograd(F32, F32, NOVO_OPTS[2], 16, dev=True)


# --------------------------------------------------------------------------- Adagrad
def _run_adagrad(gt, pt, mode, pad, dev=False, steps=3):
    amp_C = _amp_C()
    gmul, scale, inv, lr_of = _scalars(dev)
    pool = Pool(pad)
    p, h = pool.make(pt, 1), pool.make(pt, 3, kind="sq", mag=_gmag)
    noop = _noop()
    for step in range(1, steps + 1):
        g = pool.make(gt, 10 + step, mag=_gmag, mul=gmul)
        p0, h0 = _clone(p), _clone(h)
        amp_C.multi_tensor_adagrad(65536, noop, [g, p, h], lr_of(0.05), 1e-10, mode, 0.02,
                                   scale=scale, scale_inv=inv)
        for i in range(len(p)):
            r = R.ref_adagrad(g[i], p0[i], h0[i], lr=0.05, eps=1e-10, mode=mode, wd=0.02,
                              scale=scale, scale_inv=inv)
            R.assert_within(p[i], r["p"], "adagrad p[%d]" % i)
            R.assert_within(h[i], r["h"], "adagrad h[%d]" % i)
        pool.check_bands()


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("gt,pt", STATE_GRID + [MIXED])
def test_adagrad_types(gt, pt, pad):
    _run_adagrad(gt, pt, 0, pad, steps=2)


@pytest.mark.parametrize("gt,pt", [(F32, F32), (BF16, BF16)])
@pytest.mark.parametrize("mode", [0, 1])
def test_adagrad_modes(mode, gt, pt):
    _run_adagrad(gt, pt, mode, 16)


def test_adagrad_device_scalars():
    _run_adagrad(BF16, F32, 1, 17, dev=True)


# --------------------------------------------------------------------------- skipped steps
def _frozen(tensors, call):
    """``call()`` with the noop flag set must leave every tensor bitwise unchanged."""
    before = [_bits(t).clone() for t in tensors]
    call()
    torch.cuda.synchronize()
    for k, (b, t) in enumerate(zip(before, tensors)):
        assert torch.equal(b, _bits(t)), "tensor %d changed on a skipped step" % k


@pytest.mark.parametrize("kernel", ["sgd3", "sgd4", "sgd_pair", "adam4", "adam5", "lamb4", "lamb5",
                                    "legacy1", "legacy2", "novograd", "adagrad"])
def test_noop_flag_freezes_every_output(kernel):
    """noop = 1: p, all state, the 16-bit copies (prefilled with a value that is not p), the
    NovoGrad v vector, the device step counter and the first-run flag keep their bits."""
    amp_C, mt = _amp_C(), _mt()
    pool = Pool(17)
    noop = _noop(1)
    gt, ct = BF16, BF16
    g = pool.make(gt, 11, mag=_gmag, mul=128.0)
    p, m = pool.make(F32, 1), pool.make(F32, 2, mag=_gmag)
    v, c = pool.make(F32, 3, kind="sq", mag=_gmag), pool.make(ct, 0, kind="fill")
    step_t = torch.full((1,), 3, dtype=torch.int32, device=DEV)
    flag = _noop(0)
    sc = torch.tensor([128.0], device=DEV)
    lr = torch.tensor([0.05], device=DEV)
    gn = torch.tensor([global_norm(g, 128.0)], dtype=F32, device=DEV)
    vvec = pool.one(torch.linspace(0.5, 2.0, len(p), dtype=F64), F32)
    per = pool.one(torch.linspace(1.0, 3.0, len(p), dtype=F64), F32)   # != vvec: a seed shows
    extra = []
    if kernel in ("sgd3", "sgd4"):
        lists = [g, p, m] + ([c] if kernel == "sgd4" else [])

        def call():
            amp_C.multi_tensor_sgd(65536, noop, lists, 0.01, 0.9, 0.1, lr, False, False, False,
                                   sc, scale_inv=True, first_run_flag=flag)
    elif kernel == "sgd_pair":
        pool_b = Pool(17, [(5,), (8193,)])
        (pa, ma, ca, plan_a), (pb, mb, plan_b) = _pair_sets(pool, pool_b, gt, ct)
        gb = pool_b.make(F32, 21, mag=_gmag)
        for owner, gr in zip(ca + pb, g + gb):
            owner.grad = gr
        extra = pa + ma + ca + pb + mb

        def call():
            assert plan_a.sgd_pair(plan_b, noop, 0.01, 0.9, 0.0, 0.05, False, False, 1.0, sc,
                                   True, 1.0, None, False) is True
    elif kernel in ("adam4", "adam5"):
        lists = [g, p, m, v] + ([c] if kernel == "adam5" else [])

        def call():
            amp_C.multi_tensor_adam(65536, noop, lists, lr, 0.9, 0.99, 1e-8, step_t, 0, True,
                                    0.1, scale=sc, scale_inv=True)
    elif kernel in ("lamb4", "lamb5"):
        def call():
            amp_C.multi_tensor_lamb(65536, noop, [g, p, m, v], lr, 0.9, 0.99, 1e-6, step_t, True,
                                    0.01, True, 1, gn, 0.5 * float(gn), False,
                                    model_copies=c if kernel == "lamb5" else None, scale=sc,
                                    scale_inv=True)
    elif kernel == "legacy1":
        g32 = pool.make(F32, 12, mag=_gmag)
        u = pool.make(F32, 0, kind="fill")
        extra = g32 + u

        def call():
            amp_C.multi_tensor_lamb_stage1_cuda(65536, noop, [g32, p, m, v, u], per, 2, 0.9, 0.99,
                                                1e-6, gn, 0.5 * float(gn))
    elif kernel == "legacy2":
        def call():
            amp_C.multi_tensor_lamb_stage2_cuda(65536, noop, [p, m], per, vvec, 0.01, 0.01, True)
    elif kernel == "novograd":
        def call():
            mt.novograd(noop, [g, p, m], vvec, per, False, flag, 0.01, lr, 0.9, 0.99, 1e-8, 0,
                        step_t, True, 0.01, True, 1, 2, 1.0, sc, True)
    else:
        def call():
            amp_C.multi_tensor_adagrad(65536, noop, [g, p, v], lr, 1e-10, 0, 0.02, scale=sc,
                                       scale_inv=True)

    def step():
        call()
        mt.advance_step(step_t, noop)
        mt.mark_step_done(flag, noop)

    _frozen(g + p + m + v + c + extra + [vvec, per, step_t, flag, noop], step)
    assert step_t.item() == 3 and flag.item() == 0
    pool.check_bands()


def _o2_run(opt_name, kw, norm, inject=(), feed=None):
    """amp O2 (bf16, sync-free, raw 16-bit grads read by the kernels) on a three-layer model
    Linear -> ``norm`` -> Linear.  amp keeps BatchNorm parameters fp32 (a 16-bit and an fp32
    launch set per group); LayerNorm is cast with the rest (one 16-bit set).
    Without ``feed``: 5 iterations, an inf written into one grad on the iterations of
    ``inject``; returns the (grads, loss scale) of the clean ones.  With ``feed``: one
    iteration per recorded entry, whose grads replace the computed ones (times the exact
    power-of-two ratio of the loss scales)."""
    import apex_example_amd.optimizers as O
    from apex_example_amd import amp
    from apex_example_amd.amp import amp as amp_mod

    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(24, 40), getattr(torch.nn, norm)(40),
                                torch.nn.Linear(40, 8)).to(DEV)
    opt = getattr(O, opt_name)(model.parameters(), materialize_master_grads=False, **kw)
    model, opt = amp.initialize(model, opt, opt_level="O2", half_dtype=BF16, verbosity=0)
    scaler = amp._amp_state.loss_scalers[0]
    assert scaler.sync_free and scaler.dynamic
    x = torch.randn(16, 24, device=DEV)
    y = torch.randint(0, 8, (16,), device=DEV)
    params = list(model.parameters())
    recorded = []
    for it in range(5 if feed is None else len(feed)):
        loss = F.cross_entropy(model(x).float(), y)
        opt.zero_grad()
        with amp.scale_loss(loss, opt) as s:
            s.backward()
            scale = scaler.loss_scale()
            if feed is not None:
                grads, scale_a = feed[it]
                for p, g in zip(params, grads):
                    p.grad.copy_(g.double() * (scale / scale_a))
            elif it in inject:
                params[0].grad[0].fill_(float("inf"))
            else:
                recorded.append(([p.grad.clone() for p in params], scale))
        opt.step()
    torch.cuda.synchronize()
    sets = opt._set_cache[0][2]
    assert sorted(str(s["grads"][0].dtype) for s in sets.values()) == \
        ["torch.bfloat16"] + ["torch.float32"] * (norm == "BatchNorm1d")
    masters = list(amp.master_params(opt))
    out = {"scale": scaler.loss_scale()}
    for i, p in enumerate(params):
        out["model%d" % i] = p.detach().clone()
    for i, p in enumerate(masters):
        out["master%d" % i] = p.detach().clone()
        for k, t in sorted(opt.state[p].items()):
            if isinstance(t, torch.Tensor):
                out["state%d.%s" % (i, k)] = t.detach().clone()
    for i, t in enumerate(opt.param_groups[0].get("exp_avg_sq", [])):
        out["novograd_v%d" % i] = t.clone()
    for k, t in opt._dev_steps.items():
        out["dev_step%s" % (k,)] = t.clone()
    for k, t in opt._dev_flags.items():
        out["dev_flag%s" % (k,)] = t.clone()
    amp_mod.deinit()
    amp._amp_state.handle = None
    return recorded, out


@pytest.mark.parametrize("opt_name,kw", [
    ("FusedSGD", dict(lr=0.05, momentum=0.9, weight_decay=1e-4)),
    ("FusedSGD", dict(lr=0.05, momentum=0.9, dampening=0.1)),
    ("FusedAdam", dict(lr=1e-2, weight_decay=0.01)),
    ("FusedLAMB", dict(lr=1e-2, weight_decay=0.01, max_grad_norm=0.05)),
    ("FusedNovoGrad", dict(lr=1e-2, bias_correction=True)),
    ("FusedNovoGrad", dict(lr=1e-2, bias_correction=False)),
    ("FusedNovoGrad", dict(lr=1e-2, bias_correction=False, norm_type=0, init_zero=True)),
    ("FusedAdagrad", dict(lr=1e-2)),
], ids=lambda v: v if isinstance(v, str) else "-".join("%s=%s" % kv for kv in v.items()))
@pytest.mark.parametrize("norm", ["LayerNorm", "BatchNorm1d"])
def test_overflow_steps_never_happened(opt_name, kw, norm):
    """Overflows on iterations 1 and 3 of 5 (the very first step among them): masters,
    model copies, every piece of optimizer state, the device step counters and first-run
    flags equal, bitwise, a run fed the same grads in which those two steps never were."""
    recorded, a = _o2_run(opt_name, kw, norm, inject=(0, 2))
    assert len(recorded) == 3 and [s for _, s in recorded] == [2.0 ** 15, 2.0 ** 14, 2.0 ** 14]
    _, b = _o2_run(opt_name, kw, norm, feed=recorded)
    assert a["scale"] == 2.0 ** 14 and b["scale"] == 2.0 ** 16
    assert sorted(a) == sorted(b)
    assert any(k.startswith("state") for k in a) and any(k.startswith("master") for k in a)
    for k in sorted(a):
        if k == "scale":
            continue
        assert a[k].dtype == b[k].dtype and torch.equal(_bits(a[k]), _bits(b[k])), k
    assert all(int(v) == 3 for k, v in a.items() if k.startswith("dev_step"))


# --------------------------------------------------------------------------- rejected inputs
def _d(n=5, dtype=F64):
    return [torch.ones(n, dtype=dtype, device=DEV)]


DOUBLE = "float32 / float16 / bfloat16"


@pytest.mark.parametrize("op", ["scale", "check_finite", "norm", "axpby", "zero", "sgd", "adam",
                                "lamb", "legacy1", "legacy2", "novograd", "adagrad"])
def test_double_tensors_raise(op):
    """The kernels are instantiated for fp32 / fp16 / bf16: a GPU double tensor is an
    error in every multi-tensor op, not a launch of nothing that reports success."""
    amp_C, mt = _amp_C(), _mt()
    noop = _noop()
    f = torch.ones(1, device=DEV)
    calls = {
        "scale": lambda: amp_C.multi_tensor_scale(65536, noop, [_d(), _d()], 0.5),
        "check_finite": lambda: amp_C.multi_tensor_check_finite(65536, noop, [_d()]),
        "norm": lambda: amp_C.multi_tensor_l2norm(65536, noop, [_d()], True),
        "axpby": lambda: amp_C.multi_tensor_axpby(65536, noop, [_d(), _d(), _d()], 1.0, 1.0, -1),
        "zero": lambda: amp_C.multi_tensor_zero(65536, noop, [_d()]),
        "sgd": lambda: amp_C.multi_tensor_sgd(65536, noop, [_d(), _d(), _d()], 0.0, 0.9, 0.0,
                                              0.1, False, False, False, 1.0),
        "adam": lambda: amp_C.multi_tensor_adam(65536, noop, [_d(), _d(), _d(), _d()], 0.01, 0.9,
                                                0.99, 1e-8, 1, 0, True, 0.0),
        "lamb": lambda: amp_C.multi_tensor_lamb(65536, noop, [_d(), _d(), _d(), _d()], 0.01, 0.9,
                                                0.99, 1e-6, 1, True, 0.0, True, 1, f, 1.0),
        "legacy1": lambda: amp_C.multi_tensor_lamb_stage1_cuda(
            65536, noop, [_d(), _d(), _d(), _d(), _d()], f, 1, 0.9, 0.99, 1e-6, f, 1.0),
        "legacy2": lambda: amp_C.multi_tensor_lamb_stage2_cuda(65536, noop, [_d(), _d()], f, f,
                                                               0.01),
        "novograd": lambda: amp_C.multi_tensor_novograd(65536, noop, [_d(), _d(), _d()], f, 0.01,
                                                        0.9, 0.99, 1e-8, 1, True, 0.0, True, 1, 2),
        "adagrad": lambda: amp_C.multi_tensor_adagrad(65536, noop, [_d(), _d(), _d()], 0.01,
                                                      1e-10, 0, 0.0),
    }
    with pytest.raises(RuntimeError, match=DOUBLE):
        calls[op]()


def test_double_tensors_raise_in_the_plan():
    mt = _mt()
    with pytest.raises(RuntimeError, match=DOUBLE):
        mt.StepPlan(_d(), [_d(), _d()])
    # fp32 params, a double grad: rejected when the plan reads the grad
    p, m, v = _d(dtype=F32), _d(dtype=F32), _d(dtype=F32)
    p[0].grad = None
    owner = torch.ones(5, dtype=F64, device=DEV)
    owner.grad = torch.ones(5, dtype=F64, device=DEV)
    noop = _noop()
    with pytest.raises(RuntimeError, match=DOUBLE):
        mt.StepPlan([owner], [p, m]).sgd(noop, 0.0, 0.9, 0.0, 0.1, False, False, None, False,
                                         1.0, None, False)
    with pytest.raises(RuntimeError, match=DOUBLE):
        mt.StepPlan([owner], [p, m, v]).adam(noop, 0.01, None, 0.9, 0.99, 1e-8, 1, None, 0, True,
                                             0.0, 1.0, None, False, False)
    gn = torch.ones(1, device=DEV)
    with pytest.raises(RuntimeError, match=DOUBLE):
        mt.StepPlan([owner], [p, m, v]).lamb(noop, 0.01, None, 0.9, 0.99, 1e-6, 1, None, True,
                                             0.0, True, 1, gn, 1.0, False, 1.0, None, False,
                                             False)
    with pytest.raises(RuntimeError, match=DOUBLE):
        mt.StepPlan([owner], [p]).grad_norm_into(torch.zeros(1, device=DEV), 0, _noop(), 1.0,
                                                 None)


def test_state_dtype_mismatch_raises():
    """Momentum / exp_avg / sum of another dtype than the parameter would be read and
    written at the parameter's width: rejected before any launch, in the op and the plan."""
    amp_C, mt = _amp_C(), _mt()
    noop = _noop()
    g, p, s16 = _d(dtype=F32), _d(dtype=F32), _d(dtype=BF16)
    c = _d(dtype=BF16)
    with pytest.raises(RuntimeError, match="sgd: momentum must match the parameter dtype"):
        amp_C.multi_tensor_sgd(65536, noop, [g, p, s16], 0.0, 0.9, 0.0, 0.1, False, False, False,
                               1.0)
    with pytest.raises(RuntimeError, match="novograd: exp_avg must match the parameter dtype"):
        mt.novograd(noop, [g, p, s16], torch.ones(1, device=DEV), torch.ones(1, device=DEV), True,
                    None, 0.01, None, 0.9, 0.99, 1e-8, 1, None, True, 0.0, True, 1, 2, 1.0, None,
                    False)
    with pytest.raises(RuntimeError, match="adagrad: sum must match the parameter dtype"):
        amp_C.multi_tensor_adagrad(65536, noop, [g, p, s16], 0.01, 1e-10, 0, 0.0)
    p[0].grad = g[0]
    c[0].grad = _d(dtype=BF16)[0]
    with pytest.raises(RuntimeError, match="sgd: momentum must match the parameter dtype"):
        mt.StepPlan(p, [p, s16]).sgd(noop, 0.0, 0.9, 0.0, 0.1, False, False, None, False, 1.0,
                                     None, False)
    with pytest.raises(RuntimeError, match="sgd: momentum must match the parameter dtype"):
        mt.StepPlan(c, [p, s16, c]).sgd_pair(mt.StepPlan(p, [p, _d(dtype=F32)]), noop, 0.0, 0.9,
                                             0.0, 0.1, False, False, 1.0, None, False, 1.0, None,
                                             False)
    with pytest.raises(RuntimeError, match="adam: exp_avg / exp_avg_sq must match"):
        mt.StepPlan(p, [p, s16, _d(dtype=F32)]).adam(noop, 0.01, None, 0.9, 0.99, 1e-8, 1, None,
                                                     0, True, 0.0, 1.0, None, False, False)
    assert torch.equal(p[0], torch.ones(5, device=DEV)) and torch.equal(
        s16[0], torch.ones(5, dtype=BF16, device=DEV))
