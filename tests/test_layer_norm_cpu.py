"""The CPU branch of the LayerNorm / RMSNorm operators (``!x.is_cuda()`` in
csrc/torch/norm_ops.cpp) against the float64 references of tests/norm_ref.py, through
FusedLayerNorm / FusedRMSNorm on CPU tensors and through the operators themselves (for the
saved statistics).  No GPU needed; the built extension is.

The branch computes in float32 with ATen elementwise operations and reductions in the
order of the reference's formulas: it IS the float32 emulation that
tests/test_norm_ref_cpu.py::test_k_measured holds under K/2 (its pairwise sums sit far
below the serial chains S budgets), so the same bound with the same K applies."""
import pytest
import torch

import norm_ref as R
from norm_ref import BF16, F32

from apex_example_amd import _native

pytestmark = pytest.mark.skipif(not _native.available(), reason="native extension not built")

OPS = ["ln-affine", "ln-noaffine", "rms-affine", "rms-noaffine"]


def _name(dt):
    return {F32: "fp32", BF16: "bf16"}[dt]


def _within(got, ref, what, shape=None):
    assert got is not None, what
    if shape is not None:
        ref = R._shaped(ref, shape)
    R.assert_within(got.detach(), ref, what, R.K)


def _module(rms, affine, nshape, eps, gamma, beta, dt):
    from apex_example_amd.normalization import FusedLayerNorm, FusedRMSNorm

    m = (FusedRMSNorm if rms else FusedLayerNorm)(nshape, eps=eps, elementwise_affine=affine)
    if affine:
        m = m.to(dt)
        with torch.no_grad():
            m.weight.copy_(gamma.reshape(nshape))
            if not rms:
                m.bias.copy_(beta.reshape(nshape))
    return m


def _run(shape, nshape, dt, rms, affine, eps=1e-5):
    n2 = 1
    for s in nshape:
        n2 *= s
    n1 = 1
    for s in shape:
        n1 *= s
    n1 //= n2
    x, dy, gamma, beta = R.make_inputs(n1, n2, dt, shape=shape)
    m = _module(rms, affine, nshape, eps, gamma, beta, dt)
    xa = x.clone().requires_grad_(True)
    y = m(xa)
    y.backward(dy)
    tag = "cpu %s%s %s %s over %s" % ("rms" if rms else "ln", "" if affine else "-noaffine",
                                      _name(dt), tuple(shape), tuple(nshape))
    g_ref, b_ref = (gamma, None if rms else beta) if affine else (None, None)
    fw = R.ref_forward(x, g_ref, b_ref, n2, eps, rms)
    bw = R.ref_backward(dy, x, g_ref, n2, eps, rms)
    assert y.dtype == dt and y.shape == x.shape and xa.grad.dtype == dt
    _within(y, fw["y"], tag + " y")
    _within(xa.grad, bw["dx"], tag + " dx")
    if affine:
        assert m.weight.grad.dtype == dt and m.weight.grad.shape == tuple(nshape)
        _within(m.weight.grad, bw["dgamma"], tag + " dgamma", nshape)
        if not rms:
            assert m.bias.grad.shape == tuple(nshape)
            _within(m.bias.grad, bw["dbeta"], tag + " dbeta", nshape)
        if n1 == 0:     # what torch returns for an empty batch
            assert bool((m.weight.grad == 0).all())
    # the saved statistics, through the operator
    C = _native.require().layer_norm
    w = m.weight.detach() if affine else (torch.ones(n2, dtype=dt) if rms else None)
    b = m.bias.detach() if affine and not rms else None
    y2, mean, invvar = C.forward(x, n2, w, b, eps, rms)
    assert torch.equal(y2, y.detach())
    assert mean.dtype == F32 and mean.shape == (n1,) and invvar.shape == (n1,)
    _within(mean, fw["mean"], tag + " mean")
    _within(invvar, fw["invvar"], tag + " invvar")
    if rms:
        assert bool((mean == 0).all())


@pytest.mark.parametrize("shape", [(5, 64), (33, 777), (0, 64)], ids=str)
@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("op", OPS)
def test_cpu_branch(op, dt, shape):
    _run(shape, shape[-1:], dt, op.startswith("rms"), op.endswith("-affine"))


@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("op", ["ln-affine", "rms-affine"])
def test_cpu_branch_multi_dim_normalized_shape(op, dt):
    """normalized_shape (4, 8): autograd rejects a weight gradient of shape [32]."""
    _run((3, 5, 4, 8), (4, 8), dt, op.startswith("rms"), True)


@pytest.mark.parametrize("eps", [1e-12, 0.1])
def test_cpu_branch_eps(eps):
    _run((33, 777), (777,), F32, False, True, eps=eps)
    _run((5, 64), (64,), BF16, True, True, eps=eps)
