"""The fused softmax cross entropy kernels (csrc/hip/xentropy.hip) against the float64
references of tests/xent_ref.py.  Few rows; what matters is the width V and the alignment:
every width is run at every base offset 0 .. E-1 elements (E = 16 / sizeof(T)) into a flat
buffer, so that the forward's scalar head takes every length, ``head > V`` included, and
the backward - called directly on the view; its dx comes from empty_like and is aligned -
takes both values of ``vec_ok`` (asserted from the pointers): offset 0 is the vector
backward, with a non-zero head in every row whose start V*sizeof(T) puts off 16 bytes, any
other offset the scalar backward.

Instantiations: xent_fwd_k<T, TO> for T in fp32 / fp16 / bf16 with TO = fp32
(half_to_float) and TO = T; xent_bwd_k<T, TG> with TG = fp32 and TG = T.  Every
(smoothing, padding_idx, loss type, grad type) combination of the issue's lists is walked
round-robin over the (offset, row maker) cases of each width.

loss, lse and dx are held to optim_ref.bound with the error magnitudes of xent_ref's
docstring; ignored rows give exactly 0 and an all-zero dx row; rows with -inf logits give
no NaN / inf in lse and dx, nor in the loss without smoothing.

Worst |err| / bound measured on an MI355X (printed at the end of a run with -s): fp32
outputs lse 0.04, loss 0.03, dx 0.11 (float32 emulation on the CPU: 0.16, 0.14, 0.45);
16-bit losses 0.90 and 16-bit dx 0.99 .. 1.00 are the final rounding to the storage type."""
import itertools
import math

import pytest
import torch

import xent_ref as R
from xent_ref import BF16, F16, F32, F64

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}
DTYPES = [F32, F16, BF16]
COMBOS = list(itertools.product([0.0, 0.1, 1.0], [-1, 0, 3], [True, False], [True, False]))


def X():
    from apex_example_amd import _native

    return _native.require().xentropy


def _name(v):
    return {F32: "fp32", F16: "fp16", BF16: "bf16"}.get(v, str(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst |err| / bound per kernel output over the run:")
    for k in sorted(WORST):
        print("  WORST %-44s %.3f" % (k, WORST[k]))


def _within(got, ref, name, tag, rows=None):
    g = got.detach().cpu()
    if rows is not None:
        g, ref = g[rows], R.Val(ref.v[rows], ref.e[rows])
    r = R.worst_ratio(g, ref)
    WORST[name] = max(WORST.get(name, 0.0), r)
    assert r <= 1.0, "%s %s: |err| / bound = %g" % (tag, name, r)


def _heads(N, V, dtype, off):
    es = torch.finfo(dtype).bits // 8
    return [R.row_split((off + r * V) * es, V, es) for r in range(N)]


def _makers(N, V, dtype, heads):
    out = {"randn": R.randn_rows(N, V, dtype, 1)}
    for r in (0, N - 1):
        for pos in R.max_positions(V, *heads[r]):
            out["max_at%d" % pos] = R.max_at(N, V, pos, dtype, pos)
    out["neg_inf"] = R.neg_inf_vectors(R.randn_rows(N, V, dtype, 2), heads)
    out["offset+"] = R.offset(N, V, dtype, 1.0)
    out["offset-"] = R.offset(N, V, dtype, -1.0)
    out["flat"] = R.flat(N, V, dtype)
    return out


def _run(x, off, name, smoothing, padding_idx, h2f, g32, heads, tag):
    N, V = x.shape
    dtype = x.dtype
    xg = R.carve(x, off, DEV)
    es = x.element_size()
    assert xg.data_ptr() % 16 == (off * es) % 16 and R.row_heads(xg) == heads, tag
    neg = name == "neg_inf"
    lab = R.finite_labels(x) if neg else R.labels_for(N, V, padding_idx, 4)
    ign = R.ignored(lab, padding_idx, V)
    labg = lab.to(DEV)
    loss, lse = X().forward(xg, labg, smoothing, padding_idx, h2f)
    assert loss.dtype == (F32 if h2f else dtype) and lse.dtype == F32
    rl, rs = R.ref_xent_fwd(x, lab, smoothing, padding_idx)
    fk = "xent_fwd_k<%s,%s>" % (_name(dtype), _name(loss.dtype))
    _within(lse, rs, fk + " lse", tag)
    finite = torch.isfinite(rl.v)
    if neg and smoothing != 0.0:
        # the mean of a row with -inf logits is -inf: the loss is +inf there, by the maths
        assert bool((loss.cpu()[~finite & ~ign] == float("inf")).all()), tag
    else:
        assert bool(finite.all())
    _within(loss, rl, fk + " loss", tag, rows=finite)
    assert bool((loss.cpu()[ign] == 0).all()), tag + ": ignored rows"
    if neg:
        assert bool(torch.isfinite(lse).all()), tag + ": lse of a row with -inf logits"
    if name == "flat":
        assert float((rs.v - (float(x[0, 0]) + math.log(V))).abs().max()) < 1e-12

    g = torch.rand(N, generator=torch.Generator().manual_seed(9)).add(0.25)
    g = g.to(F32 if g32 else dtype)
    dx = X().backward(g.to(DEV), xg, lse, labg, smoothing, padding_idx)
    assert (xg.data_ptr() % 16 == dx.data_ptr() % 16) == (off == 0), tag + ": vec_ok"
    assert dx.dtype == dtype and dx.shape == x.shape
    ref = R.ref_xent_bwd(g, x, lse.cpu(), lab, smoothing, padding_idx)["dx"]
    bk = "xent_bwd_k<%s,%s>%s" % (_name(dtype), _name(g.dtype), " vector" if off == 0 else " scalar")
    _within(dx, ref, bk + " dx", tag)
    dxc = dx.cpu()
    assert bool((dxc[ign] == 0).all()), tag + ": dx of ignored rows"
    assert bool(torch.isfinite(dxc).all()), tag
    # softmax sums to 1, smoothing to eps, the one-hot to 1 - eps: a row sums to g * 0
    slack = R.bound(ref, dtype).sum(1)
    assert bool(((dxc.to(F64).sum(1) - ref.v.sum(1)).abs() <= slack).all()), tag + ": row sums"
    # ... up to the stored lse's own error: sum_j p_j = exp(lse - lse_stored)
    gmag = torch.where(ign, torch.zeros(N, dtype=F64), g.to(F64).abs())
    zero = slack + 1.01 * gmag * R.bound(rs, F32)
    assert bool((dxc.to(F64).sum(1).abs() <= zero).all()), tag + ": rows do not sum to 0"


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("V", R.WIDTHS + [R.BIG_V])
def test_xentropy(V, dtype):
    N = 4 if V == R.BIG_V else 6
    E = 16 // (torch.finfo(dtype).bits // 8)
    combos = itertools.cycle(COMBOS[(V + E) % len(COMBOS):] + COMBOS[:(V + E) % len(COMBOS)])
    for off in range(E):
        heads = _heads(N, V, dtype, off)
        for name, x in _makers(N, V, dtype, heads).items():
            smoothing, padding_idx, h2f, g32 = next(combos)
            tag = "V=%d %s off=%d %s eps=%g pad=%d h2f=%d g32=%d" % (
                V, _name(dtype), off, name, smoothing, padding_idx, h2f, g32)
            _run(x, off, name, smoothing, padding_idx, h2f, g32, heads, tag)
            if name == "neg_inf" and smoothing != 0.0:
                _run(x, off, name, 0.0, padding_idx, h2f, g32, heads, tag + " eps=0")


def test_every_combination_is_walked():
    """Each (smoothing, padding_idx, loss type, grad type) of COMBOS is used by some case
    of every type (no GPU work: the round-robin above, replayed)."""
    for dtype in DTYPES:
        E = 16 // (torch.finfo(dtype).bits // 8)
        seen = set()
        for V in R.WIDTHS + [R.BIG_V]:
            N = 4 if V == R.BIG_V else 6
            start = (V + E) % len(COMBOS)
            n = sum(len(_makers(N, min(V, 4099), dtype, _heads(N, min(V, 4099), dtype, off)))
                    for off in range(E))
            seen |= {COMBOS[(start + i) % len(COMBOS)] for i in range(n)}
        assert seen == set(COMBOS)


def test_head_longer_than_row_and_every_head():
    """The widths and offsets above give every head length 0 .. E-1, a head longer than the
    row (clamped to V), rows with and without a body, and - at offset 0 - rows of the
    vector backward with a non-zero head."""
    for dtype in DTYPES:
        es = torch.finfo(dtype).bits // 8
        E = 16 // es
        heads = {h for V in R.WIDTHS for off in range(E) for h, _ in _heads(6, V, dtype, off)}
        assert set(range(E)) <= heads
        assert any(E - off > V for V in R.WIDTHS for off in range(1, E))
        assert any(h > 0 for V in R.WIDTHS for h, _ in _heads(6, V, dtype, 0))
