"""The float64 BatchNorm references of tests/bn_ref.py are right (no GPU needed): they agree
with torch's batch_norm in float64 under double autograd to 1e-12, the SyncBN merge agrees
with the statistics of the concatenated batch, the constant K of the tolerance holds the
float32 emulation of every reference under half the bound on exactly the cases the kernels
are held to, every listed shape reaches the condition named beside it (by the geometry
mirror, so a change of tuning defaults fails here instead of silently shrinking coverage),
no ReLU case has an ambiguous element, and an unshifted one-pass variance misses the bound.
Where the extension is built, its CPU branches (``!x.is_cuda()`` in
csrc/torch/norm_ops.cpp) are held to the same references with the same bound."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R
from bn_ref import BF16, F16, F32, F64


def _close(got, want, what):
    atol = 1e-12 * float(want.abs().max()) if want.numel() else 0.0
    torch.testing.assert_close(got, want, rtol=1e-12, atol=atol, msg=lambda m: what + ": " + m)


def _name(v):
    return {F32: "fp32", F16: "fp16", BF16: "bf16"}.get(v, str(v))


def _case_id(c):
    return "%s-%s%s%s" % ("x".join(map(str, c.shape)), c.layout, "-off" if c.offset else "",
                          "-tuned" if c.tune else "")


# ------------------------------------------------------------ reference vs torch float64
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("mode", list(R.MODES))
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("shape,layout", [((6, 20, 5, 3), "nhwc"), ((6, 20, 5, 3), "nchw"),
                                          ((33, 8), "nhwc"), ((4, 5, 10), "nchw"),
                                          ((2, 3, 2, 3, 4), "nchw")])
def test_ref_matches_torch(shape, layout, affine, mode, dtype):
    relu, residual, _ = R.MODES[mode]
    inp = R.make_inputs(shape, dtype, F32, layout, relu=relu, residual=residual, affine=affine)
    chain = R.red_chain(shape, layout == "nhwc" and len(shape) == 4)
    xd = inp["x"].to(F64).requires_grad_(True)
    zd = inp["z"].to(F64).requires_grad_(True) if residual else None
    wd = inp["weight"].to(F64).requires_grad_(True) if affine else None
    bd = inp["bias"].to(F64).requires_grad_(True) if affine else None
    rm, rv = inp["running_mean"].to(F64), inp["running_var"].to(F64)
    eps, mom = R.f32(R.EPS), R.f32(R.MOMENTUM)
    yd = F.batch_norm(xd, rm, rv, wd, bd, True, mom, eps)
    if residual:
        yd = yd + zd
    if relu:
        yd = torch.relu(yd)
    yd.backward(inp["dy"].to(F64))
    out, mask = R.ref_all(inp["x"], inp["dy"], inp["z"], inp["weight"], inp["bias"],
                          inp["running_mean"], inp["running_var"], chain=chain, relu=relu)
    dims = [0] + list(range(2, len(shape)))
    x64 = inp["x"].to(F64)
    _close(out["y"].v, yd.detach(), "y")
    _close(out["mean"].v, x64.mean(dims), "mean")
    _close(out["var"].v, x64.var(dims, unbiased=False), "var")
    _close(out["invstd"].v, (x64.var(dims, unbiased=False) + eps).rsqrt(), "invstd")
    _close(out["running_mean"].v, rm, "running_mean")     # torch updated rm / rv in place
    _close(out["running_var"].v, rv, "running_var")
    _close(out["dx"].v, xd.grad, "dx")
    assert out["dx"].v.shape == inp["x"].shape and out["y"].v.shape == inp["x"].shape
    if relu:
        assert torch.equal(mask, yd.detach() > 0)
    if residual:
        _close(out["dz"].v, zd.grad, "dz")
    if affine:
        _close(out["dgamma"].v, wd.grad, "dgamma")
        _close(out["dbeta"].v, bd.grad, "dbeta")
    # a second momentum step, from the first one's stored running statistics
    rm1, rv1 = out["running_mean"].v.to(F32), out["running_var"].v.to(F32)
    st2 = R.ref_stats(inp["dy"], R.EPS, chain, R.MOMENTUM, rm1, rv1)
    rm2, rv2 = rm1.to(F64), rv1.to(F64)
    F.batch_norm(inp["dy"].to(F64), rm2, rv2, None, None, True, mom, eps)
    _close(st2["running_mean"].v, rm2, "running_mean step 2")
    _close(st2["running_var"].v, rv2, "running_var step 2")


def test_ref_stats_single_element_running_var():
    """count 1: the unbiased factor is 1, not n/(n-1)."""
    x = torch.tensor([[1.5, -2.0, 0.25]])
    rm, rv = torch.zeros(3), torch.ones(3)
    st = R.ref_stats(x, R.EPS, R.red_chain(x.shape, False), 0.5, rm, rv)
    _close(st["var"].v, torch.zeros(3, dtype=F64), "var")
    _close(st["running_var"].v, torch.full((3,), 0.5, dtype=F64), "running_var")
    _close(st["running_mean"].v, x[0].to(F64) * 0.5, "running_mean")


def test_ref_backward_forms():
    """The sum_scale form (sums pre-divided, dx unchanged) and the accumulate form."""
    shape = (6, 20, 5, 3)
    inp = R.make_inputs(shape, F32, F32, "nchw")
    chain = R.red_chain(shape, False)
    st = R.ref_stats(inp["x"], R.EPS, chain)
    n = inp["x"].numel() // shape[1]
    sc = torch.tensor(1.0 / n, dtype=F32)
    gw0, gb0 = torch.randn(20), torch.randn(20)
    a = R.ref_backward(inp["dy"], inp["x"], None, st["mean"], st["invstd"], inp["weight"], chain)
    b = R.ref_backward(inp["dy"], inp["x"], None, st["mean"], st["invstd"], inp["weight"], chain,
                       sum_scale=sc, gw0=gw0, gb0=gb0)
    s = float(sc)
    _close(b["sum_dy"].v, a["sum_dy"].v * s, "sum_dy")
    _close(b["sum_dy_xmu"].v, a["sum_dy_xmu"].v * s, "sum_dy_xmu")
    # (1/n reaches the second form rounded to fp32: 6e-8 of each mean term)
    torch.testing.assert_close(b["dx"].v, a["dx"].v, rtol=0,
                               atol=1e-6 * float(a["dx"].v.abs().max()))
    _close(b["dgamma"].v, a["dgamma"].v + gw0.to(F64), "dgamma")
    _close(b["dbeta"].v, a["dbeta"].v + gb0.to(F64), "dbeta")


@pytest.mark.parametrize("counts", R.COMBINE_WORLDS, ids=str)
def test_ref_combine_matches_concatenated_batch(counts):
    C = 20
    xs, means, vars_, cnt = R.combine_inputs(counts, C)
    # from the float64 per-rank statistics, so that the merge itself is what is compared
    m64 = torch.stack([x.double().mean(0) for x in xs])
    v64 = torch.stack([x.double().var(0, unbiased=False) for x in xs])
    rm, rv = torch.randn(C, dtype=F64), torch.rand(C, dtype=F64)
    out = R.ref_combine(m64, v64, cnt.double(), R.EPS, R.MOMENTUM, rm, rv)
    allx = torch.cat(xs).double()
    N = allx.shape[0]
    eps, mom = R.f32(R.EPS), R.f32(R.MOMENTUM)
    _close(out["mean"].v, allx.mean(0), "mean")
    _close(out["var"].v, allx.var(0, unbiased=False), "var")
    _close(out["invstd"].v, (allx.var(0, unbiased=False) + eps).rsqrt(), "invstd")
    _close(out["inv_total"].v, torch.tensor([1.0 / N], dtype=F64), "inv_total")
    unb = allx.var(0, unbiased=True) if N > 1 else allx.var(0, unbiased=False)
    _close(out["running_mean"].v, (1 - mom) * rm + mom * allx.mean(0), "running_mean")
    _close(out["running_var"].v, (1 - mom) * rv + mom * unb, "running_var")


@pytest.mark.parametrize("S", [1, 65, 300])
def test_ref_slab_matches_plain_sums(S):
    C = 8
    slab, count, shift = R.slab_inputs(S, C)
    st = R.ref_slab_stats(slab, count, shift, R.EPS)
    s = slab.double().sum(2)
    m = s[0] / count
    _close(st["mean"].v, shift.double() + m, "mean")
    _close(st["var"].v, s[1] / count - m * m, "var")
    g, iv = R.grad_slab_inputs(S, C)
    r = R.ref_slab_reduce(g, iv)
    _close(r["sum_dy"].v, g[0].double().sum(1), "sum_dy")
    _close(r["dgamma"].v, g[1].double().sum(1) * iv.double(), "dgamma")


def test_mask_bytes_layout():
    mask = torch.zeros(2, 16, 1, 1, dtype=torch.bool)
    mask[1, 9] = True          # row 1, channel 9 -> byte [1][1], bit 1
    mask[0, 7] = True          # row 0, channel 7 -> byte [0][0], bit 7
    mb = R.mask_bytes(mask)
    assert mb.tolist() == [[128, 0], [0, 2]]


# ------------------------------------------------------------ K, measured on the reference
def _mode_of(i, c):
    names = list(R.MODES)
    return names[i % len(names)]


def _merge(total, part, prefix=""):
    for k, v in part.items():
        total[prefix + k] = max(total.get(prefix + k, 0.0), v)


def test_k_measured(capsys):
    """Worst |ref in float32 - ref in float64| / (eps32 * S) of every output over every
    case of tests/test_batch_norm_gpu.py and every storage type: at most K / 2."""
    worst = {}
    for i, c in enumerate(R.all_cases()):
        relu, residual, _ = R.MODES[_mode_of(i, c)]
        chain = R.red_chain(c.shape, c.layout == "nhwc" and len(c.shape) == 4,
                            c.tune or R.DEFAULT_TUNING)
        for dt, wdt in ((F32, F32), (F16, F16), (BF16, F32)):
            inp = R.make_inputs(c.shape, dt, wdt, c.layout, relu=relu, residual=residual,
                                tune=c.tune)
            _, mask = R.ref_all(inp["x"], inp["dy"], inp["z"], inp["weight"], inp["bias"],
                                inp["running_mean"], inp["running_var"], chain=chain, relu=relu)

            def fn(*t, work):
                return R.ref_all(*t, chain=chain, relu=relu, mask=mask, work=work)[0]

            _merge(worst, R.emulation_ratio(fn, inp["x"], inp["dy"], inp["z"], inp["weight"],
                                            inp["bias"], inp["running_mean"],
                                            inp["running_var"]))
    for kind, dt, c in R.KIND_CASES:
        relu, residual = kind == "allneg", kind == "allneg"
        chain = R.red_chain(c.shape, c.layout == "nhwc" and len(c.shape) == 4)
        inp = R.make_inputs(c.shape, dt, F32, c.layout, kind=kind, relu=relu, residual=residual)
        _, mask = R.ref_all(inp["x"], inp["dy"], inp["z"], inp["weight"], inp["bias"],
                            inp["running_mean"], inp["running_var"], chain=chain, relu=relu)

        def fn(*t, work):
            return R.ref_all(*t, chain=chain, relu=relu, mask=mask, work=work)[0]

        _merge(worst, R.emulation_ratio(fn, inp["x"], inp["dy"], inp["z"], inp["weight"],
                                        inp["bias"], inp["running_mean"], inp["running_var"]))
    for counts in R.COMBINE_WORLDS:
        _, means, vars_, cnt = R.combine_inputs(counts, 520)
        rm, rv = torch.randn(520), torch.rand(520)
        _merge(worst, R.emulation_ratio(R.ref_combine, means, vars_, cnt, R.EPS, R.MOMENTUM,
                                        rm, rv), "combine.")
    for S in R.SLAB_S:
        for C in R.SLAB_C:
            slab, count, shift = R.slab_inputs(S, C)
            rm, rv = torch.randn(C), torch.rand(C)
            _merge(worst, R.emulation_ratio(R.ref_slab_stats, slab, count, shift, R.EPS,
                                            R.MOMENTUM, rm, rv), "slab.")
            g, iv = R.grad_slab_inputs(S, C)
            _merge(worst, R.emulation_ratio(R.ref_slab_reduce, g, iv,
                                            torch.tensor(1.0 / 3), torch.randn(C),
                                            torch.randn(C)), "slab.")
    with capsys.disabled():
        print("\nbn_ref emulation ratios:",
              "  ".join("%s %.2f" % kv for kv in sorted(worst.items())))
    for name, r in worst.items():
        assert r <= R.K / 2, (name, r)


# ------------------------------------------------------------ the case list reaches its claims
@pytest.mark.parametrize("c", R.all_cases(), ids=_case_id)
def test_case_reaches_named_condition(c):
    for esize in (4, 2):
        info = R.geom(c, esize)
        for name in c.reaches:
            assert R.REACH[name](info), (name, info)


def test_every_condition_is_listed():
    listed = {r for c in R.all_cases() for r in c.reaches}
    assert listed == set(R.REACH), set(R.REACH) ^ listed


def test_geometry_examples():
    """The launch geometry the issue's examples quote, from the mirror."""
    g = R.ngeom(2048, True)
    assert (g.ctile, g.rows_iter, g.cblocks) == (64, 4, 4)
    s = R.reduce_splits(1030, g)
    assert s == 128 and -(-1030 // s) == 9             # the last splits start past M
    g = R.ngeom(24, True)
    assert (g.ctile, g.rows_iter) == (3, 85)
    assert R.ngeom(520, True).cblocks == 2 and R.ngeom(600, False).cblocks == 10
    assert R.nchw_splits(8, 64, 14 * 14) == 1 and R.nchw_splits(5, 8, 576) == 2
    assert [R.slab_ch(S) for S in R.SLAB_S] == [32, 32, 32, 32, 32, 16, 8, 4, 2, 1, 1]
    assert R.elem_grid(2 * 16 * 257 * 257) == 8192


# ------------------------------------------------------------ ambiguity, one-pass emulation
@pytest.mark.parametrize("c", R.NHWC_CASES[::5] + R.NCHW_CASES[::3] + [R.NCHW_BIG],
                         ids=_case_id)
@pytest.mark.parametrize("mode", ["relu", "relu_z"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
def test_no_ambiguous_relu_element(c, mode, dtype):
    relu, residual, _ = R.MODES[mode]
    inp = R.make_inputs(c.shape, dtype, F32, c.layout, relu=relu, residual=residual)
    chain = R.red_chain(c.shape, c.layout == "nhwc" and len(c.shape) == 4)
    st = R.ref_stats(inp["x"], R.EPS, chain)
    fw = R.ref_apply(inp["x"], st["mean"], st["invstd"], inp["weight"], inp["bias"], inp["z"],
                     True)
    assert int(R.ambiguous(fw["o"], dtype).sum()) == 0
    assert inp["x"].dtype == dtype and (inp["z"] is None or inp["z"].dtype == dtype)


def test_ambiguous_elements_are_found_and_moved():
    """The generator's check is not vacuous: an o planted at exactly 0 is ambiguous."""
    inp = R.make_inputs((6, 20, 5, 3), F32, F32, "nchw", residual=True)
    chain = R.red_chain((6, 20, 5, 3), False)
    st = R.ref_stats(inp["x"], R.EPS, chain)
    fw = R.ref_apply(inp["x"], st["mean"], st["invstd"], inp["weight"], inp["bias"], None, True)
    inp["z"] = (-fw["o"].v).to(F32)
    fw = R.ref_apply(inp["x"], st["mean"], st["invstd"], inp["weight"], inp["bias"], inp["z"],
                     True)
    assert int(R.ambiguous(fw["o"], F32).sum()) > 1000
    R._deambiguate(inp, F32, chain)
    fw = R.ref_apply(inp["x"], st["mean"], st["invstd"], inp["weight"], inp["bias"], inp["z"],
                     True)
    assert int(R.ambiguous(fw["o"], F32).sum()) == 0


def test_one_pass_fails():
    """An unshifted one-pass E[x^2] - mean^2 in float32 lands outside the bound on the
    large-mean input (mean / sigma = 1e5), the shifted sums in float32 inside it."""
    shape = (350, 24, 2, 1)
    inp = R.make_inputs(shape, F32, F32, "nhwc", kind="large_mean")
    chain = R.red_chain(shape, True)
    st = R.ref_stats(inp["x"], R.EPS, chain)
    assert float((st["mean"].v.abs() / st["var"].v.sqrt()).min()) > 5e4
    mean, var, invstd = R.one_pass_stats(inp["x"], R.EPS)
    assert R.worst_ratio(var, st["var"]) > 100
    assert R.worst_ratio(invstd, st["invstd"]) > 100
    st32 = R.ref_stats(inp["x"], R.EPS, chain, work=F32)
    assert R.worst_ratio(st32["var"].v, st["var"]) <= 0.5
    assert R.worst_ratio(st32["invstd"].v, st["invstd"]) <= 0.5


def test_outlier_first_budget_is_what_the_docstring_says():
    """With the shift D = 100 sigma off, the variance budget is ~ K*eps32*3*chain*D^2."""
    shape = (350, 24, 2, 1)
    inp = R.make_inputs(shape, F32, F32, "nhwc", kind="outlier_first")
    chain = R.red_chain(shape, True)
    st = R.ref_stats(inp["x"], R.EPS, chain)
    rel = R.bound(st["var"], F32) / st["var"].v
    want = R.K * R.EPS32 * 3 * chain * 200.0 ** 2 / float(st["var"].v.mean())
    assert 0.5 * want < float(rel.max()) < 2 * want, (float(rel.max()), want)
    assert 0.05 < float(rel.max()) < 0.15
    mb = float(R.bound(st["mean"], F32).max())            # ~ K*eps32*chain*D: 0.5 % of sigma
    assert 0.5 * R.K * R.EPS32 * chain * 200 < mb < 2 * R.K * R.EPS32 * chain * 200 < 0.02
    ok = R.make_inputs(shape, F32, F32, "nhwc")
    rel_ok = R.bound(R.ref_stats(ok["x"], R.EPS, chain)["var"], F32)
    assert float((rel_ok / R.ref_stats(ok["x"], R.EPS, chain)["var"].v).max()) < 1e-3


# ------------------------------------------------------------ the extension's CPU branches
def _bn():
    from apex_example_amd import _native

    if not _native.available():
        pytest.skip("native extension not built")
    return _native.require().bn


def _within(got, ref, what):
    R.assert_within(got.detach(), ref, what, R.K)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_name)
@pytest.mark.parametrize("mode", ["none", "relu", "relu_z"])
@pytest.mark.parametrize("shape,layout", [((6, 20, 5, 3), "nchw"), ((33, 8), "nhwc"),
                                          ((4, 5, 10), "nchw")])
def test_extension_cpu_branches(shape, layout, mode, dtype):
    """local_stats, combine_stats, apply, reduce_grad and backward_elemt on CPU tensors: the
    float32 ATen emulation of the formulas, held to the kernels' bound."""
    C = _bn()
    relu, residual, _ = R.MODES[mode]
    inp = R.make_inputs(shape, dtype, F32, layout, relu=relu, residual=residual)
    chain = R.red_chain(shape, False)
    x, dy, z, w, b = (inp[k] for k in ("x", "dy", "z", "weight", "bias"))
    ref, mask = R.ref_all(x, dy, z, w, b, inp["running_mean"], inp["running_var"], chain=chain,
                          relu=relu)
    mean, var = C.local_stats(x)
    _within(mean, ref["mean"], "cpu mean")
    _within(var, ref["var"], "cpu var")
    n = x.numel() // x.shape[1]
    rm, rv = inp["running_mean"].clone(), inp["running_var"].clone()
    # the merge of one rank, from the stored fp32 statistics (exact inputs to ref_combine)
    cref = R.ref_combine(mean, var, torch.tensor([float(n)]), R.EPS, R.MOMENTUM,
                         inp["running_mean"], inp["running_var"])
    mean_g, invstd, var_b = C.combine_stats(mean.view(1, -1), var.view(1, -1),
                                            torch.tensor([float(n)]), R.EPS, R.MOMENTUM, rm, rv)
    for got, name in ((mean_g, "mean"), (invstd, "invstd"), (var_b, "var"),
                      (rm, "running_mean"), (rv, "running_var")):
        _within(got, cref[name], "cpu combine " + name)
    _within(invstd, ref["invstd"], "cpu invstd")
    y = C.apply(x, mean_g, invstd, w, b, z, relu)
    assert y.dtype == dtype
    _within(y, ref["y"], "cpu y")
    if relu:
        assert torch.equal(y > 0, mask)
    sdy, sdx, gw, gb = C.reduce_grad(dy, x, mean_g, invstd, w, b, z, relu, True)
    _within(sdy, ref["sum_dy"], "cpu sum_dy")
    _within(sdx, ref["sum_dy_xmu"], "cpu sum_dy_xmu")
    _within(gw, ref["dgamma"], "cpu dgamma")
    _within(gb, ref["dbeta"], "cpu dbeta")
    dx, dz = C.backward_elemt(dy, x, mean_g, invstd, w, b, sdy, sdx, float(n), z, relu, residual)
    _within(dx, ref["dx"], "cpu dx")
    if residual:
        _within(dz, ref["dz"], "cpu dz")
    else:
        assert dz is None


@pytest.mark.parametrize("counts", R.COMBINE_WORLDS, ids=str)
def test_extension_cpu_combine(counts):
    C = _bn()
    _, means, vars_, cnt = R.combine_inputs(counts, 20)
    rm0, rv0 = torch.randn(20), torch.rand(20) + 0.5
    ref = R.ref_combine(means, vars_, cnt, R.EPS, R.MOMENTUM, rm0, rv0)
    rm, rv = rm0.clone(), rv0.clone()
    mean, invstd, var = C.combine_stats(means, vars_, cnt, R.EPS, R.MOMENTUM, rm, rv)
    for got, name in ((mean, "mean"), (invstd, "invstd"), (var, "var"), (rm, "running_mean"),
                      (rv, "running_var")):
        _within(got, ref[name], "cpu combine %s %s" % (counts, name))
