#!/usr/bin/env python3
"""Kernel microbenchmarks on one MI355X (interleaved A/B in one process).

    python tools/microbench.py bn      # fused BN kernels vs HBM copy roofline vs MIOpen BN
    python tools/microbench.py conv1x1 # ResNet-50 1x1 convs: MIOpen conv vs GEMM (hipBLASLt)
    python tools/microbench.py optim   # optimizer step bandwidth (ResNet-50 sizes)
    python tools/microbench.py ln      # FusedLayerNorm fwd/bwd vs torch LayerNorm
    python tools/microbench.py lamb    # FusedLAMB / FusedAdam on BERT-large's 336M params
    python tools/microbench.py attn-packed  # packed (cu_seqlens) vs padded + key mask attention
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


BN_SHAPES = [  # (N, C, H, W) ResNet-50 @ bs256 NHWC
    (256, 64, 112, 112), (256, 64, 56, 56), (256, 256, 56, 56), (256, 128, 28, 28),
    (256, 512, 28, 28), (256, 256, 14, 14), (256, 1024, 14, 14), (256, 2048, 7, 7),
    (256, 512, 7, 7),
]


def bench_bn(args):
    from apex_example_amd import _native

    C_ = _native.require().bn
    dev = "cuda"
    print("| shape (NHWC bf16) | MB/tensor | copy TB/s | stats | apply+relu | apply+z+relu | "
          "reduce+relu+z | bwd+relu+z | MIOpen fwd | MIOpen bwd |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for (n, c, h, w) in BN_SHAPES:
        x = torch.randn(n, c, h, w, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        z = torch.randn_like(x)
        dy = torch.randn_like(x)
        wt = torch.ones(c, device=dev)
        bs = torch.zeros(c, device=dev)
        nb = x.numel() * 2
        mb = nb / 1e6
        t_copy = timeit(lambda: x.clone())
        mean, var = C_.local_stats(x)
        invstd = (var + 1e-5).rsqrt()
        t_stats = timeit(lambda: C_.local_stats(x))
        t_apply = timeit(lambda: C_.apply(x, mean, invstd, wt, bs, None, True))
        t_applyz = timeit(lambda: C_.apply(x, mean, invstd, wt, bs, z, True))
        t_red = timeit(lambda: C_.reduce_grad(dy, x, mean, invstd, wt, bs, z, True, True))
        s1, s2, _, _ = C_.reduce_grad(dy, x, mean, invstd, wt, bs, z, True, True)
        t_bwd = timeit(lambda: C_.backward_elemt(dy, x, mean, invstd, wt, bs, s1, s2,
                                                 float(n * h * w), z, True, True))
        bn = torch.nn.BatchNorm2d(c).to(dev)
        xr = x.detach().requires_grad_(True)
        t_mf = timeit(lambda: F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias,
                                           True, 0.1, 1e-5))
        yb = F.batch_norm(xr, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, 0.1, 1e-5)

        def mb_bwd():
            torch.autograd.grad(yb, xr, dy, retain_graph=True)

        t_mb = timeit(mb_bwd)

        def tbs(nbytes, t):
            return "%.0f us (%.2f TB/s)" % (t, nbytes / (t * 1e-6) / 1e12)

        print("| %s | %.0f | %.2f | %s | %s | %s | %s | %s | %s | %s |" % (
            (n, c, h, w), mb, 2 * nb / (t_copy * 1e-6) / 1e12, tbs(nb, t_stats),
            tbs(2 * nb, t_apply), tbs(3 * nb, t_applyz), tbs(3 * nb, t_red), tbs(5 * nb, t_bwd),
            tbs(2 * nb, t_mf), tbs(3 * nb, t_mb)))


# (N, C, H, W) -> number of BN layers of that shape in ResNet-50 (bs 256)
R50_BN = {(256, 64, 112, 112): 1, (256, 64, 56, 56): 6, (256, 256, 56, 56): 4,
          (256, 128, 56, 56): 1, (256, 128, 28, 28): 7, (256, 512, 28, 28): 5,
          (256, 256, 28, 28): 1, (256, 256, 14, 14): 11, (256, 1024, 14, 14): 7,
          (256, 512, 14, 14): 1, (256, 512, 7, 7): 5, (256, 2048, 7, 7): 4}


def bench_bn_tune(args):
    """Sweep the NHWC BN grid-sizing knobs; report the ResNet-50-weighted total
    (forward stats+finalize+apply, backward reduce+finalize+elementwise) per config."""
    from apex_example_amd import _native

    C_ = _native.require().bn
    dev = "cuda"
    data = {}
    for (n, c, h, w), cnt in R50_BN.items():
        x = torch.randn(n, c, h, w, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        data[(n, c, h, w)] = (x, torch.randn_like(x), torch.randn_like(x), torch.ones(c, device=dev),
                              torch.zeros(c, device=dev), cnt)
    default = C_.get_tuning()

    def run_red():
        tot = 0.0
        per = {}
        for shp, (x, z, dy, wt, bs, cnt) in data.items():
            t1 = timeit(lambda: C_.local_stats(x), iters=10, warmup=3)
            mean, var = C_.local_stats(x)
            invstd = (var + 1e-5).rsqrt()
            t2 = timeit(lambda: C_.reduce_grad(dy, x, mean, invstd, wt, bs, z, True, True),
                        iters=10, warmup=3)
            per[shp] = (t1, t2)
            tot += cnt * (t1 + t2)
        return tot, per

    def run_elem():
        tot = 0.0
        per = {}
        for shp, (x, z, dy, wt, bs, cnt) in data.items():
            mean, var = C_.local_stats(x)
            invstd = (var + 1e-5).rsqrt()
            s1, s2, _, _ = C_.reduce_grad(dy, x, mean, invstd, wt, bs, z, True, True)
            t1 = timeit(lambda: C_.apply(x, mean, invstd, wt, bs, z, True), iters=10, warmup=3)
            t2 = timeit(lambda: C_.backward_elemt(dy, x, mean, invstd, wt, bs, s1, s2,
                                                  float(x.numel() // x.size(1)), z, True, True),
                        iters=10, warmup=3)
            per[shp] = (t1, t2)
            tot += cnt * (t1 + t2)
        return tot, per

    print("default", default)
    res = []
    for rpt in (8, 16, 32, 64):
        for cap in (1024, 2048, 4096):
            for mn in (0, 512, 1024):
                C_.set_tuning(red_rpt=rpt, red_cap=cap, red_min=mn)
                tot, per = run_red()
                res.append((tot, rpt, cap, mn, per))
                print("reduce rpt=%d cap=%d min=%d: %.0f us (R50-weighted)" % (rpt, cap, mn, tot),
                      flush=True)
    res.sort(key=lambda r: r[0])
    print("BEST reduce:", res[0][1:4], "%.0f us" % res[0][0])
    for shp, (a, b) in res[0][4].items():
        print("   ", shp, "stats %.1f us, reduce %.1f us" % (a, b))
    C_.set_tuning(red_rpt=default[0], red_cap=default[1], red_min=default[2])
    res = []
    for rpt in (2, 4, 8, 16, 32):
        for cap in (4096, 8192, 16384):
            for mn in (0, 1024, 2048):
                C_.set_tuning(elem_rpt=rpt, elem_cap=cap, elem_min=mn)
                tot, per = run_elem()
                res.append((tot, rpt, cap, mn, per))
                print("elem rpt=%d cap=%d min=%d: %.0f us (R50-weighted)" % (rpt, cap, mn, tot),
                      flush=True)
    res.sort(key=lambda r: r[0])
    print("BEST elem:", res[0][1:4], "%.0f us" % res[0][0])
    for shp, (a, b) in res[0][4].items():
        print("   ", shp, "apply %.1f us, backward %.1f us" % (a, b))


def bench_conv1x1(args):
    dev = "cuda"
    torch.backends.cudnn.benchmark = False
    shapes = [(256, 64, 256, 56), (256, 256, 64, 56), (256, 256, 128, 56), (256, 128, 512, 28),
              (256, 512, 128, 28), (256, 512, 256, 28), (256, 256, 1024, 14),
              (256, 1024, 256, 14), (256, 1024, 512, 14), (256, 512, 2048, 7),
              (256, 2048, 512, 7)]
    print("| N,Cin,Cout,HW | GFLOP | MIOpen fwd | GEMM fwd | MIOpen dgrad | GEMM dgrad | "
          "MIOpen wgrad | GEMM wgrad |")
    print("|---|---|---|---|---|---|---|---|")
    for (n, ci, co, hw) in shapes:
        x = torch.randn(n, ci, hw, hw, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        w = torch.randn(co, ci, 1, 1, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        dy = torch.randn(n, co, hw, hw, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        M = n * hw * hw
        gf = 2 * M * ci * co / 1e9
        x2 = x.permute(0, 2, 3, 1).reshape(M, ci)
        dy2 = dy.permute(0, 2, 3, 1).reshape(M, co)
        w2 = w.reshape(co, ci)
        t_cf = timeit(lambda: F.conv2d(x, w))
        t_gf = timeit(lambda: torch.mm(x2, w2.t()))
        t_cd = timeit(lambda: torch.ops.aten.convolution_backward(
            dy, x, w, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1, (True, False, False)))
        t_gd = timeit(lambda: torch.mm(dy2, w2))
        t_cw = timeit(lambda: torch.ops.aten.convolution_backward(
            dy, x, w, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1, (False, True, False)))
        t_gw = timeit(lambda: torch.mm(dy2.t(), x2))

        def tf(t):
            return "%.0f us (%.0f TF)" % (t, gf / (t * 1e-6) / 1e3)

        print("| %d,%d,%d,%d | %.1f | %s | %s | %s | %s | %s | %s |" % (
            n, ci, co, hw, gf, tf(t_cf), tf(t_gf), tf(t_cd), tf(t_gd), tf(t_cw), tf(t_gw)))


def bench_conv1x1_own(args):
    """Stride-1 1x1 conv forward: hipBLASLt GEMM (torch.mm on the NHWC rows) vs the
    own MFMA implicit-GEMM kernel (conv_tap_k kFwd1), with bandwidth - the base a
    fused BN prologue / statistics epilogue would be built on."""
    from apex_example_amd import _native

    cv = _native.require().conv
    dev = "cuda"
    shapes = [(256, 64, 256, 56), (256, 256, 64, 56), (256, 128, 512, 28), (256, 512, 128, 28),
              (256, 256, 1024, 14), (256, 1024, 256, 14), (256, 512, 2048, 7),
              (256, 2048, 512, 7)]
    print("| N,Cin,Cout,HW | MB moved | hipBLASLt | own MFMA | max abs diff |")
    print("|---|---|---|---|---|")
    for (n, ci, co, hw) in shapes:
        x = torch.randn(n, ci, hw, hw, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        w = (torch.randn(co, ci, 1, 1, device=dev) * 0.05).to(torch.bfloat16).to(
            memory_format=torch.channels_last)
        M = n * hw * hw
        x2 = x.permute(0, 2, 3, 1).reshape(M, ci)
        w2 = w.reshape(co, ci)
        mb = (M * ci + M * co) * 2 / 1e6
        t_g = timeit(lambda: torch.mm(x2, w2.t()))
        t_o = timeit(lambda: cv.conv_fwd(x, w, 1))
        y_g = torch.mm(x2, w2.t())
        y_o = cv.conv_fwd(x, w, 1).permute(0, 2, 3, 1).reshape(M, co)
        d = float((y_g.float() - y_o.float()).abs().max())

        def bw(t):
            return "%.0f us (%.2f TB/s)" % (t, mb / 1e6 / (t * 1e-6))

        print("| %d,%d,%d,%d | %.0f | %s | %s | %.3g |" % (n, ci, co, hw, mb, bw(t_g), bw(t_o), d),
              flush=True)
    # weight gradient dW = dY^T X: split-K hipBLASLt (ops/conv.py wgrad_1x1) vs the
    # own per-tap MFMA wgrad kernel with one tap
    from apex_example_amd.ops.conv import wgrad_1x1

    print("\n| N,Cin,Cout,HW | split-K hipBLASLt wgrad | own MFMA wgrad | rel diff |")
    print("|---|---|---|---|")
    for (n, ci, co, hw) in shapes:
        x = torch.randn(n, ci, hw, hw, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        dy = torch.randn(n, co, hw, hw, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        M = n * hw * hw
        x2 = x.permute(0, 2, 3, 1).reshape(M, ci)
        dy2 = dy.permute(0, 2, 3, 1).reshape(M, co)
        t_g = timeit(lambda: wgrad_1x1(dy2, x2, torch.bfloat16))
        t_o = timeit(lambda: cv.conv_wgrad(dy, x, torch.bfloat16, 0, 1, 1))
        a = wgrad_1x1(dy2, x2, torch.float32)
        b = cv.conv_wgrad(dy, x, torch.float32, 0, 1, 1).reshape(co, ci)
        rd = float((a - b).abs().max() / a.abs().max())
        print("| %d,%d,%d,%d | %.0f us | %.0f us | %.2g |" % (n, ci, co, hw, t_g, t_o, rd),
              flush=True)


def bench_wgrad_o1(args):
    """amp O1 weight gradients of GPT-2-medium's dense layers (fp16 operands, T = 8192
    tokens, fp32 weight): one GEMM writing fp32 (mm(out_dtype=fp32), what fused_dense
    runs) vs an fp16 GEMM + cast (Apex O1's dataflow), the fp16 GEMM with PyTorch's
    default heuristic and with TunableOp-tuned selections."""
    dev = "cuda"
    T = 8192
    shapes = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)]  # (out, in)
    data = []
    for (o, i) in shapes:
        dy = torch.randn(T, o, device=dev, dtype=torch.float16)
        x = torch.randn(T, i, device=dev, dtype=torch.float16)
        data.append((o, i, dy, x))
    rows = {}
    for (o, i, dy, x) in data:
        rows[(o, i)] = [timeit(lambda: torch.mm(dy.t(), x, out_dtype=torch.float32)),
                        timeit(lambda: dy.t() @ x),
                        timeit(lambda: (dy.t() @ x).float())]
    t = torch.cuda.tunable
    t.enable(True)
    t.tuning_enable(True)
    t.set_max_tuning_duration(100)
    t.set_max_tuning_iterations(100)
    for (o, i, dy, x) in data:
        for _ in range(2):  # first call tunes
            dy.t() @ x
            torch.mm(dy.t(), x, out_dtype=torch.float32)
        torch.cuda.synchronize()
        rows[(o, i)] += [timeit(lambda: torch.mm(dy.t(), x, out_dtype=torch.float32)),
                         timeit(lambda: dy.t() @ x), timeit(lambda: (dy.t() @ x).float())]
    t.tuning_enable(False)
    t.enable(False)
    print("| dW [out, in], T=8192 | GF | fp32-out mm | fp16 mm | fp16 mm + cast | tuned: fp32-out | "
          "fp16 | fp16 + cast |")
    print("|---|---|---|---|---|---|---|---|")
    for (o, i), r in rows.items():
        gf = 2 * T * o * i / 1e9
        print("| %d x %d | %.1f | %s |" % (o, i, gf, " | ".join(
            "%.0f us (%.0f TF)" % (v, gf / 1e3 / (v * 1e-6)) for v in r)), flush=True)


def bench_wgrad_dense(args):
    """Transformer dense-layer weight gradients dW[out, in] = dY^T X over T tokens (long
    K, small output: 16-48 output tiles of 256 x 256 cannot fill 256 CUs): one GEMM
    (PyTorch heuristic, and the committed TunableOp table) vs split-K over S token
    chunks (fp32 partials from one batched GEMM + the slab reduction kernel)."""
    from apex_example_amd import _native
    from apex_example_amd.utils.gemm_tuning import use_tuned_gemms

    cv = _native.require().conv
    dev = "cuda"
    cases = [("bert", 16384, torch.bfloat16, torch.bfloat16),
             ("gpt2-O1", 8192, torch.float16, torch.float32)]
    shapes = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)]
    Ss = (2, 4, 8, 16)
    print("| model | dW [out, in] | T | GF | mm | mm tuned | " +
          " | ".join("split-K S=%d" % S for S in Ss) + " |")
    print("|---|---|---|---|---|---|" + "---|" * len(Ss))
    for name, T, dt, odt in cases:
        for (o, i) in shapes:
            dy = torch.randn(T, o, device=dev, dtype=dt)
            x = torch.randn(T, i, device=dev, dtype=dt)
            gf = 2 * T * o * i / 1e9

            def one():
                if odt == dt:
                    return dy.t() @ x
                return torch.mm(dy.t(), x, out_dtype=odt)

            def splitk(S):
                a = dy.view(S, T // S, o).transpose(1, 2)
                b = x.view(S, T // S, i)
                return cv.splitk_reduce(torch.bmm(a, b, out_dtype=torch.float32), odt)

            t_mm = timeit(one)
            ref = one().float()
            torch.cuda.tunable.enable(False)
            tuned = use_tuned_gemms("bert_large" if name == "bert" else "gpt2_medium")
            t_tuned = timeit(one) if tuned else float("nan")
            torch.cuda.tunable.enable(False)
            cols = []
            for S in Ss:
                t = timeit(lambda S=S: splitk(S))
                err = float((splitk(S).float() - ref).abs().max() / ref.abs().max())
                cols.append("%.0f us (%.0f TF, err %.1e)" % (t, gf / 1e3 / (t * 1e-6), err))
            print("| %s | %d x %d | %d | %.1f | %.0f us (%.0f TF) | %.0f us | %s |" % (
                name, o, i, T, gf, t_mm, gf / 1e3 / (t_mm * 1e-6), t_tuned, " | ".join(cols)),
                flush=True)


def bench_wgrad(args):
    """1x1-conv weight gradient dW[co,ci] = sum_m dY[m,co] X[m,ci]: MIOpen vs
    split-K hipBLASLt (bmm over S row-chunks with fp32 output, then a sum)."""
    dev = "cuda"
    torch.backends.cudnn.benchmark = False
    shapes = [(256, 64, 256, 56), (256, 256, 64, 56), (256, 256, 128, 56), (256, 128, 512, 28),
              (256, 512, 128, 28), (256, 512, 256, 28), (256, 256, 1024, 14),
              (256, 1024, 256, 14), (256, 1024, 512, 14), (256, 512, 2048, 7),
              (256, 2048, 512, 7)]
    print("| N,Cin,Cout,HW | GFLOP | MIOpen wgrad | " + " | ".join(
        "splitK %d" % s for s in (1, 2, 4, 8, 16, 32, 64, 128, 256)) + " |")
    print("|---|---|---|" + "---|" * 9)
    for (n, ci, co, hw) in shapes:
        x = torch.randn(n, ci, hw, hw, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        w = torch.randn(co, ci, 1, 1, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        dy = torch.randn(n, co, hw, hw, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        M = n * hw * hw
        gf = 2 * M * ci * co / 1e9
        x2 = x.permute(0, 2, 3, 1).reshape(M, ci)
        dy2 = dy.permute(0, 2, 3, 1).reshape(M, co)
        t_cw = timeit(lambda: torch.ops.aten.convolution_backward(
            dy, x, w, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1, (False, True, False)))
        ref = torch.ops.aten.convolution_backward(
            dy, x, w, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1,
            (False, True, False))[1].float().reshape(co, ci)
        cells = []
        for S in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            if M % S:
                cells.append("-")
                continue
            a = dy2.view(S, M // S, co).transpose(1, 2)   # [S, co, m]
            b = x2.view(S, M // S, ci)                     # [S, m, ci]

            def f():
                return torch.bmm(a, b, out_dtype=torch.float32).sum(0).to(torch.bfloat16)

            out = f().float()
            err = float((out - ref).norm() / ref.norm())
            t = timeit(f)
            cells.append("%.0f us (%.0f TF)%s" % (t, gf / (t * 1e-6) / 1e3,
                                                  "" if err < 1e-2 else " ERR %.3f" % err))
        print("| %d,%d,%d,%d | %.1f | %.0f us (%.0f TF) | %s |" % (
            n, ci, co, hw, gf, t_cw, gf / (t_cw * 1e-6) / 1e3, " | ".join(cells)), flush=True)


def bench_conv3x3(args):
    """3x3 stride-1 convs of ResNet-50: MIOpen vs the MFMA implicit-GEMM kernel."""
    from apex_example_amd import _native
    from apex_example_amd.ops.conv import _rot_weight

    cv = _native.require().conv
    dev = "cuda"
    torch.backends.cudnn.benchmark = False
    print("| N,C,K,HW | GFLOP | MIOpen fwd | MFMA fwd | MIOpen dgrad | MFMA dgrad (+rot) | "
          "MIOpen wgrad | MFMA wgrad per-tap | MFMA wgrad 9-tap | max rel err fwd / wgrad |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for (n, c, k, hw) in [(256, 64, 64, 56), (256, 128, 128, 28), (256, 256, 256, 14),
                          (256, 512, 512, 7)]:
        x = torch.randn(n, c, hw, hw, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        w = (torch.randn(k, c, 3, 3, device=dev, dtype=torch.bfloat16) * 0.05).to(
            memory_format=torch.channels_last)
        dy = torch.randn(n, k, hw, hw, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        gf = 2 * n * hw * hw * c * k * 9 / 1e9
        t_mf = timeit(lambda: F.conv2d(x, w, padding=1))
        t_of = timeit(lambda: cv.conv_fwd(x, w))
        t_md = timeit(lambda: torch.ops.aten.convolution_backward(
            dy, x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, (True, False, False)))
        t_od = timeit(lambda: cv.conv_fwd(dy, _rot_weight(w)))
        t_mw = timeit(lambda: torch.ops.aten.convolution_backward(
            dy, x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1, (False, True, False)))
        t_ow = timeit(lambda: cv.conv_wgrad(dy, x, torch.bfloat16, 0))
        t_o9 = timeit(lambda: cv.conv_wgrad(dy, x, torch.bfloat16, 1)) if hw <= 56 else 0.0
        t_v = [timeit(lambda: cv.conv_wgrad(dy, x, torch.bfloat16, a)) for a in (2, 3)]
        ref = F.conv2d(x, w, padding=1).float()
        err = float((cv.conv_fwd(x, w).float() - ref).abs().max() / ref.abs().max())
        wref = torch.ops.aten.convolution_backward(
            dy.float(), x.float(), w.float(), None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
            (False, True, False))[1]
        werr = float((cv.conv_wgrad(dy, x, torch.float32, 0) - wref).abs().max()
                     / wref.abs().max())

        def tf(t):
            return "%.0f us (%.0f TF)" % (t, gf / (t * 1e-6) / 1e3)

        print("| %d,%d,%d,%d | %.1f | %s | %s | %s | %s | %s | %s | %s | %.2e / %.2e |" % (
            n, c, k, hw, gf, tf(t_mf), tf(t_of), tf(t_md), tf(t_od), tf(t_mw), tf(t_ow),
            tf(t_o9) if t_o9 else "-", err, werr), "variants 2/3: %.0f / %.0f us" % tuple(t_v),
            flush=True)


def bench_conv_s2(args):
    """Stride-2 convs of ResNet-50 (3x3 in layer2-4's first block, 1x1 downsample
    projections): MIOpen vs the MFMA kernels, forward / data grad / weight grad."""
    from apex_example_amd import _native
    from apex_example_amd.ops.conv import _rot_weight

    cv = _native.require().conv
    dev = "cuda"
    print("| k,N,C,K,HW(in) | GFLOP | MIOpen fwd | MFMA fwd | MIOpen dgrad | MFMA dgrad | "
          "MIOpen wgrad | MFMA wgrad |")
    print("|---|---|---|---|---|---|---|---|")
    for (k, n, c, co, hw) in [(3, 256, 128, 128, 56), (3, 256, 256, 256, 28), (3, 256, 512, 512, 14),
                              (1, 256, 256, 512, 56), (1, 256, 512, 1024, 28),
                              (1, 256, 1024, 2048, 14)]:
        x = torch.randn(n, c, hw, hw, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        w = (torch.randn(co, c, k, k, device=dev, dtype=torch.bfloat16) * 0.05).to(
            memory_format=torch.channels_last)
        ho = hw // 2
        dy = torch.randn(n, co, ho, ho, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        gf = 2 * n * ho * ho * c * co * k * k / 1e9
        pad = k // 2
        t_mf = timeit(lambda: F.conv2d(x, w, stride=2, padding=pad))
        t_of = timeit(lambda: cv.conv_fwd(x, w, 2))
        t_md = timeit(lambda: torch.ops.aten.convolution_backward(
            dy, x, w, None, (2, 2), (pad, pad), (1, 1), False, (0, 0), 1, (True, False, False)))
        if k == 3:
            t_od = timeit(lambda: cv.conv_dgrad_s2(dy, _rot_weight(w), hw, hw))
        else:
            t_od = timeit(lambda: cv.conv_dgrad_s2(
                dy, w.reshape(co, c).t().contiguous().view(c, co, 1, 1), hw, hw))
        t_mw = timeit(lambda: torch.ops.aten.convolution_backward(
            dy, x, w, None, (2, 2), (pad, pad), (1, 1), False, (0, 0), 1, (False, True, False)))
        t_ow = timeit(lambda: cv.conv_wgrad(dy, x, torch.bfloat16, 0, 2, k))

        def tf(t):
            return "%.0f us (%.0f TF)" % (t, gf / (t * 1e-6) / 1e3)

        print("| %d,%d,%d,%d,%d | %.1f | %s | %s | %s | %s | %s | %s |" % (
            k, n, c, co, hw, gf, tf(t_mf), tf(t_of), tf(t_md), tf(t_od), tf(t_mw), tf(t_ow)),
            flush=True)


def bench_attn(args):
    """SDPA fwd+bwd at the BERT-large / GPT-2-medium shapes: AOTriton vs CK flash."""
    dev = "cuda"
    shapes = [("bert-large", 32, 16, 512, 64, False), ("gpt2-medium", 8, 16, 1024, 64, True)]
    from apex_example_amd import _native

    for name, b, h, s_, d, causal in shapes:  # this framework's gfx950 kernels, [B,S,H,D]
        q, k, v = (torch.randn(b, s_, h, d, device=dev, dtype=torch.bfloat16, requires_grad=True)
                   for _ in range(3))
        do = torch.randn(b, s_, h, d, device=dev, dtype=torch.bfloat16)
        # ~2 s of untimed calls first: without it the first variant timed read 10 %
        # slower than the same kernels later in the process (clock / first-use ramp)
        A = _native.require().attn
        o, lse = A.fwd(q, k, v, causal, 0.1, 1234, 1.0 / d ** 0.5)
        dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
        t_end = time.time() + 2.0
        while time.time() < t_end:
            for _ in range(10):
                A.fwd(q, k, v, causal, 0.1, 1234, 1.0 / d ** 0.5)
                A.bwd(do, q, k, v, o, lse, causal, 0.1, 1234, 1.0 / d ** 0.5, dq, dk, dv)
            torch.cuda.synchronize()
        for vname in ("gfx950",):
            for p in (0.0, 0.1):  # training runs use attention dropout 0.1
                # the native calls themselves (the autograd engine adds a ~80 us host floor
                # per backward call that hid the kernels; round-4 fix of the committed
                # table, whose 232 us GPT-2 row was that floor plus first-use effects)
                A = _native.require().attn
                sc = 1.0 / d ** 0.5
                f = lambda p=p: A.fwd(q, k, v, causal, p, 1234, sc)  # noqa: E731
                tf_ = timeit(f, iters=50, warmup=10)
                o, lse = f()
                dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
                tb = timeit(lambda p=p: A.bwd(do, q, k, v, o, lse, causal, p, 1234, sc, dq, dk,
                                              dv), iters=50, warmup=10)
                fl = 4 * b * h * s_ * s_ * d * (0.5 if causal else 1.0)
                print("%-12s %-12s p=%.1f fwd %.0f us (%.0f TF)  bwd %.0f us (%.0f TF)" % (
                    vname, name, p, tf_,
                    fl / (tf_ * 1e-6) / 1e12, tb, 2.5 * fl / (tb * 1e-6) / 1e12), flush=True)
    for lib in ("default", "ck"):
        try:
            torch.backends.cuda.preferred_rocm_fa_library(lib)
        except Exception as e:  # noqa: BLE001
            print("backend %s unavailable: %s" % (lib, e))
            continue
        for name, b, h, s_, d, causal in shapes:
            q, k, v = (torch.randn(b, h, s_, d, device=dev, dtype=torch.bfloat16, requires_grad=True)
                       for _ in range(3))
            do = torch.randn(b, h, s_, d, device=dev, dtype=torch.bfloat16)
            f = lambda: F.scaled_dot_product_attention(q, k, v, is_causal=causal)  # noqa: E731
            try:
                tf_ = timeit(f)
                o = f()
                tb = timeit(lambda: torch.autograd.grad(o, (q, k, v), do, retain_graph=True))
            except Exception as e:  # noqa: BLE001
                print("%s %s failed: %s" % (lib, name, str(e)[:200]))
                continue
            fl = 4 * b * h * s_ * s_ * d * (0.5 if causal else 1.0)
            print("%-8s %-12s fwd %.0f us (%.0f TF)  bwd %.0f us (%.0f TF)" % (
                lib, name, tf_, fl / (tf_ * 1e-6) / 1e12, tb, 2.5 * fl / (tb * 1e-6) / 1e12),
                flush=True)
    bench_attn_packed(args)


def bench_attn_packed(args):
    """Packed variable-length attention (fwd_varlen / bwd_varlen on the real tokens) against
    the padded [32, 512] call with the equivalent key-padding mask: B = 32 sequences with
    lengths drawn once (seed 0) uniformly from [64, 512], H = 16, bf16, forward + backward.
    The two are timed alternately, three rounds each; the share of real (query, key) pairs
    is what the packed time would be of the padded one if time followed the pairs alone."""
    from apex_example_amd import _native

    dev, dt, B, S, H, d = "cuda", torch.bfloat16, 32, 512, 16, 64
    A = _native.require().attn
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(64, S + 1, (B,), generator=g)
    T, sc = int(lens.sum()), 1.0 / d ** 0.5
    pairs = float((lens.double() ** 2).sum()) / (B * S * S)
    print("lengths %s" % lens.tolist())
    print("T = %d of %d tokens (%.3f), real (query, key) pairs %.3f of the padded batch's" % (
        T, B * S, T / (B * S), pairs))
    cu = torch.nn.functional.pad(lens.cumsum(0), (1, 0)).to(torch.int32).to(dev)
    gone = (torch.arange(S).view(1, S) >= lens.view(B, 1)).to(dev)
    kb, kl = A.prepare_key_mask(gone, S)   # once per forward for all layers: not timed
    pq, pk, pv, pdo = (torch.randn(B, S, H, d, device=dev, dtype=dt) for _ in range(4))
    keep = (~gone).reshape(-1).nonzero().squeeze(1)
    q, k, v, do = (t.reshape(B * S, H, d).index_select(0, keep) for t in (pq, pk, pv, pdo))
    pg = [torch.empty_like(pq) for _ in range(3)]
    vg = [torch.empty_like(q) for _ in range(3)]
    for p in (0.0, 0.1):
        po, plse = A.fwd(pq, pk, pv, False, p, 1234, sc, kb, kl)
        o, lse = A.fwd_varlen(q, k, v, cu, S, False, p, 1234, sc)
        calls = {
            "padded fwd": lambda: A.fwd(pq, pk, pv, False, p, 1234, sc, kb, kl),
            "packed fwd": lambda: A.fwd_varlen(q, k, v, cu, S, False, p, 1234, sc),
            "padded bwd": lambda: A.bwd(pdo, pq, pk, pv, po, plse, False, p, 1234, sc, *pg, kb,
                                        kl),
            "packed bwd": lambda: A.bwd_varlen(do, q, k, v, o, lse, cu, S, False, p, 1234, sc,
                                               *vg),
        }
        t_end = time.time() + 2.0   # untimed first (clock / first-use ramp, see bench_attn)
        while time.time() < t_end:
            for f in calls.values():
                f()
            torch.cuda.synchronize()
        times = {n: [] for n in calls}
        for _ in range(3):
            for n, f in calls.items():
                times[n].append(timeit(f, iters=100, warmup=10))
        best = {n: min(ts) for n, ts in times.items()}
        for n, ts in times.items():
            print("p=%.1f %s: %s us" % (p, n, " ".join("%.0f" % t for t in ts)), flush=True)
        pad_t = best["padded fwd"] + best["padded bwd"]
        pack_t = best["packed fwd"] + best["packed bwd"]
        print("p=%.1f fwd+bwd padded %.0f us, packed %.0f us: %.3f of padded (pairs %.3f)" % (
            p, pad_t, pack_t, pack_t / pad_t, pairs), flush=True)


def bench_optim(args):
    """Optimizer-kernel bandwidth on ResNet-50's 161 tensors, straight through
    amp_C (no Python optimizer bookkeeping in the loop)."""
    from apex_example_amd import amp_C
    from apex_example_amd.models import resnet50
    from apex_example_amd.optimizers import FusedAdam, FusedSGD

    dev = "cuda"
    m = resnet50().to(dev)
    ps = [p.detach() for p in m.parameters()]
    n = sum(p.numel() for p in ps)
    g32 = [torch.randn_like(p) for p in ps]
    g16 = [g.to(torch.bfloat16) for g in g32]
    mom = [torch.zeros_like(p) for p in ps]
    v = [torch.zeros_like(p) for p in ps]
    cp = [p.to(torch.bfloat16) for p in ps]
    noop = torch.zeros(1, dtype=torch.int32, device=dev)
    cases = [
        ("SGD fp32 [g,p,m]", 20, lambda: amp_C.multi_tensor_sgd(
            0, noop, [g32, ps, mom], 1e-4, 0.9, 0.0, 0.1, False, False, False, 1.0)),
        ("SGD O2 [g16,p,m,copy16]", 20, lambda: amp_C.multi_tensor_sgd(
            0, noop, [g16, ps, mom, cp], 1e-4, 0.9, 0.0, 0.1, False, False, False, 1 / 1024.)),
        ("Adam fp32 [g,p,m,v]", 28, lambda: amp_C.multi_tensor_adam(
            0, noop, [g32, ps, mom, v], 1e-3, 0.9, 0.999, 1e-8, 1, 1, True, 0.0)),
        ("LAMB fp32 [g,p,m,v]", 40, lambda: amp_C.multi_tensor_lamb(
            0, noop, [g32, ps, mom, v], 1e-3, 0.9, 0.999, 1e-6, 1, True, 0.01, True, 1,
            torch.ones(1, device=dev), 1.0)),
    ]
    print("| kernel | B/param | time |")
    print("|---|---|---|")
    for name, bpp, fn in cases:
        t = timeit(fn, iters=50, warmup=5)
        print("| %s | %d | %.1f us %.2f TB/s |" % (name, bpp, t, bpp * n / (t * 1e-6) / 1e12),
              flush=True)
    # whole optimizer.step() (Python bookkeeping included) vs torch's fused optimizers
    for p_, g_ in zip(ps, g32):
        p_.grad = g_
    o = FusedSGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-4)
    o.step()
    print("FusedSGD.step() fp32: %.1f us" % timeit(lambda: o.step()))
    ref = torch.optim.SGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-4, fused=True)
    ref.step()
    print("torch.optim.SGD(fused).step(): %.1f us" % timeit(lambda: ref.step()))
    oa = FusedAdam(ps, lr=1e-3)
    oa.step()
    print("FusedAdam.step() fp32: %.1f us" % timeit(lambda: oa.step()))
    ra = torch.optim.AdamW(ps, lr=1e-3, fused=True)
    ra.step()
    print("torch.optim.AdamW(fused).step(): %.1f us" % timeit(lambda: ra.step()))


def bench_ln(args):
    from apex_example_amd.normalization import FusedLayerNorm

    dev = "cuda"
    from apex_example_amd import _native

    C = _native.require().layer_norm
    print("| rows x n2 (dtype) | MB in | fused fwd | torch fwd | fused bwd (dx,dg,db) | torch bwd "
          "| native bwd call (kernels only) |")
    print("|---|---|---|---|---|---|---|")
    for (rows, n2, dt) in [(16384, 1024, torch.bfloat16), (8192, 1024, torch.float32),
                           (16384, 768, torch.bfloat16), (4096, 4096, torch.bfloat16),
                           (65536, 1024, torch.bfloat16)]:
        x = torch.randn(rows, n2, device=dev, dtype=dt, requires_grad=True)
        dy = torch.randn(rows, n2, device=dev, dtype=dt)
        fl = FusedLayerNorm(n2).to(dev).to(dt)
        tl = torch.nn.LayerNorm(n2).to(dev).to(dt)
        nb = x.numel() * x.element_size()
        res = []
        for m in (fl, tl):
            tf = timeit(lambda: m(x))
            y = m(x)
            tb = timeit(lambda: torch.autograd.grad(y, [x, m.weight, m.bias], dy,
                                                    retain_graph=True))
            res.append((tf, tb))

        def tbs(nbytes, t):
            return "%.1f us (%.2f TB/s)" % (t, nbytes / (t * 1e-6) / 1e12)

        # the autograd.grad columns carry the autograd engine's ~80 us host floor per
        # call; this one times the native backward (dx + the dgamma / dbeta partials and
        # their column reduction) as the model's backward launches it
        xi = x.detach().contiguous()
        _, mean, invvar = C.forward(xi, n2, fl.weight, fl.bias, fl.eps, False)
        tn = timeit(lambda: C.backward(dy, xi, mean, invvar, n2, fl.weight, True, True, False))

        print("| %dx%d (%s) | %.1f | %s | %s | %s | %s | %s |" % (
            rows, n2, str(dt).split(".")[1], nb / 1e6, tbs(2 * nb, res[0][0]),
            tbs(2 * nb, res[1][0]), tbs(3 * nb, res[0][1]), tbs(3 * nb, res[1][1]),
            tbs(3 * nb, tn)))


def bench_ln_join(args):
    """GPT-2-medium O1 sublayer join in isolation: s = x + dropout(h), y = LN(s) with an
    fp32 residual x and fp16 h / y (bs 8 x seq 1024 rows).  Bytes: fwd reads x, h and
    writes s, y; bwd reads s, dy, ds_ext and writes ds, dh."""
    from apex_example_amd.normalization import FusedLayerNorm, fused_add_dropout_layer_norm

    dev = "cuda"
    print("| rows x n2 | p | fwd | bwd (ds, dh, dg, db) | blocks env |")
    print("|---|---|---|---|---|")
    for rows, n2, p in [(8192, 1024, 0.1), (8192, 1024, 0.0), (16384, 1024, 0.1)]:
        x = torch.randn(rows, n2, device=dev, requires_grad=True)
        h = torch.randn(rows, n2, device=dev, dtype=torch.float16, requires_grad=True)
        ln = FusedLayerNorm(n2).to(dev)
        dy = torch.randn(rows, n2, device=dev, dtype=torch.float16)
        ds = torch.randn(rows, n2, device=dev)
        tf = timeit(lambda: fused_add_dropout_layer_norm(x, h, ln, p, True, True))
        y, s = fused_add_dropout_layer_norm(x, h, ln, p, True, True)
        assert y.dtype == torch.float16 and s.dtype == torch.float32
        tb = timeit(lambda: torch.autograd.grad((y, s), [x, h, ln.weight, ln.bias], (dy, ds),
                                                retain_graph=True))
        fb = rows * n2 * (4 + 2 + 4 + 2)
        bb = rows * n2 * (4 + 2 + 4 + 4 + 2)
        print("| %dx%d | %.1f | %.1f us (%.2f TB/s) | %.1f us (%.2f TB/s) |" % (
            rows, n2, p, tf, fb / tf / 1e6, tb, bb / tb / 1e6), flush=True)


def bench_conv_bnbwd(args):
    """BN backward folded into the dgrad conv epilogue vs the unfused chain, per ResNet-50
    shape (bs 256): unfused = dgrad (own kernel, or the hipBLASLt addmm with the residual
    gradient) + BN reduce + BN elementwise backward (+ dz); fused = conv_fwd_bnbwd +
    slab_reduce_grad + elementwise backward (no dz)."""
    from apex_example_amd import _native

    C = _native.require()
    dev = "cuda"
    cl = torch.channels_last
    print("| case | dy -> BN ch @ HW | unfused us (dgrad / reduce / elem) | fused us (conv / fin+elem) | saved |")
    print("|---|---|---|---|---|")
    cases = []
    for hw, p in ((56, 64), (28, 128), (14, 256), (7, 512)):
        cases.append(("3x3 -> bn1", p, p, hw, 3, 2, False))
        cases.append(("1x1 4p->p -> bn2", 4 * p, p, hw, 1, 2, False))
        cases.append(("1x1 p->4p +skip -> bn3", p, 4 * p, hw, 1, 1, True))
    tot = [0.0, 0.0]
    for name, cd, co, hw, k, mode, skip in cases:
        n = 256
        dy = torch.randn(n, cd, hw, hw, device=dev).to(torch.bfloat16).contiguous(memory_format=cl)
        wt = (torch.randn(co, cd, k, k, device=dev) / (cd * k * k) ** 0.5).to(
            torch.bfloat16).contiguous(memory_format=cl)
        x = torch.randn(n, co, hw, hw, device=dev).to(torch.bfloat16).contiguous(memory_format=cl)
        add = torch.randn_like(x) if skip else None
        mean = torch.zeros(co, device=dev)
        invstd = torch.ones(co, device=dev)
        bw, bb = torch.ones(co, device=dev), torch.zeros(co, device=dev)
        z = torch.randn_like(x) if skip else None
        _, mask = C.bn.apply_mask(x, mean, invstd, bw, bb, z, True) if skip else (None, None)
        M = n * hw * hw
        w2 = wt.reshape(co, cd).t().contiguous() if k == 1 else None

        def dgrad():
            if skip:
                return torch.addmm(add.permute(0, 2, 3, 1).reshape(M, co),
                                   dy.permute(0, 2, 3, 1).reshape(M, cd), w2)
            return C.conv.conv_fwd(dy, wt, 1)
        o = dgrad()
        o4 = o if not skip else o.view(n, hw, hw, co).permute(0, 3, 1, 2)
        zz = None if skip else None

        def red():
            return C.bn.reduce_grad(o4, x, mean, invstd, bw, bb, zz, True, True, mask=mask)
        sdy, sdx, _, _ = red()

        def elem():
            return C.bn.backward_elemt(o4, x, mean, invstd, bw, bb, sdy, sdx, float(M), zz, True,
                                       skip, mask=mask)
        t_d, t_r, t_e = timeit(dgrad), timeit(red), timeit(elem)
        g, slab = C.conv.conv_fwd_bnbwd(dy, wt, add, x, mask, mean, invstd, bw, bb,
                                        1 if skip else mode)

        def fused_conv():
            return C.conv.conv_fwd_bnbwd(dy, wt, add, x, mask, mean, invstd, bw, bb,
                                         1 if skip else mode)

        def fin_elem():
            a, b_, _, _ = C.bn.slab_reduce_grad(slab, invstd, bw, True)
            return C.bn.backward_elemt(g, x, mean, invstd, bw, bb, a, b_, float(M), None, False,
                                       False)
        t_f, t_fe = timeit(fused_conv), timeit(fin_elem)
        un, fu = t_d + t_r + t_e, t_f + t_fe
        tot[0] += un
        tot[1] += fu
        print("| %s | %d -> %d @ %d | %.0f (%.0f / %.0f / %.0f) | %.0f (%.0f / %.0f) | %+.0f |" % (
            name, cd, co, hw, un, t_d, t_r, t_e, fu, t_f, t_fe, un - fu), flush=True)
    print("| total (one layer per case) | | %.0f | %.0f | %+.0f |" % (tot[0], tot[1],
                                                                    tot[0] - tot[1]))


def bench_lamb(args):
    from apex_example_amd.optimizers import FusedAdam, FusedLAMB
    from apex_example_amd.models.bert import bert_large

    dev = "cuda"
    m = bert_large().to(dev)
    ps = list(m.parameters())
    n = sum(p.numel() for p in ps)
    for p in ps:
        p.grad = torch.randn_like(p)
    for name, o, bpp in [("FusedLAMB", FusedLAMB(ps, lr=1e-3, weight_decay=0.01), 32),
                         ("FusedAdam", FusedAdam(ps, lr=1e-3, weight_decay=0.01), 28),
                         ("torch AdamW(fused)", torch.optim.AdamW(ps, lr=1e-3, fused=True), 28)]:
        o.step()
        t = timeit(lambda: o.step(), iters=10)
        print("%s fp32 BERT-large (%d params, %d tensors): %.0f us, %.2f TB/s (%d B/param min)" % (
            name, n, len(ps), t, bpp * n / (t * 1e-6) / 1e12, bpp))



def bench_conv1x1_stats(args):
    """Channel-expanding / reducing 1x1 conv forward feeding a BatchNorm: hipBLASLt GEMM
    + the BN statistics pass vs the own MFMA kernel writing the statistics in its
    epilogue (conv_fwd_stats + the slab finalize), and the own kernel alone."""
    from apex_example_amd import _native

    C = _native.require()
    dev = "cuda"
    shapes = [(256, 64, 256, 56), (256, 256, 64, 56), (256, 128, 512, 28), (256, 512, 128, 28),
              (256, 256, 1024, 14), (256, 1024, 256, 14), (256, 512, 2048, 7),
              (256, 2048, 512, 7), (256, 64, 64, 56)]
    print("| N,Cin,Cout,HW | MB | hipBLASLt | + stats pass | own | own + epilogue stats + finalize |")
    print("|---|---|---|---|---|---|")
    for (n, ci, co, hw) in shapes:
        x = torch.randn(n, ci, hw, hw, device=dev, dtype=torch.bfloat16).to(
            memory_format=torch.channels_last)
        w = (torch.randn(co, ci, 1, 1, device=dev) * 0.05).to(torch.bfloat16).to(
            memory_format=torch.channels_last)
        M = n * hw * hw
        x2 = x.permute(0, 2, 3, 1).reshape(M, ci)
        w2 = w.reshape(co, ci)
        mb = (M * ci + M * co) * 2 / 1e6
        rm = torch.zeros(co, device=dev)
        rv = torch.ones(co, device=dev)
        y_nhwc = torch.mm(x2, w2.t()).view(n, hw, hw, co).permute(0, 3, 1, 2)

        def gemm_stats():
            y = torch.mm(x2, w2.t()).view(n, hw, hw, co).permute(0, 3, 1, 2)
            C.bn.train_stats(y, rm, rv, None, 1e-5, 0.1)

        def own_stats():
            y, slab = C.conv.conv_fwd_stats(x, w, 1, rm)
            C.bn.slab_train_stats(slab, M, rm, rm, rv, None, 1e-5, 0.1)

        t_g = timeit(lambda: torch.mm(x2, w2.t()))
        t_gs = timeit(gemm_stats)
        t_o = timeit(lambda: C.conv.conv_fwd(x, w, 1))
        t_os = timeit(own_stats)
        del y_nhwc

        def bw(t):
            return "%.0f us (%.2f TB/s)" % (t, mb / 1e6 / (t * 1e-6))

        print("| %d,%d,%d,%d | %.0f | %s | %.0f us | %s | %.0f us |" % (
            n, ci, co, hw, mb, bw(t_g), t_gs, bw(t_o), t_os), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["bn", "bn-tune", "conv1x1", "conv1x1-own", "conv1x1-stats", "wgrad", "wgrad-o1", "wgrad-dense", "conv3x3", "conv-s2", "optim", "ln", "ln-join", "conv-bnbwd", "lamb",
                             "attn", "attn-packed"])
    a = ap.parse_args()
    {"bn": bench_bn, "bn-tune": bench_bn_tune, "conv1x1": bench_conv1x1, "conv1x1-own": bench_conv1x1_own, "conv1x1-stats": bench_conv1x1_stats, "wgrad-o1": bench_wgrad_o1, "wgrad-dense": bench_wgrad_dense, "optim": bench_optim,
     "ln": bench_ln, "ln-join": bench_ln_join, "conv-bnbwd": bench_conv_bnbwd, "lamb": bench_lamb, "wgrad": bench_wgrad,
     "conv3x3": bench_conv3x3, "conv-s2": bench_conv_s2, "attn": bench_attn,
     "attn-packed": bench_attn_packed}[a.what](a)


if __name__ == "__main__":
    main()
