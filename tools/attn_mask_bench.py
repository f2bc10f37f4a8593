#!/usr/bin/env python
"""Times the fused attention kernels with and without a key-padding mask against the
SDPA fallback, at BERT-large's attention shape (docs/PERF.md "Key-padding masks"), or
with `--seq-k` at a cross-attention shape: a [B, seq] query side against a [B, seq-k]
key side (docs/PERF.md "Cross-attention").

    python tools/attn_mask_bench.py                    # masked fused vs SDPA, padding sweep
    python tools/attn_mask_bench.py --seq 128 --seq-k 512   # the same, decoder over encoder
    python tools/attn_mask_bench.py --raw [--so PATH]  # mask-free raw kernel calls only;
                                                       # --so times another build's _C

Forward + backward per call, device events around `--iters` calls, `--windows` windows
after a warm-up; prints one JSON line per measurement (median, min, max in ms).
"""
import argparse
import importlib.machinery
import importlib.util
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, iters, windows, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    ms.sort()
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4),
            "ms_max": round(ms[-1], 4)}


def report(name, r, **extra):
    print(json.dumps(dict(name=name, **r, **extra)), flush=True)


def load_ext(path):
    if path is None:
        from apex_example_amd import _native

        return _native.require()
    loader = importlib.machinery.ExtensionFileLoader("apex_example_amd._C", path)
    spec = importlib.util.spec_from_loader("apex_example_amd._C", loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)   # bench.py's bert_large per-GPU batch
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--seq-k", type=int, default=None,
                    help="key-side length (default: --seq); the query side is --seq")
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--raw", action="store_true")
    ap.add_argument("--so", default=None)
    a = ap.parse_args()
    B, S, H = a.batch, a.seq, a.heads
    cross = a.seq_k is not None
    Sk = a.seq_k if cross else S
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    do = torch.randn(B, S, H, 64, device=dev, dtype=torch.bfloat16)
    t = lambda fn: timed(fn, a.iters, a.windows, a.warmup)  # noqa: E731
    cfg = dict(B=B, S=S, H=H, dropout=a.dropout)
    if cross:
        # the layouts of a q projection and a fused kv projection
        cfg["Sk"] = Sk
        qx = torch.randn(B, S, H, 64, device=dev, dtype=torch.bfloat16)
        kvx = torch.randn(B, Sk, 2, H, 64, device=dev, dtype=torch.bfloat16)
    else:
        qkv = torch.randn(B, S, 3, H, 64, device=dev, dtype=torch.bfloat16)

    if a.raw:
        C = load_ext(a.so).attn
        if cross:
            q, (k, v) = qx, kvx.unbind(2)
            dq = torch.empty_like(qx)
            dk, dv = torch.empty_like(kvx).unbind(2)
        else:
            q, k, v = qkv.unbind(2)
            dq, dk, dv = torch.empty_like(qkv).unbind(2)

        def raw():
            o, lse = C.fwd(q, k, v, False, a.dropout, 11, 0.125)
            C.bwd(do, q, k, v, o, lse, False, a.dropout, 11, 0.125, dq, dk, dv)

        report("fused_mask_free_raw", t(raw), so=a.so or "in-tree", **cfg)
        return

    from apex_example_amd.ops.attention import (fused_attention_kv, fused_attention_qkv,
                                                prepare_key_mask)

    if cross:
        xq, xkv = qx.clone().requires_grad_(True), kvx.clone().requires_grad_(True)

        def run_fused(pm):
            xq.grad = xkv.grad = None
            fused_attention_kv(xq, xkv, dropout_p=a.dropout, key_bias=pm).backward(do)

        def run_sdpa(mask):  # the fallback path on the same q and packed kv
            xq.grad = xkv.grad = None
            k, v = xkv.permute(2, 0, 3, 1, 4).unbind(0)
            o = F.scaled_dot_product_attention(xq.transpose(1, 2), k, v, attn_mask=mask,
                                               dropout_p=a.dropout)
            o.transpose(1, 2).backward(do)
    else:
        x = qkv.clone().requires_grad_(True)

        def run_fused(pm):
            x.grad = None
            fused_attention_qkv(x, dropout_p=a.dropout, key_bias=pm).backward(do)

        def run_sdpa(mask):  # the model's fallback path on the same packed qkv
            x.grad = None
            q, k, v = x.permute(2, 0, 3, 1, 4).unbind(0)
            o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=a.dropout)
            o.transpose(1, 2).backward(do)

    fu = t(lambda: run_fused(None))
    report("fused_mask_free", fu, **cfg)
    if cross:  # equal lengths: docs/PERF.md "Fused attention" has the mask-free comparison
        sd = t(lambda: run_sdpa(None))
        report("sdpa_mask_free", sd, **cfg)
        report("ratio_sdpa_over_fused", {"ratio": round(sd["ms_median"] / fu["ms_median"], 3)},
               padding="none")
    g = torch.Generator().manual_seed(0)
    sweeps = [("uniform[%d,%d]" % (Sk // 4, Sk),
               torch.randint(Sk // 4, Sk + 1, (B,), generator=g))]
    sweeps += [("len=%d" % n, torch.full((B,), n)) for n in (Sk, 3 * Sk // 4, Sk // 2, Sk // 4)]
    for label, lens in sweeps:
        keep = torch.arange(Sk).view(1, Sk) < lens.view(B, 1)
        add = ((1.0 - keep.float()) * -10000.0).to(dev)   # BERT's additive convention
        report("prepare_key_mask", t(lambda: prepare_key_mask(add)), padding=label, **cfg)
        pm = prepare_key_mask(add)
        mask = add.to(torch.bfloat16).view(B, 1, 1, Sk)
        fu = t(lambda: run_fused(pm))
        sd = t(lambda: run_sdpa(mask))
        report("fused_masked", fu, padding=label, mean_len=float(lens.float().mean()), **cfg)
        report("sdpa_masked", sd, padding=label, **cfg)
        report("ratio_sdpa_over_fused", {"ratio": round(sd["ms_median"] / fu["ms_median"], 3)},
               padding=label)
        # a boolean mask lets whole padded tiles be skipped (-10000 keeps them live)
        pb = prepare_key_mask(~keep.to(dev))
        report("fused_masked_bool", t(lambda: run_fused(pb)), padding=label, **cfg)


if __name__ == "__main__":
    main()
