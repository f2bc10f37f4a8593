"""conv3 recomputed inside bn3's passes (conv.conv1x1_stats_only / conv1x1_bn_apply /
conv1x1_bn_bwd) against the launches they replace, on the two ResNet-50 shapes (bs 256):
us per call, median of several device-event windows.  Each window cycles through three
sets of tensors so that no call finds its inputs in the Infinity Cache from the call before
(the 28x28 tensors would fit it).  The statistics finalize is the same launch on both
paths and is left out.

    python tools/diag/bn3_recompute_bench.py [batch]
"""
import sys

import torch

sys.path.insert(0, ".")
from apex_example_amd import _native  # noqa: E402

C = _native.require()
dev = "cuda"
cl = torch.channels_last
SETS, WINDOWS, PER = 3, 9, 6


def timeit(fn):
    """us per call: fn(i) runs on tensor set i % SETS."""
    for i in range(SETS):
        fn(i)
    ts = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(PER):
            fn(i % SETS)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000 / PER)
    ts.sort()
    return ts[len(ts) // 2]


def bf(*shape):
    return torch.randn(*shape, device=dev).to(torch.bfloat16).contiguous(memory_format=cl)


n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
print("| conv3 @ hw | conv+stats | apply | old fwd | stats-only | recompute+apply | new fwd "
      "| bwd elemt | recompute+bwd |")
print("|---" * 9 + "|")
for ci, co, hw in [(64, 256, 56), (128, 512, 28)]:
    a = [torch.relu(bf(n, ci, hw, hw)) for _ in range(SETS)]
    z = [bf(n, co, hw, hw) for _ in range(SETS)]
    g = [bf(n, co, hw, hw) for _ in range(SETS)]
    w = (torch.randn(co, ci, 1, 1, device=dev) / ci ** 0.5).to(torch.bfloat16).contiguous(
        memory_format=cl)
    shift = torch.zeros(co, device=dev)
    mean, invstd = torch.randn(co, device=dev) * 0.1, torch.rand(co, device=dev) + 0.5
    bw, bb = torch.rand(co, device=dev) + 0.5, torch.randn(co, device=dev) * 0.2
    sdy, sdx = torch.randn(co, device=dev), torch.randn(co, device=dev)
    cnt = float(n * hw * hw)
    x3 = [C.conv.conv_fwd_stats(a[i], w, 1, shift)[0] for i in range(SETS)]

    t_conv = timeit(lambda i: C.conv.conv_fwd_stats(a[i], w, 1, shift))
    t_apply = timeit(lambda i: C.bn.apply_mask(x3[i], mean, invstd, bw, bb, z[i], True))
    t_so = timeit(lambda i: C.conv.conv1x1_stats_only(a[i], w, shift))
    t_ra = timeit(lambda i: C.conv.conv1x1_bn_apply(a[i], w, x3[i], mean, invstd, bw, bb, z[i]))
    t_be = timeit(lambda i: C.bn.backward_elemt(g[i], x3[i], mean, invstd, bw, bb, sdy, sdx, cnt,
                                                None, False, False))
    t_rb = timeit(lambda i: C.conv.conv1x1_bn_bwd(a[i], w, g[i], mean, invstd, bw, sdy, sdx, cnt))
    print("| %d -> %d @ %d | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f |" % (
        ci, co, hw, t_conv, t_apply, t_conv + t_apply, t_so, t_ra, t_so + t_ra, t_be, t_rb),
        flush=True)
    del a, z, g, x3
