// Grouped-query and multi-query attention (Hkv < H key/value heads, query head h reading
// key/value head h / G with G = H / Hkv: torch's enable_gqa, the Llama / Megatron layout):
// the launches of the GQA mode of the head dim 64 and 128 kernels.
//
// The kernels are the templates of attention.hip and attention_d128.hip; this file includes
// both for them (ATTN_KERNELS_ONLY leaves their host halves out), so that the GQA
// instantiations are compiled here, with the flags of attention_d128.hip (tools/build_ext.py:
// packed fp32 VALU forms off), while the objects of those two files keep their code.
//
// Grids.  Forward and dQ: one workgroup per (128-query tile, b, QUERY head), as with equal
// head counts - G workgroups stream the same K / V head, G times fewer bytes behind them in
// L2 / HBM.  dK/dV: one workgroup per (128-key tile, b, KEY/VALUE head), which walks the
// query tiles of its G query heads (the kernel's comment has the ring): the grid is G times
// smaller and each workgroup G times longer, K / V are loaded once per group and dK / dV are
// stored once from fp32 sums, with no reduction launch and no atomics.  The price is
// parallelism where B * Hkv * ceil(Sk / 128) is small (multi-query heads at small batch);
// docs/PERF.md, "Attention: grouped-query heads", has the measured cases.
#define ATTN_KERNELS_ONLY 1
#include "attention.hip"
#include "attention_d128.hip"

namespace amd {

namespace {
bool gqa_head_dim_128(const char* who, const AttnProblem& p) {
  if (p.D != 64 && p.D != 128) {
    fprintf(stderr, "%s: head dim must be 64 or 128, got %d\n", who, p.D);
    abort();
  }
  return p.D == 128;
}
}  // namespace

void attn_fwd_gqa(const AttnProblem& p, void* o, float* lse, hipStream_t st) {
  const bool d128 = gqa_head_dim_128("attn_fwd", p);
  AttnArgs a = kernel_args<AttnArgs>("attn_fwd", p);
  a.o = o; a.lse = lse;
  dim3 grid((p.Sq + 127) / 128, p.B * p.H), block(kAT);
  dispatch_gqa(p, a.thr8 != 0, [&](auto t, auto c, auto d, auto m) {
    if (d128) hipLaunchKernelGGL((ATTN_GQA_KERNEL(attn128_fwd_k)), grid, block, 0, st, a);
    else hipLaunchKernelGGL((ATTN_GQA_KERNEL(attn_fwd_k)), grid, block, 0, st, a);
  });
}

void attn_bwd_gqa(const AttnProblem& p, const AttnBwd& g, hipStream_t st) {
  const bool d128 = gqa_head_dim_128("attn_bwd", p);
  AttnBwdArgs a = bwd_kernel_args("attn_bwd", p, g);
  // dQ first (it writes D per query head), then dK/dV over the key/value heads
  dim3 qgrid((p.Sq + 127) / 128, p.B * p.H), kgrid((p.Sk + 127) / 128, p.B * p.Hkv), block(kAT);
  dispatch_gqa(p, a.thr8 != 0, [&](auto t, auto c, auto d, auto m) {
    if (d128) {
      hipLaunchKernelGGL((ATTN_GQA_KERNEL(attn128_bwd_dq_k)), qgrid, block, 0, st, a);
      hipLaunchKernelGGL((ATTN_GQA_KERNEL(attn128_bwd_dkdv_k)), kgrid, block, 0, st, a);
    } else {
      hipLaunchKernelGGL((ATTN_GQA_KERNEL(attn_bwd_dq_k)), qgrid, block, 0, st, a);
      hipLaunchKernelGGL((ATTN_GQA_KERNEL(attn_bwd_dkdv_k)), kgrid, block, 0, st, a);
    }
  });
}
#undef ATTN_KERNEL
#undef ATTN_AMASK_KERNEL
#undef ATTN_GQA_KERNEL

}  // namespace amd
