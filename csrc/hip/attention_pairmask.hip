// Boolean [Sq, Sk] attention masks for the fused attention kernels (the AMASK mode of
// attention.hip and attention_d128.hip): the prepare kernel that turns mask bytes into bit
// tiles, and the head dim 64 launches under such a mask.
//
// Why bits.  A lane of the forward / dQ kernels owns one query and sees exactly 64 keys of
// it per K/V tile; a lane of the dK/dV kernel owns one key and sees 64 queries of it per
// Q / dO tile.  So the whole mask of a lane and a tile is ONE 64-bit word, and the words of
// a workgroup's 128 rows and one tile are a contiguous 1 KiB: one global_load_lds by one
// wave puts them on the ring beside the tile, a ds_read_b64 gives the lane its word, and
// each accumulator register tests a compile-time bit of it (pair_word / pair_bit in
// attention_common.h).  An fp32 bias per pair would move 32 x the bytes.
//
// Prepared form (set bit = attend; bits past Sq or Sk are 0), Bm = 1 shared or B:
//   wq [Bm][ceil(Sq/128)][ceil(Sk/64)][128]: word (qt, kt, r) = keys 64 kt .. 64 kt + 63 of
//      query 128 qt + r - forward and dQ;
//   wk [Bm][ceil(Sk/128)][ceil(Sq/64)][128]: word (kt, qt, r) = queries 64 qt .. 64 qt + 63
//      of key 128 kt + r - dK/dV;
//   cq, ck: one class byte per 1 KiB block: 0 dead (no bit), 2 full (every bit, which puts
//      the block inside Sq x Sk), 1 mixed.  The kernels walk the non-dead blocks of their
//      row (PairTiles): dead tiles cost no DMA and no math wherever they lie, full tiles run
//      the mask-free math, mixed ones test bits.
//
// The head dim 64 kernels are templates of attention.hip; this file includes it for them
// (ATTN_KERNELS_ONLY leaves its host half out) so that their AMASK instantiations are
// compiled with this file's flags (tools/build_ext.py: packed fp32 VALU forms off, as for
// attention_d128.hip) while attention.hip's own object, flags and code stay as they were.
#define ATTN_KERNELS_ONLY 1
#include "attention.hip"

namespace amd {

namespace {

// One workgroup per 128 x 128 block of pairs: the block's attend bytes go to LDS once (row
// pitch 132 bytes = 33 words, so the 64 rows a transposed ballot reads fall into different
// banks), then every wave forms the words of 32 rows of each side with __ballot over 64
// bytes - along the row for wq, down the column for wk - lane i keeping ballot i, so a wave
// stores 2 x 32 consecutive words per side.  The block covers two 64-wide tiles per side;
// their classes come from per-wave any / all flags combined through LDS.
constexpr int kPmPitch = 132;

__global__ void __launch_bounds__(256) attn_pair_mask_prep_k(
    const unsigned char* __restrict__ mask, int64_t mask_sb, const unsigned char* __restrict__ kpm,
    int Sq, int Sk, unsigned long long* __restrict__ wq, unsigned char* __restrict__ cq,
    unsigned long long* __restrict__ wk, unsigned char* __restrict__ ck) {
  __shared__ unsigned char att[128 * kPmPitch];
  __shared__ int some[4], every[4];  // [0, 1]: wq tiles j = 0, 1; [2, 3]: wk tiles
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int K = blockIdx.x, Q = blockIdx.y, b = blockIdx.z;
  const int nq64 = (Sq + 63) / 64, nk64 = (Sk + 63) / 64;
  const int nq128 = (Sq + 127) / 128, nk128 = (Sk + 127) / 128;
  const unsigned char* mb = mask + b * mask_sb;
  const unsigned char* kb = kpm != nullptr ? kpm + (int64_t)b * Sk : nullptr;
  if (tid < 4) {
    some[tid] = 0;
    every[tid] = 1;
  }
  for (int i = tid; i < 128 * 128; i += 256) {
    const int r = i >> 7, c = i & 127;
    const int q = 128 * Q + r, k = 128 * K + c;
    bool attend = false;
    if (q < Sq && k < Sk) attend = mb[(int64_t)q * Sk + k] == 0 && (kb == nullptr || kb[k] == 0);
    att[r * kPmPitch + c] = attend ? 1 : 0;
  }
  __syncthreads();
  // lane i of wave w keeps the word of row 32 w + (i & 31) against 64-wide tile j = i >> 5
  unsigned long long mq = 0, mk = 0;
#pragma unroll 4
  for (int i = 0; i < 64; ++i) {
    const int j = i >> 5, r = 32 * wid + (i & 31);
    const unsigned long long bq = __ballot(att[r * kPmPitch + 64 * j + lane] != 0);
    const unsigned long long bk = __ballot(att[(64 * j + lane) * kPmPitch + r] != 0);
    if (lane == i) {
      mq = bq;
      mk = bk;
    }
  }
  const int j = lane >> 5, r = 32 * wid + (lane & 31);
  const bool hasq = 2 * K + j < nk64, hask = 2 * Q + j < nq64;  // the tile exists on that side
  const int64_t tq = ((int64_t)b * nq128 + Q) * nk64 + 2 * K + j;
  const int64_t tk = ((int64_t)b * nk128 + K) * nq64 + 2 * Q + j;
  if (hasq) wq[tq * 128 + r] = mq;
  if (hask) wk[tk * 128 + r] = mk;
  // per wave and tile: any bit, every bit (lanes of the other tile vote neutral)
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const bool mine = j == jj;
    if (__any(mine && mq != 0)) some[jj] = 1;
    if (!__all(!mine || mq == ~0ull)) every[jj] = 0;
    if (__any(mine && mk != 0)) some[2 + jj] = 1;
    if (!__all(!mine || mk == ~0ull)) every[2 + jj] = 0;
  }
  __syncthreads();
  if (tid < 4) {
    const int jj = tid & 1;
    const unsigned char cls = every[tid] ? 2 : (some[tid] ? 1 : 0);
    if (tid < 2) {
      if (2 * K + jj < nk64) cq[((int64_t)b * nq128 + Q) * nk64 + 2 * K + jj] = cls;
    } else {
      if (2 * Q + jj < nq64) ck[((int64_t)b * nk128 + K) * nq64 + 2 * Q + jj] = cls;
    }
  }
}

}  // namespace

void attn_prepare_pair_mask(const unsigned char* mask, int64_t mask_sb, const unsigned char* kpm,
                            int Bm, int Sq, int Sk, unsigned long long* wq, unsigned char* cq,
                            unsigned long long* wk, unsigned char* ck, hipStream_t st) {
  dim3 grid((Sk + 127) / 128, (Sq + 127) / 128, Bm), block(256);
  hipLaunchKernelGGL(attn_pair_mask_prep_k, grid, block, 0, st, mask, mask_sb, kpm, Sq, Sk, wq, cq,
                     wk, ck);
}

void attn_fwd_amask64(const AttnProblem& p, void* o, float* lse, hipStream_t st) {
  AttnArgs a = kernel_args<AttnArgs>("attn_fwd", p);
  a.o = o; a.lse = lse;
  dim3 grid((p.Sq + 127) / 128, p.B * p.H), block(kAT);
  dispatch_amask(p, a.thr8 != 0, [&](auto t, auto d) {
    hipLaunchKernelGGL((ATTN_AMASK_KERNEL(attn_fwd_k)), grid, block, 0, st, a);
  });
}

void attn_bwd_amask64(const AttnProblem& p, const AttnBwd& g, hipStream_t st) {
  AttnBwdArgs a = bwd_kernel_args("attn_bwd", p, g);
  dim3 qgrid((p.Sq + 127) / 128, p.B * p.H), kgrid((p.Sk + 127) / 128, p.B * p.H), block(kAT);
  dispatch_amask(p, a.thr8 != 0, [&](auto t, auto d) {
    hipLaunchKernelGGL((ATTN_AMASK_KERNEL(attn_bwd_dq_k)), qgrid, block, 0, st, a);
    hipLaunchKernelGGL((ATTN_AMASK_KERNEL(attn_bwd_dkdv_k)), kgrid, block, 0, st, a);
  });
}
#undef ATTN_KERNEL
#undef ATTN_AMASK_KERNEL
#undef ATTN_GQA_KERNEL

}  // namespace amd
