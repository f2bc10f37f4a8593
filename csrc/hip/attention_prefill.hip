// Fused attention of a chunk of new tokens over a KV cache for gfx950 (head dim 64 / 128, bf16 /
// fp16, forward only): the Sq new tokens of each batch element against the L_b keys of a
// [B, Smax, Hkv, D] cache that already holds a prefix - chunked prefill, the next turn of a
// conversation, a prompt behind a shared prefix, a long speculative draft.  The lengths, the
// bottom-right causal mask, the clip to Smax and the append are those of attention_decode.hip
// (read its header first); what differs is the shape of the work.  Decode has a few rows and a
// long cache, so its waves split the keys; here there are hundreds to thousands of rows, so the
// rows are split and the keys are shared, as in the training forward (attention.hip) - which
// cannot serve this step because its causal mask needs Sq == Sk and host lengths.
//
// Row order.  The R = G * Sq rows of one (batch element, key/value head) are ordered
//   token-major, r = i * G + g (token i, query head g of the group).  A workgroup of four waves
//   owns 128 consecutive rows, one row per lane (32 per wave, the 32 columns of the swapped
//   S^T = K . Q^T on v_mfma_f32_32x32x16; softmax lane-local up to the lane ^ 32 exchange, P.V
//   straight from the accumulators, V read transposed from LDS - the register layouts of
//   attn_fwd_k).  A row tile is therefore ceil(128 / G) consecutive TOKENS of all G heads: its
//   rows see nearly the same keys, so the causal bounds below are tight for every wave, and K /
//   V of the group are read once per tile for all its query heads.  G need not divide 32 or 128:
//   a token's heads may straddle waves and tiles, each lane carries its own (i, g).  Rows past R
//   repeat row R - 1 on load and are not stored.
// Shared K / V tiles.  The four waves share each 64-key K / V tile in LDS (D / 64 images of
//   [64][64] per operand: 16 KiB per tile at D = 64, 32 KiB at D = 128), double buffered and
//   filled by global_load_lds, each wave moving 16 rows; K with the swz_rows swizzle (row
//   fragments), V with swz_tr (transposed reads).  One s_waitcnt vmcnt(0) + barrier per tile
//   orders the ring, the refill of the other slot follows the barrier.  K / V pass through LDS
//   once per 128 rows.
// Causal skipping.  Row (i, g) sees keys j <= L_b - Sq + i.  A workgroup's key loop ends at the
//   last key of its last token; a wave stops computing at its own last token's last key (it
//   keeps feeding the ring); only tiles that reach past the last key of the wave's FIRST row
//   test the mask per element (such a tile may hold rows with no visible key yet: it takes the
//   -inf-safe softmax step, the tiles before it the plain one).  Keys at or past L_b are never
//   loaded: a tile that reaches past L_b clamps its row addresses to L_b - 1 (0 * NaN from a
//   torch.empty cache would poison o) and the mask covers them, every row's last key lying
//   below L_b.  A workgroup none of whose rows sees a key writes o = 0, lse = -inf and returns
//   before any DMA or barrier; a row that sees no key gets the same from the epilogue.
// Launch.  Grid (ceil(R / 128), Hkv, B), flattened and re-split as tile_of_block does: blocks
//   are dispatched in id order over the 8 XCDs, so the tiles of one (b, key/value head) are
//   Hkv * B ids apart (one XCD's L2 streams that head's K / V whenever Hkv * B % 8 == 0), and
//   the row tiles that see the most keys (the last ones) are dispatched FIRST.  Both orders were
//   timed on an MI355X (docs/PERF.md, "Attention: chunked prefill over a KV cache"): heavy
//   first is 9 - 10 % faster at B = 8 without a prefix (the light diagonal tiles fill the tail)
//   and within the spread of light first elsewhere, so it is the only order kept.  One launch,
//   no split-KV, no workspace, no atomics: results are bitwise reproducible.
// Append.  attn_decode_append (attention_decode.hip) stores k_new / v_new first, on the same
//   stream.
//
// Resources (hipcc -O3 gfx950 resource report, both dtypes alike): attn_prefill_k<D = 64> 32768 B
// LDS, 152 VGPRs, 0 AGPRs, occupancy 3 waves per SIMD; attn_prefill_k<D = 128> 65536 B LDS, 198
// VGPRs, 0 AGPRs, occupancy 2 waves per SIMD; ScratchSize 0, no SGPR or VGPR spill.
// Timings: docs/PERF.md, same section.
#include "attention_common.h"

namespace amd {

namespace {

struct PrefillArgs {
  const void* q;
  const void* k;
  const void* v;
  int64_t qsb, qss, qsh, ksb, kss, ksh, vsb, vss, vsh;  // element strides
  const int* lens;  // [B] keys in the cache before the call
  int append;       // 1: the Sq new rows are in the cache behind lens[b]
  void* o;          // [B][Sq][H][D]
  float* lse;       // [B][H][Sq]
  int H, Hkv, G, Sq, Smax, R;  // R = G * Sq rows per (b, key/value head)
  float scale_log2;
};

// attention_decode.hip's decode_len: the visible length, clipped to the rows the views hold
__device__ __forceinline__ int prefill_len(const int* lens, int b, int append, int Sq, int Smax) {
  int l = lens[b];
  l = l < 0 ? 0 : (l > Smax ? Smax : l);
  l += append ? Sq : 0;
  return l > Smax ? Smax : l;
}

template <typename T, int D>
__global__ void __launch_bounds__(kAT, 2) attn_prefill_k(PrefillArgs a) {
  typedef typename Frag<T>::v8 v8;
  constexpr int NI = D / kAD;           // 64-wide LDS images per K (or V) tile
  constexpr int IMG = kAKT * kARow;     // 8 KiB: one [64][64] image
  constexpr int BUF = 2 * NI * IMG;     // K and V of one tile
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * BUF];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hl = lane >> 5, c32 = lane & 31;
  // block -> (row tile, b, key/value head), heavy tiles first (the header's "Launch")
  const int nt = gridDim.x, nbh = gridDim.y * gridDim.z;
  const int id = blockIdx.x + nt * (blockIdx.y + gridDim.y * blockIdx.z);
  const int td = id / nbh, bh = id - td * nbh;
  const int tile = nt - 1 - td;
  const int b = bh / a.Hkv, hk = bh - b * a.Hkv;
  const int Sq = a.Sq, R = a.R, G = a.G;
  const int L = prefill_len(a.lens, b, a.append, Sq, a.Smax);

  // this lane's row (clamped: rows past R repeat row R - 1, never stored)
  const int r = tile * 128 + wid * 32 + c32;
  const int rr = r < R ? r : R - 1;
  const int qi = rr / G, g = rr - qi * G, hh = hk * G + g;
  const int lim = L - Sq + qi;  // the last key this row sees
  T* orow = static_cast<T*>(a.o) + (((int64_t)b * Sq + qi) * a.H + hh) * D;
  float* lrow = a.lse + ((int64_t)b * a.H + hh) * Sq + qi;

  // the workgroup's keys: [0, kend), up to the last key of its last token
  const int rlast = tile * 128 + 127 < R ? tile * 128 + 127 : R - 1;
  const int kend = L - Sq + rlast / G + 1;  // <= L
  if (kend <= 0) {  // no row sees a key: before any DMA or barrier
    if (r < R) {
#pragma unroll
      for (int j = 0; j < D / 2; j += 8)
        *reinterpret_cast<uint4*>(orow + hl * (D / 2) + j) = uint4{0, 0, 0, 0};
      if (hl == 0) *lrow = -INFINITY;
    }
    return;
  }
  const int nkt = (kend + kAKT - 1) / kAKT;

  // the wave's own bounds (wave-uniform): the last key of its last row, where it stops, and the
  // last key of its first row, past which tiles test the mask; a wave with no row computes nothing
  const int r0 = tile * 128 + wid * 32;
  const int wlast = r0 < R ? L - Sq + (r0 + 31 < R ? r0 + 31 : R - 1) / G : -1;
  const int wfull = L - Sq + (r0 < R ? r0 : R - 1) / G;

  const T* Q = static_cast<const T*>(a.q) + b * a.qsb + (int64_t)qi * a.qss + hh * a.qsh;
  const T* K = static_cast<const T*>(a.k) + b * a.ksb + hk * a.ksh;
  const T* V = static_cast<const T*>(a.v) + b * a.vsb + hk * a.vsh;

  // DMA: each wave fills rows 16 wid .. 16 wid + 15 of every image (2 x 1 KiB instructions)
  const int drow = lane >> 3, pch = lane & 7;
  uint32_t kof[2], vof[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (wid * 2 + i) * 8 + drow;
    kof[i] = row_off<T>(row, a.kss, (swz_rows(row, pch) - row * kARow) >> 4);  // logical chunk at pch
    vof[i] = row_off<T>(row, a.vss, (swz_tr(row, pch) - row * kARow) >> 4);
  }
  auto issue = [&](int kt, int buf) {
    unsigned char* Kl = lds + buf * BUF;
    unsigned char* Vl = Kl + NI * IMG;
    const int k0 = kt * kAKT;
    if (k0 + kAKT <= L) {
      const T* kb = tile_base(K, k0, a.kss);
      const T* vb = tile_base(V, k0, a.vss);
#pragma unroll
      for (int h = 0; h < NI; ++h)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          glds16o(kb + kAD * h, kof[i], Kl + h * IMG + (wid * 2 + i) * 1024);
          glds16o(vb + kAD * h, vof[i], Vl + h * IMG + (wid * 2 + i) * 1024);
        }
      return;
    }
    // the tile reaches past L: rows at or past L read row L - 1 (L >= kend >= 1 here)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (wid * 2 + i) * 8 + drow;
      const int key = k0 + row;
      const int kk = key < L ? key : L - 1;
      const int chk = (swz_rows(row, pch) - row * kARow) >> 4;
      const int chv = (swz_tr(row, pch) - row * kARow) >> 4;
#pragma unroll
      for (int h = 0; h < NI; ++h) {
        glds16(K + (int64_t)kk * a.kss + kAD * h + chk * 8, Kl + h * IMG + (wid * 2 + i) * 1024);
        glds16(V + (int64_t)kk * a.vss + kAD * h + chv * 8, Vl + h * IMG + (wid * 2 + i) * 1024);
      }
    }
  };

  f32x16_t o[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
  float m = -INFINITY, l = 0.f;

  // loop-invariant LDS offsets inside an image
  int koff[2][4];  // [key half t][d step s & 3]: K row 32t + c32, chunk 2s + hl
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 4; ++s) koff[t][s] = swz_rows(32 * t + c32, 2 * s + hl);
  int vlo[2][2][2], vhi[2][2][2];  // [d tile & 1][key half t][k step s]
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int rk = 32 * t + 16 * s + 4 * hl;
        const int c0 = 32 * dt + ((lane >> 4) & 1) * 16;
        vlo[dt][t][s] = tr_addr(rk, c0, lane);
        vhi[dt][t][s] = tr_addr(rk + 8, c0, lane);
      }

  v8 qf[D / 16];  // Q^T fragments, loaded behind the first tile's DMA (below)

  auto step = [&](int kt, int buf) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nkt) issue(kt + 1, buf ^ 1);
    const int k0 = kt * kAKT;
    if (k0 > wlast) return;  // past this wave's last visible key
    const unsigned char* Kl = lds + buf * BUF;
    const unsigned char* Vl = Kl + NI * IMG;

    f32x16_t x[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int i = 0; i < 16; ++i) x[t][i] = 0.f;
#pragma unroll
      for (int s = 0; s < D / 16; ++s)
        x[t] = mfma32<T>(lds_row8<T>(Kl + (s >> 2) * IMG, koff[t][s & 3]), qf[s], x[t]);
    }
    bool grow;
    float alpha, psum = 0.f;
    if (k0 + kAKT - 1 > wfull) {
      // a tile past the first row's last key (wave-uniform): masked scores in log2 units; a row
      // with no visible key so far keeps m = -inf and exponent offset 0, so p = exp2(-inf) = 0,
      // never exp2(-inf - -inf)
      float tmax = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) {
          const int key = k0 + 32 * t + (rg & 3) + 8 * (rg >> 2) + 4 * hl;
          x[t][rg] = key > lim ? -INFINITY : x[t][rg] * a.scale_log2;
          tmax = fmaxf(tmax, x[t][rg]);
        }
      tmax = max_halves(tmax);
      const float mnew = fmaxf(m, tmax);
      const float msafe = mnew == -INFINITY ? 0.f : mnew;
      grow = __any(mnew != m);
      alpha = grow ? fexp2(m - msafe) : 1.f;
      m = mnew;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) {
          const float p = fexp2(x[t][rg] - msafe);
          psum += p;
          x[t][rg] = p;
        }
    } else {
      // every row of the wave sees every key of the tile: running max on the raw scores, one
      // fma + exp2 per score (the softmax scale is positive)
      float tmax = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) tmax = fmaxf(tmax, x[t][rg]);
      tmax = max_halves(tmax);
      const float mnew = fmaxf(m, tmax * a.scale_log2);
      grow = __any(mnew != m);
      alpha = grow ? fexp2(m - mnew) : 1.f;
      m = mnew;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) {
          const float p = fexp2(fmaf(x[t][rg], a.scale_log2, -mnew));
          psum += p;
          x[t][rg] = p;
        }
    }
    l = l * alpha + psum;
    if (grow) {  // skipped while no row of the wave raised its max (alpha == 1 exactly)
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
    }
    // O^T[d][row] += V^T[d][key] . P^T[key][row]: d tile dt lives in V image dt >> 1
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const v8 pf = acc_frag<T>(x[t], s);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt)
          o[dt] = mfma32<T>(lds_tr8<T>(Vl + (dt >> 1) * IMG, vlo[dt & 1][t][s], vhi[dt & 1][t][s]),
                            pf, o[dt]);
      }
  };

  issue(0, 0);
  // Q^T fragments (B operand of S^T = K . Q^T): d = 16s + 8hl + j.  The empty asm is a use the
  // compiler must wait for HERE, once: left to itself it waits for these loads inside the loop,
  // and its vmcnt(0) there also waits out the tile that was just issued.
#pragma unroll
  for (int s = 0; s < D / 16; ++s) qf[s] = *reinterpret_cast<const v8*>(Q + 16 * s + 8 * hl);
#pragma unroll
  for (int s = 0; s < D / 16; ++s) asm volatile("" : "+v"(qf[s]));
  for (int kt = 0; kt < nkt; ++kt) step(kt, kt & 1);

  if (r >= R) return;
  const float lt = l + __shfl_xor(l, 32);
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
#pragma unroll
  for (int h = 0; h < NI; ++h)
    store_dT<T>(orow + kAD * h, reinterpret_cast<const f32x16_t(&)[2]>(o[2 * h]), hl, inv);
  if (hl == 0) *lrow = lt > 0.f ? m + log2f(lt) : -INFINITY;
}

}  // namespace

void attn_prefill(const AttnPrefill& pp, void* o, float* lse, hipStream_t st) {
  const AttnDecode& p = pp.d;
  if (p.D != 64 && p.D != 128) {
    fprintf(stderr, "attn_prefill: head dim must be 64 or 128, got %d\n", p.D);
    abort();
  }
  if (p.Hkv <= 0 || p.H % p.Hkv != 0) {
    fprintf(stderr, "attn_prefill: %d query heads do not split over %d key/value heads\n", p.H,
            p.Hkv);
    abort();
  }
  if (p.B <= 0 || p.Sq <= 0) return;
  const int64_t R = (int64_t)(p.H / p.Hkv) * p.Sq, tiles = (R + 127) / 128;
  if (p.Hkv > 65535 || p.B > 65535 || tiles > (1 << 23) || tiles * p.Hkv * p.B > 0x7fffffff) {
    fprintf(stderr, "attn_prefill: %lld row tiles x %d key/value heads x batch %d exceed a launch "
                    "grid\n", (long long)tiles, p.Hkv, p.B);
    abort();
  }
  attn_decode_append(p, st);
  PrefillArgs a{};
  a.q = p.q.p; a.qsb = p.q.sb; a.qss = p.q.ss; a.qsh = p.q.sh;
  a.k = p.k.p; a.ksb = p.k.sb; a.kss = p.k.ss; a.ksh = p.k.sh;
  a.v = p.v.p; a.vsb = p.v.sb; a.vss = p.v.ss; a.vsh = p.v.sh;
  a.lens = p.cache_seqlens;
  a.append = p.k_new.p != nullptr ? 1 : 0;
  a.o = o; a.lse = lse;
  a.H = p.H; a.Hkv = p.Hkv; a.G = p.H / p.Hkv; a.Sq = p.Sq; a.Smax = p.Smax; a.R = (int)R;
  a.scale_log2 = p.scale * 1.4426950408889634f;
  const dim3 grid((unsigned)tiles, (unsigned)p.Hkv, (unsigned)p.B), block(kAT);
  if (p.dtype == DType::BF16) {
    if (p.D == 64) hipLaunchKernelGGL((attn_prefill_k<bf16_t, 64>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((attn_prefill_k<bf16_t, 128>), grid, block, 0, st, a);
  } else {
    if (p.D == 64) hipLaunchKernelGGL((attn_prefill_k<half_t, 64>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((attn_prefill_k<half_t, 128>), grid, block, 0, st, a);
  }
}

}  // namespace amd
