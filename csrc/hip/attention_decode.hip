// Fused attention decode step over a KV cache for gfx950 (head dim 64 / 128, bf16 / fp16,
// forward only): the Sq newest tokens of each batch element against the L_b keys of a
// [B, Smax, Hkv, D] cache, split-KV ("flash-decoding").  The training forward (attn_fwd_k)
// gives a workgroup 128 queries of one query head; at Sq = 1 that is 127 padded MFMA columns,
// B * H workgroups however long the cache is, and the K/V head of a group streamed once per
// query head.  A decode step is bound by K/V bytes, so these kernels are laid out for that:
//
// Rows, not queries.  The R = G * Sq rows of one (batch element, key/value head) - the G =
//   H / Hkv query heads of the group times the Sq new tokens, row r = g * Sq + i - are the 32
//   columns of the swapped S^T = K . Q^T MFMA (v_mfma_f32_32x32x16), so K / V of a group are
//   read once for all its query heads.  A lane owns one row's scores (softmax lane-local up to
//   the lane ^ 32 exchange), P.V comes straight from the accumulators, V is read transposed
//   from LDS - the register layouts are those of attn_fwd_k.  R > 32 runs in column blocks of
//   32 (grid.y); rows past R are clamped on load and not stored.
// Waves split keys.  Workgroup = 4 waves; wave w takes slot tiles w, w + 4, ... of the
//   workgroup's key range and keeps its own (m, l, o) in registers.  Each wave owns two LDS
//   slots (K and V images of one slot tile, 16 KiB) filled by global_load_lds and ordered by
//   wave-local s_waitcnt (vmcnt counts a slot's 16 DMA instructions; lgkmcnt(0) before a slot
//   is refilled), so the key loop has no workgroup barrier and all four waves stream at
//   Sq = 1.  A slot tile is 64 keys at D = 64; at D = 128 two 64-key K+V slots per wave
//   (256 KiB) do not fit the CU's 160 KiB, and of {32-key slots, fewer waves, K straight to
//   registers} this file takes 32-KEY SLOTS: the same 16 KiB slot, four streaming waves and one
//   code path (a slot is KS keys x D/64 images; the scores of a slot are KS / 32 accumulators).
//   The four states are merged once at the end through the waves' own (then idle) slots, in
//   wave order.
// Workgroups split the cache.  Grid (nsplit, ceil(R / 32), B * Hkv).  L_b = cache_seqlens[b]
//   (+ Sq after an append), clipped to [0, Smax], is read on the device (no host sync: the call
//   is graph-capture safe); split s owns a contiguous range of the ceil(L_b / 64) 64-key
//   tiles.  An empty range writes lse = -inf (and, unsplit, o = 0) and returns before any DMA
//   or barrier.  The mask is causal, aligned bottom-right: row (g, i) sees keys j <= L_b - Sq
//   + i; only slot tiles that reach past key L_b - Sq test it per element.  Keys at or past
//   L_b are never loaded (their addresses are clamped to row L_b - 1, as the training kernels'
//   tail path does): a cache from torch.empty may hold NaN bit patterns, and 0 * NaN in the
//   P.V MFMA would poison o.  A row that sees no key gets o = 0, lse = -inf.
// Fixed-order combine.  nsplit == 1: the kernel writes the final 16-bit o and the lse.
//   nsplit > 1: each split writes its normalised fp32 partial o and its lse to a workspace and
//   attn_decode_combine_k joins them in split order (max of the lse, exp2 weights, sum, one
//   rounding to 16 bits).  No atomics: results are bitwise reproducible for a given nsplit.
// Append.  attn_decode_append_k copies k_new / v_new [B, Sq, Hkv, D] into cache rows
//   cache_seqlens[b] + i (skipping rows outside [0, Smax)) with plain 16-byte loads and stores,
//   launched before the attention kernel on the same stream.
//
// Resources (hipcc -O3 gfx950 resource report, both dtypes alike): attn_decode_k<D = 64>
// 131072 B LDS, 145 VGPRs + 64 AGPRs; attn_decode_k<D = 128> 131072 B LDS, 180 VGPRs + 80
// AGPRs; no scratch, no spill; occupancy 1 wave per SIMD (one workgroup per CU, set by LDS).
// Timings: docs/PERF.md, "Attention: decode over a KV cache".
#include "attention_common.h"

namespace amd {

namespace {

struct DecodeArgs {
  const void* q;
  const void* k;
  const void* v;
  int64_t qsb, qss, qsh, ksb, kss, ksh, vsb, vss, vsh;  // element strides
  const int* lens;   // [B] keys in the cache before the call
  int append;        // 1: the Sq new rows are in the cache behind lens[b]
  void* o;           // [B][Sq][H][D], written when nsplit == 1
  float* lse;        // [B][H][Sq], written when nsplit == 1
  float* o_part;     // [nsplit][B][Sq][H][D] normalised fp32 partials (nsplit > 1)
  float* lse_part;   // [nsplit][B][H][Sq]
  int B, H, Hkv, G, Sq, Smax, R;  // R = G * Sq rows per (b, key/value head)
  float scale_log2;
};

// the visible length of batch element b: clipped to the rows the cache views hold
__device__ __forceinline__ int decode_len(const int* lens, int b, int append, int Sq, int Smax) {
  int l = lens[b];
  l = l < 0 ? 0 : (l > Smax ? Smax : l);
  l += append ? Sq : 0;
  return l > Smax ? Smax : l;
}

template <typename T, int D>
__global__ void __launch_bounds__(kAT) attn_decode_k(DecodeArgs a) {
  typedef typename Frag<T>::v8 v8;
  constexpr int NI = D / kAD;            // 64-wide LDS images per K (or V) slot tile
  constexpr int KS = kAKT / NI;          // keys per slot tile: 64 (D = 64), 32 (D = 128)
  constexpr int NT = KS / 32;            // score accumulators per slot tile
  constexpr int IMG = KS * kARow;        // bytes of one image
  constexpr int SLOT = 2 * NI * IMG;     // K and V of one slot tile: 16 KiB
  constexpr int NDMA = 2 * NI * KS / 8;  // DMA instructions per slot tile: 16
  static_assert(SLOT == 16384 && NDMA == 16, "the s_waitcnt vmcnt(16) below counts one slot");
  constexpr int WAVE = 2 * SLOT;         // a wave's two slots
  static_assert(WAVE >= (D * 32 + 64) * 4, "a wave's merge state fits its own slots");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[4 * WAVE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hl = lane >> 5, c32 = lane & 31;
  const int split = blockIdx.x, nsplit = gridDim.x;
  const int b = blockIdx.z / a.Hkv, hk = blockIdx.z - b * a.Hkv;
  const int Sq = a.Sq, R = a.R;
  const int L = decode_len(a.lens, b, a.append, Sq, a.Smax);

  // this split's 64-key tiles [tb, te) of the ceil(L / 64)
  const int ntile = (L + kAKT - 1) / kAKT;
  const int per = (ntile + nsplit - 1) / nsplit;
  const int tb = split * per;
  const int te = tb + per < ntile ? tb + per : ntile;

  // the row (query head g of the group, new token i) a thread stores in the epilogue
  const int er = blockIdx.y * 32 + (tid & 31);
  const int eg = er / Sq, ei = er - eg * Sq, eh = hk * a.G + eg;
  const int64_t lrow = (((int64_t)split * a.B + b) * a.H + eh) * Sq + ei;  // lse_part row
  constexpr int DG = D / 8;  // d columns per thread in the epilogue
  const int d0 = (tid >> 5) * DG;

  if (tb >= te) {  // nothing to read: before any DMA or barrier
    if (er < R) {
      if (nsplit > 1) {
        if (d0 == 0) a.lse_part[lrow] = -INFINITY;
      } else {
        T* orow = static_cast<T*>(a.o) + (((int64_t)b * Sq + ei) * a.H + eh) * D + d0;
#pragma unroll
        for (int j = 0; j < DG; j += 8) *reinterpret_cast<uint4*>(orow + j) = uint4{0, 0, 0, 0};
        if (d0 == 0) a.lse[((int64_t)b * a.H + eh) * Sq + ei] = -INFINITY;
      }
    }
    return;
  }

  // this lane's row in the key loop (clamped: rows past R repeat row R - 1, never stored)
  const int r = blockIdx.y * 32 + c32;
  const int rr = r < R ? r : R - 1;
  const int g = rr / Sq, qi = rr - g * Sq;
  const int lim = L - Sq + qi;  // the last key this row sees
  const T* Q = static_cast<const T*>(a.q) + b * a.qsb + (int64_t)qi * a.qss + (hk * a.G + g) * a.qsh;
  const T* K = static_cast<const T*>(a.k) + b * a.ksb + hk * a.ksh;
  const T* V = static_cast<const T*>(a.v) + b * a.vsb + hk * a.vsh;

  v8 qf[D / 16];  // Q^T fragments, loaded behind the first slot's DMA (below)

  // DMA: one instruction fills 8 rows of one image; lane = (row in the 8, physical chunk)
  const int drow = lane >> 3, pch = lane & 7;
  uint32_t kof[NI][KS / 8], vof[NI][KS / 8];
#pragma unroll
  for (int h = 0; h < NI; ++h)
#pragma unroll
    for (int i = 0; i < KS / 8; ++i) {
      const int row = 8 * i + drow;
      kof[h][i] = row_off<T>(row, a.kss, 8 * h + ((swz_rows(row, pch) - row * kARow) >> 4));
      vof[h][i] = row_off<T>(row, a.vss, 8 * h + ((swz_tr(row, pch) - row * kARow) >> 4));
    }
  unsigned char* const wlds = lds + wid * WAVE;
  auto issue = [&](int k0, int slot) {  // keys k0 .. k0 + KS - 1 -> slot
    unsigned char* Kl = wlds + slot * SLOT;
    unsigned char* Vl = Kl + NI * IMG;
    if (k0 + KS <= L) {
      const T* kb = tile_base(K, k0, a.kss);
      const T* vb = tile_base(V, k0, a.vss);
#pragma unroll
      for (int h = 0; h < NI; ++h)
#pragma unroll
        for (int i = 0; i < KS / 8; ++i) {
          glds16o(kb, kof[h][i], Kl + h * IMG + i * 1024);
          glds16o(vb, vof[h][i], Vl + h * IMG + i * 1024);
        }
      return;
    }
    // the tile reaches past L: rows at or past L read row L - 1 (L >= 1 here)
#pragma unroll
    for (int h = 0; h < NI; ++h)
#pragma unroll
      for (int i = 0; i < KS / 8; ++i) {
        const int row = 8 * i + drow;
        const int key = k0 + row;
        const int kk = key < L ? key : L - 1;
        const int chk = 8 * h + ((swz_rows(row, pch) - row * kARow) >> 4);
        const int chv = 8 * h + ((swz_tr(row, pch) - row * kARow) >> 4);
        glds16(K + (int64_t)kk * a.kss + chk * 8, Kl + h * IMG + i * 1024);
        glds16(V + (int64_t)kk * a.vss + chv * 8, Vl + h * IMG + i * 1024);
      }
  };

  f32x16_t o[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
  float m = -INFINITY, l = 0.f;

  // loop-invariant LDS offsets
  int koff[NT][D / 16];  // [key half t][d step s]: image s / 4, K row 32t + c32, chunk 2(s % 4) + hl
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int s = 0; s < D / 16; ++s)
      koff[t][s] = (s >> 2) * IMG + swz_rows(32 * t + c32, 2 * (s & 3) + hl);
  int vlo[D / 32][NT][2], vhi[D / 32][NT][2];  // [d tile][key half t][k step s]
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int r0 = 32 * t + 16 * s + 4 * hl;
        const int c0 = 32 * (dt & 1) + ((lane >> 4) & 1) * 16;
        vlo[dt][t][s] = (dt >> 1) * IMG + tr_addr(r0, c0, lane);
        vhi[dt][t][s] = (dt >> 1) * IMG + tr_addr(r0 + 8, c0, lane);
      }

  auto step = [&](int k0, int slot) {
    const unsigned char* Kl = wlds + slot * SLOT;
    const unsigned char* Vl = Kl + NI * IMG;
    f32x16_t x[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int i = 0; i < 16; ++i) x[t][i] = 0.f;
#pragma unroll
      for (int s = 0; s < D / 16; ++s) x[t] = mfma32<T>(lds_row8<T>(Kl, koff[t][s]), qf[s], x[t]);
    }
    // scores in log2 units; only a tile that reaches past key L - Sq (the first row's last
    // key; keys >= L lie past every row's) tests the mask (wave-uniform)
    const bool need_mask = k0 + KS - 1 > L - Sq;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) {
        const int key = k0 + 32 * t + (rg & 3) + 8 * (rg >> 2) + 4 * hl;
        x[t][rg] = need_mask && key > lim ? -INFINITY : x[t][rg] * a.scale_log2;
      }
    float tmax = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) tmax = fmaxf(tmax, x[t][rg]);
    tmax = max_halves(tmax);
    // a row with no visible key so far keeps m = -inf: its exponent offset is 0 instead, so
    // p = exp2(-inf) = 0, never exp2(-inf - -inf)
    const float mnew = fmaxf(m, tmax);
    const float msafe = mnew == -INFINITY ? 0.f : mnew;
    const bool grow = __any(mnew != m);
    const float alpha = grow ? fexp2(m - msafe) : 1.f;
    m = mnew;
    float psum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) {
        const float p = fexp2(x[t][rg] - msafe);
        psum += p;
        x[t][rg] = p;
      }
    l = l * alpha + psum;
    if (grow) {
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
    }
    // O^T[d][row] += V^T[d][key] . P^T[key][row]
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const v8 pf = acc_frag<T>(x[t], s);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt)
          o[dt] = mfma32<T>(lds_tr8<T>(Vl, vlo[dt][t][s], vhi[dt][t][s]), pf, o[dt]);
      }
  };

  // this wave's slot tiles: k0 = kbeg + (wid + 4 n) KS below kend, double buffered; a slot's
  // 16 DMA instructions retire in order, so vmcnt(16) is "the older slot has landed"
  const int kbeg = tb * kAKT;
  const int kend = te * kAKT < L ? te * kAKT : L;
  int k0 = kbeg + wid * KS;
  if (k0 < kend) issue(k0, 0);
  // Q^T fragments (B operand of S^T = K . Q^T): d = 16s + 8hl + j.  The empty asm is a use the
  // compiler must wait for HERE, once: left to itself it waits for these loads inside the
  // loop, and its vmcnt(0) there also waits out the slot that was just issued.
#pragma unroll
  for (int s = 0; s < D / 16; ++s) qf[s] = *reinterpret_cast<const v8*>(Q + 16 * s + 8 * hl);
#pragma unroll
  for (int s = 0; s < D / 16; ++s) asm volatile("" : "+v"(qf[s]));
  for (int slot = 0; k0 < kend; k0 += 4 * KS, slot ^= 1) {
    if (k0 + 4 * KS < kend) {
      issue(k0 + 4 * KS, slot ^ 1);
      asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    step(k0, slot);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slot's reads, before its refill
  }

  // the wave's state into its own slots: O [D][32 rows] fp32, then m [32] and l [32]
  {
    float* Ow = reinterpret_cast<float*>(wlds);
    const float lt = l + __shfl_xor(l, 32);
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i)
        Ow[(32 * dt + 8 * (i >> 2) + 4 * hl + (i & 3)) * 32 + c32] = o[dt][i];
    if (hl == 0) {
      Ow[D * 32 + c32] = m;
      Ow[D * 32 + 32 + c32] = lt;
    }
  }
  __syncthreads();

  // merge in wave order: thread = (row tid % 32, DG columns from d0)
  const int col = tid & 31;
  float mw[4], mt = -INFINITY;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    mw[w] = reinterpret_cast<const float*>(lds + w * WAVE)[D * 32 + col];
    mt = fmaxf(mt, mw[w]);
  }
  const float msafe = mt == -INFINITY ? 0.f : mt;
  float lt = 0.f, acc[DG];
#pragma unroll
  for (int j = 0; j < DG; ++j) acc[j] = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float* Ow = reinterpret_cast<const float*>(lds + w * WAVE);
    const float wgt = fexp2(mw[w] - msafe);
    lt += wgt * Ow[D * 32 + 32 + col];
#pragma unroll
    for (int j = 0; j < DG; ++j) acc[j] += wgt * Ow[(d0 + j) * 32 + col];
  }
  if (er >= R) return;
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
  const float lse = lt > 0.f ? mt + log2f(lt) : -INFINITY;
  if (nsplit > 1) {
    float* orow = a.o_part + ((((int64_t)split * a.B + b) * Sq + ei) * a.H + eh) * D + d0;
#pragma unroll
    for (int j = 0; j < DG; j += 4)
      *reinterpret_cast<float4*>(orow + j) =
          float4{acc[j] * inv, acc[j + 1] * inv, acc[j + 2] * inv, acc[j + 3] * inv};
    if (d0 == 0) a.lse_part[lrow] = lse;
  } else {
    T* orow = static_cast<T*>(a.o) + (((int64_t)b * Sq + ei) * a.H + eh) * D + d0;
#pragma unroll
    for (int j = 0; j < DG; j += 8) {
      uint4 w;
      w.x = pack2<T>(acc[j] * inv, acc[j + 1] * inv);
      w.y = pack2<T>(acc[j + 2] * inv, acc[j + 3] * inv);
      w.z = pack2<T>(acc[j + 4] * inv, acc[j + 5] * inv);
      w.w = pack2<T>(acc[j + 6] * inv, acc[j + 7] * inv);
      *reinterpret_cast<uint4*>(orow + j) = w;
    }
    if (d0 == 0) a.lse[((int64_t)b * a.H + eh) * Sq + ei] = lse;
  }
}

// nsplit > 1: one thread per (b, i, h) row and four d columns joins the splits' partials in
// split order.  A split with lse = -inf (an empty range: its o was never written) is skipped.
template <typename T, int D>
__global__ void __launch_bounds__(256) attn_decode_combine_k(DecodeArgs a, int nsplit) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t rows = (int64_t)a.B * a.Sq * a.H;
  const int64_t row = id / (D / 4);  // (b * Sq + i) * H + h
  if (row >= rows) return;
  const int d = (int)(id - row * (D / 4)) * 4;
  const int h = (int)(row % a.H);
  const int64_t bi = row / a.H;
  const int i = (int)(bi % a.Sq), b = (int)(bi / a.Sq);
  const int64_t lrow = ((int64_t)b * a.H + h) * a.Sq + i, lstep = (int64_t)a.B * a.H * a.Sq;
  float mx = -INFINITY;
  for (int s = 0; s < nsplit; ++s) mx = fmaxf(mx, a.lse_part[s * lstep + lrow]);
  float sum = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (mx != -INFINITY) {
    for (int s = 0; s < nsplit; ++s) {
      const float ls = a.lse_part[s * lstep + lrow];
      if (ls == -INFINITY) continue;
      const float w = fexp2(ls - mx);
      const float4 p = *reinterpret_cast<const float4*>(a.o_part + (s * rows + row) * D + d);
      sum += w;
      acc[0] += w * p.x; acc[1] += w * p.y; acc[2] += w * p.z; acc[3] += w * p.w;
    }
  }
  const float inv = sum > 0.f ? 1.f / sum : 0.f;
  uint2 w;
  w.x = pack2<T>(acc[0] * inv, acc[1] * inv);
  w.y = pack2<T>(acc[2] * inv, acc[3] * inv);
  *reinterpret_cast<uint2*>(static_cast<T*>(a.o) + row * D + d) = w;
  if (d == 0) a.lse[lrow] = sum > 0.f ? mx + log2f(sum) : -INFINITY;
}

struct AppendArgs {
  const void* kn;
  const void* vn;
  void* kc;
  void* vc;
  int64_t knsb, knss, knsh, vnsb, vnss, vnsh, kcsb, kcss, kcsh, vcsb, vcss, vcsh;
  const int* lens;
  int B, Sq, Hkv, Smax;
};

// one thread per 16 bytes of a new K and V row: k_new[b][i][h] -> k_cache[b][lens[b] + i][h]
template <int D>
__global__ void __launch_bounds__(256) attn_decode_append_k(AppendArgs a) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = id / (D / 8);  // (b * Sq + i) * Hkv + h
  if (row >= (int64_t)a.B * a.Sq * a.Hkv) return;
  const int c = (int)(id - row * (D / 8)) * 8;  // 16-bit elements
  const int h = (int)(row % a.Hkv);
  const int64_t bi = row / a.Hkv;
  const int i = (int)(bi % a.Sq), b = (int)(bi / a.Sq);
  const int len = a.lens[b];
  if (len < 0 || len >= a.Smax - i) return;  // the row lies outside the cache views
  const int pos = len + i;
  const unsigned short* kn = static_cast<const unsigned short*>(a.kn);
  const unsigned short* vn = static_cast<const unsigned short*>(a.vn);
  unsigned short* kc = static_cast<unsigned short*>(a.kc);
  unsigned short* vc = static_cast<unsigned short*>(a.vc);
  *reinterpret_cast<uint4*>(kc + b * a.kcsb + (int64_t)pos * a.kcss + h * a.kcsh + c) =
      *reinterpret_cast<const uint4*>(kn + b * a.knsb + i * a.knss + h * a.knsh + c);
  *reinterpret_cast<uint4*>(vc + b * a.vcsb + (int64_t)pos * a.vcss + h * a.vcsh + c) =
      *reinterpret_cast<const uint4*>(vn + b * a.vnsb + i * a.vnss + h * a.vnsh + c);
}

template <typename T, int D>
void launch_decode(const AttnDecode& p, const DecodeArgs& a, hipStream_t st) {
  const int nyb = (a.R + 31) / 32;
  dim3 grid((unsigned)p.nsplit, (unsigned)nyb, (unsigned)(p.B * p.Hkv)), block(kAT);
  hipLaunchKernelGGL((attn_decode_k<T, D>), grid, block, 0, st, a);
  if (p.nsplit > 1) {
    const int64_t threads = (int64_t)p.B * p.Sq * p.H * (D / 4);
    hipLaunchKernelGGL((attn_decode_combine_k<T, D>), dim3((unsigned)((threads + 255) / 256)),
                       dim3(256), 0, st, a, p.nsplit);
  }
}

}  // namespace

int attn_decode_splits(int B, int Hkv, int R, int Smax, int num_cus) {
  const int64_t base = (int64_t)B * Hkv * ((R + 31) / 32);  // workgroups of one split
  if (base <= 0 || num_cus <= 0) return 1;
  int64_t n = (2 * (int64_t)num_cus + base - 1) / base;     // about two workgroups per CU
  const int64_t by_tiles = ((Smax + kAKT - 1) / kAKT) / 4;  // ... of at least four tiles each
  n = n < by_tiles ? n : by_tiles;
  n = n < kAttnDecodeMaxSplits ? n : kAttnDecodeMaxSplits;
  return n < 1 ? 1 : (int)n;
}

// attn_decode_combine_k on its own, for the paged kernels (attention_decode_paged.hip), whose
// splits write the same workspace
void attn_decode_combine(DType dtype, int D, int B, int H, int Sq, int nsplit, float* o_part,
                         float* lse_part, void* o, float* lse, hipStream_t st) {
  DecodeArgs a{};
  a.o = o; a.lse = lse; a.o_part = o_part; a.lse_part = lse_part;
  a.B = B; a.H = H; a.Sq = Sq;
  const int64_t threads = (int64_t)B * Sq * H * (D / 4);
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  if (dtype == DType::BF16) {
    if (D == 64) hipLaunchKernelGGL((attn_decode_combine_k<bf16_t, 64>), grid, block, 0, st, a, nsplit);
    else hipLaunchKernelGGL((attn_decode_combine_k<bf16_t, 128>), grid, block, 0, st, a, nsplit);
  } else {
    if (D == 64) hipLaunchKernelGGL((attn_decode_combine_k<half_t, 64>), grid, block, 0, st, a, nsplit);
    else hipLaunchKernelGGL((attn_decode_combine_k<half_t, 128>), grid, block, 0, st, a, nsplit);
  }
}

// attn_decode_append_k on its own: p.k_new / p.v_new (none: nothing is launched) to cache rows
// cache_seqlens[b] + i, for attn_decode below and the prefill kernels (attention_prefill.hip)
void attn_decode_append(const AttnDecode& p, hipStream_t st) {
  if (p.k_new.p == nullptr) return;
  AppendArgs c{};
  c.kn = p.k_new.p; c.knsb = p.k_new.sb; c.knss = p.k_new.ss; c.knsh = p.k_new.sh;
  c.vn = p.v_new.p; c.vnsb = p.v_new.sb; c.vnss = p.v_new.ss; c.vnsh = p.v_new.sh;
  c.kc = p.k.p; c.kcsb = p.k.sb; c.kcss = p.k.ss; c.kcsh = p.k.sh;
  c.vc = p.v.p; c.vcsb = p.v.sb; c.vcss = p.v.ss; c.vcsh = p.v.sh;
  c.lens = p.cache_seqlens;
  c.B = p.B; c.Sq = p.Sq; c.Hkv = p.Hkv; c.Smax = p.Smax;
  const int64_t threads = (int64_t)p.B * p.Sq * p.Hkv * (p.D / 8);
  dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  if (p.D == 64) hipLaunchKernelGGL((attn_decode_append_k<64>), grid, block, 0, st, c);
  else hipLaunchKernelGGL((attn_decode_append_k<128>), grid, block, 0, st, c);
}

void attn_decode(const AttnDecode& p, void* o, float* lse, hipStream_t st) {
  if (p.D != 64 && p.D != 128) {
    fprintf(stderr, "attn_decode: head dim must be 64 or 128, got %d\n", p.D);
    abort();
  }
  if (p.Hkv <= 0 || p.H % p.Hkv != 0) {
    fprintf(stderr, "attn_decode: %d query heads do not split over %d key/value heads\n", p.H,
            p.Hkv);
    abort();
  }
  if (p.nsplit < 1 || p.nsplit > kAttnDecodeMaxSplits ||
      (p.nsplit > 1 && (p.o_part == nullptr || p.lse_part == nullptr))) {
    fprintf(stderr, "attn_decode: nsplit = %d needs 1 .. %d and, above 1, the workspace\n",
            p.nsplit, kAttnDecodeMaxSplits);
    abort();
  }
  if (p.B <= 0 || p.Sq <= 0) return;
  attn_decode_append(p, st);
  DecodeArgs a{};
  a.q = p.q.p; a.qsb = p.q.sb; a.qss = p.q.ss; a.qsh = p.q.sh;
  a.k = p.k.p; a.ksb = p.k.sb; a.kss = p.k.ss; a.ksh = p.k.sh;
  a.v = p.v.p; a.vsb = p.v.sb; a.vss = p.v.ss; a.vsh = p.v.sh;
  a.lens = p.cache_seqlens;
  a.append = p.k_new.p != nullptr ? 1 : 0;
  a.o = o; a.lse = lse; a.o_part = p.o_part; a.lse_part = p.lse_part;
  a.B = p.B; a.H = p.H; a.Hkv = p.Hkv; a.G = p.H / p.Hkv; a.Sq = p.Sq; a.Smax = p.Smax;
  a.R = a.G * p.Sq;
  a.scale_log2 = p.scale * 1.4426950408889634f;
  if (p.dtype == DType::BF16) {
    if (p.D == 64) launch_decode<bf16_t, 64>(p, a, st);
    else launch_decode<bf16_t, 128>(p, a, st);
  } else {
    if (p.D == 64) launch_decode<half_t, 64>(p, a, st);
    else launch_decode<half_t, 128>(p, a, st);
  }
}

}  // namespace amd
