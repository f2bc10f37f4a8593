// Fused attention decode step over a PAGED KV cache for gfx950 (head dim 64 / 128, bf16 /
// fp16, forward only): the decode step of attention_decode.hip with the keys of batch element
// b held in fixed-size pages of one pool instead of a [Smax, Hkv, D] slab.  k_pages / v_pages
// are [num_pages, P, Hkv, D] views (any page / row / head strides: the halves of one packed
// [num_pages, P, 2, Hkv, D] pool), block_table is int32 [B, max_pages], key j of element b is
// row j % P of page block_table[b][j / P], P a power of two in 16 .. 256, Smax = max_pages * P.
//
// The work split, the math and the merge are those of attn_decode_k, statement for statement
// (rows = the G * Sq rows of a group as MFMA columns, four waves over per-wave LDS slots of KS
// keys, nsplit workgroups over 64-key tiles, the fixed-order join by attn_decode_combine_k),
// so for a given nsplit the result is bitwise that of the contiguous call on the same keys.
// What differs is where a slot tile's rows come from:
//
// Block-table walk in SGPRs, one tile ahead.  The page ids of a slot tile are wave-uniform and
//   read by scalar loads; issue(k0) forms its page bases from the ids fetched one tile earlier
//   and then, before its own 16 DMA instructions, starts the scalar loads for the tile this
//   wave issues next (k0 + 4 KS).  Those land under the DMA issue and the MFMA step; the loop's
//   s_waitcnt lgkmcnt(0) orders them.  No vector load stands in the key loop, so vmcnt(16)
//   still counts exactly one slot.
// Pages per tile.  PPT = KS / P pages make one slot tile (1 when P >= KS; 2 or 4 below: P = 16
//   / 32 at D = 64, P = 16 at D = 128).  A DMA instruction fills 8 rows, which lie in one page:
//   the page of instruction i is the compile-time (8 i) / P, its base one SGPR pair (page id *
//   page stride, 64-bit; at PPT = 1 plus the tile's first row in its page), the per-lane
//   32-bit offset (row % P) * row stride + swizzled chunk, loop-invariant as before.
// The tail tile (reaches past L) clamps twice: the page of sub-page j is the one that holds key
//   min(k0 + j P, L - 1) - table entries at or past ceil(L / P) are unallocated and never read,
//   nor is the table read past column max_pages - 1 - and each lane's row is min(key, L - 1)
//   % P of that page, which is key L - 1 wherever the key lies at or past L.
// A bad table: every page id is clamped to [0, num_pages - 1] (two scalar ops), as
//   cache_seqlens is clipped: wrong numbers, never an access outside the pool.
// Append.  attn_decode_paged_append_k writes k_new / v_new [B, Sn, Hkv, D] (any Sn: a prompt at
//   prefill) to row (len_b + i) % P of page table[b][(len_b + i) / P], skipping rows outside
//   [0, Smax), one thread per 16 bytes.
//
// Resources (hipcc -O3 gfx950 resource report): docs/PERF.md, "Attention: decode over a paged
// KV cache"; 131072 B LDS, no scratch, no spill in every instantiation.
#include "attention_common.h"

namespace amd {

namespace {

struct PagedArgs {
  const void* q;
  const void* k;  // page pools
  const void* v;
  int64_t qsb, qss, qsh, ksp, kss, ksh, vsp, vss, vsh;  // element strides (sp: page)
  const int* lens;   // [B] keys held before the call
  const int* table;  // [B][max_pages] page ids
  int append;        // 1: the Sq new rows are in the pages behind lens[b]
  void* o;           // [B][Sq][H][D], written when nsplit == 1
  float* lse;        // [B][H][Sq], written when nsplit == 1
  float* o_part;     // [nsplit][B][Sq][H][D] normalised fp32 partials (nsplit > 1)
  float* lse_part;   // [nsplit][B][H][Sq]
  int B, H, Hkv, G, Sq, Smax, R;  // Smax = max_pages << lp; R = G * Sq rows per (b, kv head)
  int num_pages, max_pages, lp;   // lp = log2 P
  float scale_log2;
};

// attention_decode.hip's decode_len: the visible length, clipped to the rows the table spans
__device__ __forceinline__ int paged_len(const int* lens, int b, int append, int Sq, int Smax) {
  int l = lens[b];
  l = l < 0 ? 0 : (l > Smax ? Smax : l);
  l += append ? Sq : 0;
  return l > Smax ? Smax : l;
}

__device__ __forceinline__ int clamp_page(int id, int num_pages) {
  return id < 0 ? 0 : (id < num_pages ? id : num_pages - 1);
}

constexpr int ilog2(int x) { return x <= 1 ? 0 : 1 + ilog2(x >> 1); }

template <typename T, int D, int PPT>
__global__ void __launch_bounds__(kAT) attn_decode_paged_k(PagedArgs a) {
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
  static_assert(PPT == 1 || (KS / PPT >= 16 && KS % PPT == 0), "pages of 16 rows or more");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[4 * WAVE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hl = lane >> 5, c32 = lane & 31;
  const int split = blockIdx.x, nsplit = gridDim.x;
  const int b = blockIdx.z / a.Hkv, hk = blockIdx.z - b * a.Hkv;
  const int Sq = a.Sq, R = a.R;
  const int L = paged_len(a.lens, b, a.append, Sq, a.Smax);

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

  if (tb >= te) {  // nothing to read: before any table load, DMA or barrier
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
  const T* K = static_cast<const T*>(a.k) + hk * a.ksh;  // this head's row 0 of page 0
  const T* V = static_cast<const T*>(a.v) + hk * a.vsh;

  v8 qf[D / 16];  // Q^T fragments, loaded behind the first slot's DMA (below)

  // pages: P = 1 << lp rows; below a slot tile's KS keys P is the compile-time KS / PPT
  const int lp = PPT == 1 ? a.lp : ilog2(KS / PPT);
  const int pmask = (1 << lp) - 1;
  // The table row through the constant address space: no launch writes the table while this
  // kernel runs, and only that promise lets the compiler read it with scalar loads behind the
  // loop's memory-clobbering asm (a plain global pointer gave global_load_dword + vmcnt(0) +
  // v_readfirstlane per id, inside the loop).
  typedef const __attribute__((address_space(4))) int* table_ptr;
  const table_ptr tab = (table_ptr)(a.table + (int64_t)b * a.max_pages);
  // the table's entry for the page that holds key min(key, L - 1): one scalar load (L >= 1
  // here).  fetch() only starts the loads; the ids are clamped where issue() uses them, so
  // nothing waits for a table load before the tile that needs it is issued.
  int idn[PPT];  // the (unclamped) pages of the slot tile this wave issues next
  auto fetch = [&](int k0) {
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int key = k0 + j * (KS / PPT);
      idn[j] = tab[(key < L ? key : L - 1) >> lp];
    }
  };

  // DMA: one instruction fills 8 rows of one image; lane = (row in the 8, physical chunk);
  // rows 8 i .. 8 i + 7 of a slot tile lie in its page (8 i) >> lp, at row % P
  const int drow = lane >> 3, pch = lane & 7;
  uint32_t kof[NI][KS / 8], vof[NI][KS / 8];
#pragma unroll
  for (int h = 0; h < NI; ++h)
#pragma unroll
    for (int i = 0; i < KS / 8; ++i) {
      const int row = 8 * i + drow;
      const int prow = PPT == 1 ? row : (row & pmask);
      kof[h][i] = row_off<T>(prow, a.kss, 8 * h + ((swz_rows(row, pch) - row * kARow) >> 4));
      vof[h][i] = row_off<T>(prow, a.vss, 8 * h + ((swz_tr(row, pch) - row * kARow) >> 4));
    }
  unsigned char* const wlds = lds + wid * WAVE;
  auto issue = [&](int k0, int slot) {  // keys k0 .. k0 + KS - 1 -> slot; idn holds its pages
    unsigned char* Kl = wlds + slot * SLOT;
    unsigned char* Vl = Kl + NI * IMG;
    const T* kb[PPT];
    const T* vb[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int64_t id = clamp_page(idn[j], a.num_pages);
      kb[j] = K + id * a.ksp;
      vb[j] = V + id * a.vsp;
    }
    fetch(k0 + 4 * KS);  // the next tile's ids travel under this tile's DMA issue and step
    if (k0 + KS <= L) {
      if constexpr (PPT == 1) {  // the tile's first row in its page
        kb[0] = tile_base(kb[0], k0 & pmask, a.kss);
        vb[0] = tile_base(vb[0], k0 & pmask, a.vss);
      }
#pragma unroll
      for (int h = 0; h < NI; ++h)
#pragma unroll
        for (int i = 0; i < KS / 8; ++i) {
          constexpr int PR8 = KS / PPT / 8;  // DMA instructions per page (PPT > 1)
          const int j = PPT == 1 ? 0 : i / PR8;
          glds16o(kb[j], kof[h][i], Kl + h * IMG + i * 1024);
          glds16o(vb[j], vof[h][i], Vl + h * IMG + i * 1024);
        }
      return;
    }
    // the tile reaches past L: rows at or past L read key L - 1 (L >= 1 here), which lies in
    // sub-page j's clamped page whenever one of j's rows does
#pragma unroll
    for (int h = 0; h < NI; ++h)
#pragma unroll
      for (int i = 0; i < KS / 8; ++i) {
        constexpr int PR8 = KS / PPT / 8;
        const int j = PPT == 1 ? 0 : i / PR8;
        const int row = 8 * i + drow;
        const int key = k0 + row;
        const int kk = (key < L ? key : L - 1) & pmask;
        const int chk = 8 * h + ((swz_rows(row, pch) - row * kARow) >> 4);
        const int chv = 8 * h + ((swz_tr(row, pch) - row * kARow) >> 4);
        glds16o(kb[j], row_off<T>(kk, a.kss, chk), Kl + h * IMG + i * 1024);
        glds16o(vb[j], row_off<T>(kk, a.vss, chv), Vl + h * IMG + i * 1024);
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

  // one slot tile of scores, online softmax and P.V: attn_decode_k's step, unchanged
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
  if (k0 < kend) {
    fetch(k0);  // the only table load a DMA issue waits for
    issue(k0, 0);
  }
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

struct PagedAppendArgs {
  const void* kn;
  const void* vn;
  void* kp;
  void* vp;
  int64_t knsb, knss, knsh, vnsb, vnss, vnsh, kpsp, kpss, kpsh, vpsp, vpss, vpsh;
  const int* lens;
  const int* table;
  int B, Sn, Hkv, Smax, num_pages, max_pages, lp;
};

// one thread per 16 bytes of a new K and V row: k_new[b][i][h] -> row (lens[b] + i) % P of page
// table[b][(lens[b] + i) / P]
template <int D>
__global__ void __launch_bounds__(256) attn_decode_paged_append_k(PagedAppendArgs a) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = id / (D / 8);  // (b * Sn + i) * Hkv + h
  if (row >= (int64_t)a.B * a.Sn * a.Hkv) return;
  const int c = (int)(id - row * (D / 8)) * 8;  // 16-bit elements
  const int h = (int)(row % a.Hkv);
  const int64_t bi = row / a.Hkv;
  const int i = (int)(bi % a.Sn), b = (int)(bi / a.Sn);
  const int len = a.lens[b];
  if (len < 0 || len >= a.Smax - i) return;  // the row lies outside the table's pages
  const int pos = len + i;
  const int64_t page = clamp_page(a.table[(int64_t)b * a.max_pages + (pos >> a.lp)], a.num_pages);
  const int prow = pos & ((1 << a.lp) - 1);
  const unsigned short* kn = static_cast<const unsigned short*>(a.kn);
  const unsigned short* vn = static_cast<const unsigned short*>(a.vn);
  unsigned short* kp = static_cast<unsigned short*>(a.kp);
  unsigned short* vp = static_cast<unsigned short*>(a.vp);
  *reinterpret_cast<uint4*>(kp + page * a.kpsp + (int64_t)prow * a.kpss + h * a.kpsh + c) =
      *reinterpret_cast<const uint4*>(kn + b * a.knsb + i * a.knss + h * a.knsh + c);
  *reinterpret_cast<uint4*>(vp + page * a.vpsp + (int64_t)prow * a.vpss + h * a.vpsh + c) =
      *reinterpret_cast<const uint4*>(vn + b * a.vnsb + i * a.vnss + h * a.vnsh + c);
}

template <typename T, int D>
void launch_paged(const AttnDecodePaged& p, const PagedArgs& a, hipStream_t st) {
  constexpr int KS = kAKT / (D / kAD);
  const int nyb = (a.R + 31) / 32;
  dim3 grid((unsigned)p.d.nsplit, (unsigned)nyb, (unsigned)(a.B * a.Hkv)), block(kAT);
  const int P = 1 << a.lp;
  if (P >= KS) hipLaunchKernelGGL((attn_decode_paged_k<T, D, 1>), grid, block, 0, st, a);
  else if (2 * P == KS) hipLaunchKernelGGL((attn_decode_paged_k<T, D, 2>), grid, block, 0, st, a);
  else if constexpr (KS == 64)
    hipLaunchKernelGGL((attn_decode_paged_k<T, D, 4>), grid, block, 0, st, a);
}

bool page_size_ok(int lp) { return lp >= 4 && lp <= 8; }

}  // namespace

void attn_paged_append(const AttnDecodePaged& p, int Sn, hipStream_t st) {
  const AttnDecode& d = p.d;
  if ((d.D != 64 && d.D != 128) || !page_size_ok(p.log2_page) || p.num_pages <= 0 ||
      p.max_pages <= 0 || d.k_new.p == nullptr || d.v_new.p == nullptr) {
    fprintf(stderr, "attn_paged_append: head dim 64 or 128, pages of 16 .. 256 rows, a pool, a "
                    "table and both new tensors, got D = %d, log2 P = %d\n", d.D, p.log2_page);
    abort();
  }
  if (d.B <= 0 || Sn <= 0 || d.Hkv <= 0) return;
  PagedAppendArgs c{};
  c.kn = d.k_new.p; c.knsb = d.k_new.sb; c.knss = d.k_new.ss; c.knsh = d.k_new.sh;
  c.vn = d.v_new.p; c.vnsb = d.v_new.sb; c.vnss = d.v_new.ss; c.vnsh = d.v_new.sh;
  c.kp = d.k.p; c.kpsp = d.k.sb; c.kpss = d.k.ss; c.kpsh = d.k.sh;
  c.vp = d.v.p; c.vpsp = d.v.sb; c.vpss = d.v.ss; c.vpsh = d.v.sh;
  c.lens = d.cache_seqlens;
  c.table = p.block_table;
  c.B = d.B; c.Sn = Sn; c.Hkv = d.Hkv; c.Smax = p.max_pages << p.log2_page;
  c.num_pages = p.num_pages; c.max_pages = p.max_pages; c.lp = p.log2_page;
  const int64_t threads = (int64_t)d.B * Sn * d.Hkv * (d.D / 8);
  dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  if (d.D == 64) hipLaunchKernelGGL((attn_decode_paged_append_k<64>), grid, block, 0, st, c);
  else hipLaunchKernelGGL((attn_decode_paged_append_k<128>), grid, block, 0, st, c);
}

void attn_decode_paged(const AttnDecodePaged& p, void* o, float* lse, hipStream_t st) {
  const AttnDecode& d = p.d;
  if (d.D != 64 && d.D != 128) {
    fprintf(stderr, "attn_decode_paged: head dim must be 64 or 128, got %d\n", d.D);
    abort();
  }
  if (d.Hkv <= 0 || d.H % d.Hkv != 0) {
    fprintf(stderr, "attn_decode_paged: %d query heads do not split over %d key/value heads\n",
            d.H, d.Hkv);
    abort();
  }
  if (!page_size_ok(p.log2_page) || p.num_pages <= 0 || p.max_pages <= 0 ||
      p.block_table == nullptr) {
    fprintf(stderr, "attn_decode_paged: pages of 16 .. 256 rows, a pool and a table, got log2 P "
                    "= %d, %d pages, %d table columns\n", p.log2_page, p.num_pages, p.max_pages);
    abort();
  }
  if (d.nsplit < 1 || d.nsplit > kAttnDecodeMaxSplits ||
      (d.nsplit > 1 && (d.o_part == nullptr || d.lse_part == nullptr))) {
    fprintf(stderr, "attn_decode_paged: nsplit = %d needs 1 .. %d and, above 1, the workspace\n",
            d.nsplit, kAttnDecodeMaxSplits);
    abort();
  }
  if (d.B <= 0 || d.Sq <= 0) return;
  if (d.k_new.p != nullptr) attn_paged_append(p, d.Sq, st);
  PagedArgs a{};
  a.q = d.q.p; a.qsb = d.q.sb; a.qss = d.q.ss; a.qsh = d.q.sh;
  a.k = d.k.p; a.ksp = d.k.sb; a.kss = d.k.ss; a.ksh = d.k.sh;
  a.v = d.v.p; a.vsp = d.v.sb; a.vss = d.v.ss; a.vsh = d.v.sh;
  a.lens = d.cache_seqlens;
  a.table = p.block_table;
  a.append = d.k_new.p != nullptr ? 1 : 0;
  a.o = o; a.lse = lse; a.o_part = d.o_part; a.lse_part = d.lse_part;
  a.B = d.B; a.H = d.H; a.Hkv = d.Hkv; a.G = d.H / d.Hkv; a.Sq = d.Sq;
  a.Smax = p.max_pages << p.log2_page;
  a.R = a.G * d.Sq;
  a.num_pages = p.num_pages; a.max_pages = p.max_pages; a.lp = p.log2_page;
  a.scale_log2 = d.scale * 1.4426950408889634f;
  if (d.dtype == DType::BF16) {
    if (d.D == 64) launch_paged<bf16_t, 64>(p, a, st);
    else launch_paged<bf16_t, 128>(p, a, st);
  } else {
    if (d.D == 64) launch_paged<half_t, 64>(p, a, st);
    else launch_paged<half_t, 128>(p, a, st);
  }
  if (d.nsplit > 1)
    attn_decode_combine(d.dtype, d.D, d.B, d.H, d.Sq, d.nsplit, d.o_part, d.lse_part, o, lse, st);
}

}  // namespace amd
