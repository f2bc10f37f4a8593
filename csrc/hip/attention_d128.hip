// Fused multi-head attention for gfx950 at head dim 128 (bf16 / fp16, optional causal
// mask, dropout, key masks, cross-attention, packed sequences): the forward, dQ and dK/dV
// kernels of attention.hip written again for 256-byte rows, on the same
// v_mfma_f32_32x32x16_{bf16,f16}, global_load_lds rings and transposed LDS reads.  Every
// convention a caller or the other direction can see is that file's (read its header
// first): strided [B, S, H, D] views, o contiguous, lse / D as [B, H, round_up(Sq, 64)] in
// log2 units, the prepared key mask (bias, live), the dropout hash of (seed, b*H+h, query,
// key quad), tile_of_block, the CAUSAL / DROP / KMASK / VARLEN switches, two backward
// launches (dQ, which also writes D, then dK/dV), no atomics.
//
// What is new is where a 128-wide tile lives and how many workgroups share a CU.
//
// LDS images.  A [64 rows][128 d] tile is kept as TWO [64][64] half images (d 0..63 and
// d 64..127, 8 KiB each, the second right behind the first), each with the swizzle
// attention.hip proved conflict-free for 128-byte rows: swz_rows for ds_read_b128 row
// fragments, swz_tr for ds_read_b64_tr_b16.  A lane's logical 16-byte chunk c (0..15)
// picks half image c >> 3 and swizzled slot c & 7, so every LDS read of these kernels is
// a D = 64 read plus a compile-time half-image offset, every DMA instruction still fills
// 8 rows x 128 B = 1 KiB of one half image, and the second half's source is the first
// half's moved by 64 elements (a scalar add on the tile base, no per-lane work).  A
// 16-chunk swizzle over 256-byte rows would need its own bank-conflict proof for both
// kinds of read and buys nothing: the MFMA steps consume 16 d at a time either way.
//
// Forward (attn128_fwd_k): one wave = 32 queries, workgroup = 4 waves = 128 queries, as at
// D = 64.  A wave holds Q^T as 8 fragments (32 VGPRs) and O^T as 4 accumulators of 32 x 32
// (64 VGPRs); S^T = K . Q^T takes 8 MFMAs per 32 keys, O^T += V^T . P^T 4 per 16 keys.
// One K + V tile is 32 KiB, the double-buffered ring 64 KiB (+ 2 x 1 KiB of key bias):
// two workgroups per CU fit the 160 KiB, and __launch_bounds__(256, 2) gives them 256
// registers per lane, which the kernel stays under without scratch (docs/PERF.md has the
// compiler's report).
//
// dQ (attn128_bwd_dq_k): same split.  The ring slot holds K as a row image (A of S^T) and
// a transposed-read image (A of dQ^T) and V as a row image (A of dP^T): 3 x 16 KiB, 96 KiB
// double buffered - ONE workgroup per CU.  Halving the slot to 32 keys (48 KiB, two to
// three workgroups) would double the barriers per key and break the 64-key granule that
// the key-mask bias rows, the liveness bytes and the causal tile count share with the
// forward; instead the single workgroup takes the 512-register budget
// (__launch_bounds__(256, 1)) and runs both 32-key halves of a tile as one straight-line
// block, so the MFMAs of one half overlap the exp2 / dropout VALU of the other inside the
// wave, which is the latency hiding a second workgroup would have provided.
//
// dK/dV (attn128_bwd_dkdv_k): workgroup = 128 keys, 32 per wave, loop over 64-query tiles.
// A wave holds K^T and V^T of its keys as 16 fragments (64 VGPRs) and dK^T, dV^T as 8
// accumulators (128 VGPRs); with the score and dP tiles of one 64-query step (64) that is
// 256 registers before a single address, so a 256-register budget cannot hold it whatever
// the ring looks like: 32-query slots would cure the LDS side of two workgroups per CU
// (65 KiB each) but not the register side, and spilling accumulators inside the loop costs
// more than the second workgroup gains.  Hence ONE workgroup per CU with the unified
// 512-register file, and the ring keeps 64-query slots: Q and dO each as a row image and
// a transposed-read image (4 x 16 KiB) + 1 KiB of lse / D, 65 KiB per slot, 130 KiB double
// buffered of the CU's 160 KiB.  The registers left over pay for the straight-line
// two-half schedule of the mask-free instantiations (the key-mask ones go half by half,
// as at D = 64: the compiler's report showed spills otherwise).
//
// Grouped-query heads (GQA = true, compiled by attention_gqa.hip): as in attention.hip - the
// dK/dV workgroup belongs to a key/value head and walks its group's query heads on one ring.
#include "attention_common.h"

namespace amd {

namespace {

constexpr int kD = 128;                  // head dim
constexpr int kImg = kAKT * kARow;       // 8 KiB: one [64][64] half image
constexpr int kTile = 2 * kImg;          // 16 KiB: a [64][128] tile, halves back to back

// row 128 d of a 4-accumulator transposed result (d = 32 dt + row) times `mul`
template <typename T>
__device__ __forceinline__ void store_dT128(T* row_ptr, const f32x16_t (&acc)[4], int hl,
                                            float mul) {
  store_dT<T>(row_ptr, reinterpret_cast<const f32x16_t(&)[2]>(acc[0]), hl, mul);
  store_dT<T>(row_ptr + kAD, reinterpret_cast<const f32x16_t(&)[2]>(acc[2]), hl, mul);
}

// One wave's share of a full [64][128] tile DMA into a tile image at `img`: rows
// (2 wid + i) * 8 + lane / 8 of both half images, `off[i]` the lane's byte offset of its
// row and logical chunk in the first half (row_off with the image's swizzle).
template <typename T>
__device__ __forceinline__ void dma_tile(const T* base, const uint32_t (&off)[2], unsigned char* img,
                                         int wid) {
#pragma unroll
  for (int hf = 0; hf < 2; ++hf)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      glds16o(base + kAD * hf, off[i], img + hf * kImg + (wid * 2 + i) * 1024);
}
// the same from a per-lane row pointer (clamped rows: tiles that reach past the length);
// `ch[i]` is the lane's logical chunk (0..7) of row (2 wid + i) * 8 + lane / 8
template <typename T>
__device__ __forceinline__ void dma_row(const T* row, int ch, unsigned char* img, int wid, int i) {
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) glds16(row + kAD * hf + ch * 8, img + hf * kImg + (wid * 2 + i) * 1024);
}

// row fragment of d step s (d = 16 s + 8 hl ..): half image s >> 2, the D = 64 offset of
// step s & 3
template <typename T>
__device__ __forceinline__ typename Frag<T>::v8 row_frag(const unsigned char* img, const int (&off)[4],
                                                         int s) {
  return lds_row8<T>(img + (s >> 2) * kImg, off[s & 3]);
}

// The register-held operand fragments come from plain global loads issued before the loop.
// The compiler counts those loads but not the inline-asm DMA (nor the ring's own
// s_waitcnt), so left alone it puts their s_waitcnt vmcnt(N) at the first use INSIDE the
// loop, every iteration, where vmcnt(0) also waits out the prefetch the iteration has just
// issued.  So, right after the prologue's DMA issue, one s_waitcnt vmcnt(0) the compiler
// can see (the first iteration waits for vmcnt(0) anyway) followed by the fragments as asm
// operands, which keep their loads above that wait whatever the scheduler does.
template <typename V, int N>
__device__ __forceinline__ void settle(V (&f)[N]) {
  typedef int v4i_t __attribute__((ext_vector_type(4)));
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), expcnt and lgkmcnt left at their maxima
#pragma unroll
  for (int s = 0; s < N; ++s) {
    v4i_t x = __builtin_bit_cast(v4i_t, f[s]);
    asm volatile("" : "+v"(x));
    f[s] = __builtin_bit_cast(V, x);
  }
}

// ---------------------------------------------------------------------------- forward
template <typename T, bool CAUSAL, bool DROP, bool KMASK, bool VARLEN, bool AMASK, bool GQA>
__global__ void __launch_bounds__(kAT, 2) attn128_fwd_k(AttnArgs a) {
  int Sq = a.Sq, Sk = CAUSAL ? a.Sq : a.Sk;
  [[maybe_unused]] const int kstride = CAUSAL ? a.lse_stride : a.key_stride;
  typedef typename Frag<T>::v8 v8;
  constexpr int KV = 2 * kTile;                 // K and V tile images: 32 KiB
  // KMASK: + the tile's 64 bias floats; AMASK: + the tile's 128 mask words
  constexpr int BUF = KV + (KMASK || AMASK ? 1024 : 0);
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hl = lane >> 5, c32 = lane & 31;
  int tile, bh;
  tile_of_block(CAUSAL, true, tile, bh);
  const int b = bh / a.H, hh = bh - b * a.H;
  const int hk = GQA ? hh / a.G : hh;  // the key/value head this query head reads
  const int qb0 = tile * 128;
  [[maybe_unused]] int s0 = 0;
  if constexpr (VARLEN) {
    if (!varlen_seq(a.cu, b, a.T, a.Sq, qb0, s0, Sq)) return;
    Sk = Sq;
  }
  const int q = qb0 + wid * 32 + c32;  // this lane's query
  const uint32_t dbase = DROP ? drop_base(a.seed, (uint32_t)bh) + (uint32_t)q * kDropQ +
                                    (uint32_t)hl * kDropK
                              : 0u;
  const T* Q = static_cast<const T*>(a.q) + seq_off<VARLEN>(b, s0, a.qsb, a.qss) + hh * a.qsh;
  const T* K = static_cast<const T*>(a.k) + seq_off<VARLEN>(b, s0, a.ksb, a.kss) + hk * a.ksh;
  const T* V = static_cast<const T*>(a.v) + seq_off<VARLEN>(b, s0, a.vsb, a.vss) + hk * a.vsh;

  // Q^T fragments (B operand of S^T = K . Q^T): d = 16s + 8hl + j
  v8 qf[8];
  {
    const int qq = q < Sq ? q : Sq - 1;
#pragma unroll
    for (int s = 0; s < 8; ++s)
      qf[s] = *reinterpret_cast<const v8*>(Q + (int64_t)qq * a.qss + 16 * s + 8 * hl);
  }

  int nkt = (Sk + kAKT - 1) / kAKT;
  if (CAUSAL) {
    const int last = (qb0 + 127 < Sq ? qb0 + 127 : Sq - 1) / kAKT + 1;
    nkt = last < nkt ? last : nkt;
  }
  // DMA: each wave fills 16 rows of K and of V per tile (4 x 1 KiB instructions each)
  const int lrow = lane >> 3, pch = lane & 7;
  uint32_t kof[2], vof[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (wid * 2 + i) * 8 + lrow;
    kof[i] = row_off<T>(row, a.kss, (swz_rows(row, pch) - row * kARow) >> 4);  // logical chunk at pch
    vof[i] = row_off<T>(row, a.vss, (swz_tr(row, pch) - row * kARow) >> 4);
  }
  const float* kbias = KMASK ? a.kbias + (int64_t)b * kstride : nullptr;
  // AMASK: row `tile` of this batch element's mask words, 1 KiB per key tile
  const unsigned long long* wrow = AMASK ? a.wq + (b * a.mqs + (int64_t)tile * nkt) * 128 : nullptr;
  auto issue = [&](int kt, int buf) {
    unsigned char* Kl = lds + buf * BUF;
    unsigned char* Vl = Kl + kTile;
    if constexpr (KMASK) {  // lanes 0-15: bias[k0 .. k0+63], the rest pad (bias again)
      if (wid == 0) glds16(kbias + kt * kAKT + (lane & 15) * 4, Kl + KV);
    }
    if constexpr (AMASK) {  // two words per lane: the tile's 128 queries
      if (wid == 0) glds16(wrow + kt * 128 + lane * 2, Kl + KV);
    }
    if ((kt + 1) * kAKT <= Sk) {
      dma_tile<T>(tile_base(K, kt * kAKT, a.kss), kof, Kl, wid);
      dma_tile<T>(tile_base(V, kt * kAKT, a.vss), vof, Vl, wid);
      return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (wid * 2 + i) * 8 + lrow;
      const int key = kt * kAKT + row;
      const int kk = key < Sk ? key : Sk - 1;
      dma_row<T>(K + (int64_t)kk * a.kss, (swz_rows(row, pch) - row * kARow) >> 4, Kl, wid, i);
      dma_row<T>(V + (int64_t)kk * a.vss, (swz_tr(row, pch) - row * kARow) >> 4, Vl, wid, i);
    }
  };

  f32x16_t o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
  float m = -INFINITY, l = 0.f;

  // loop-invariant LDS offsets inside a half image
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
        const int r0 = 32 * t + 16 * s + 4 * hl;
        const int c0 = 32 * dt + ((lane >> 4) & 1) * 16;
        vlo[dt][t][s] = tr_addr(r0, c0, lane);
        vhi[dt][t][s] = tr_addr(r0 + 8, c0, lane);
      }

  [[maybe_unused]] bool full = false;  // AMASK: every pair of the tile in hand attends
  auto step = [&](int kt, int buf, int nx) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (KMASK || AMASK) {
      if (nx < nkt) issue(nx, buf ^ 1);
    } else {
      if (kt + 1 < nkt) issue(kt + 1, buf ^ 1);
    }
    const unsigned char* Kl = lds + buf * BUF;
    const unsigned char* Vl = Kl + kTile;
    const int k0 = kt * kAKT;
    if (CAUSAL && k0 > qb0 + wid * 32 + 31) return;  // whole tile masked for this wave

    f32x16_t x[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int i = 0; i < 16; ++i) x[t][i] = 0.f;
#pragma unroll
      for (int s = 0; s < 8; ++s) x[t] = mfma32<T>(row_frag<T>(Kl, koff[t], s), qf[s], x[t]);
    }
    bool grow;
    float alpha, psum = 0.f;
    if constexpr (KMASK) {
      // biased scores in log2 units, running max over the BIASED values; a query with no
      // live key so far keeps m = -inf and exponent offset 0 (attention.hip)
      const float* bl = reinterpret_cast<const float*>(Kl + KV);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const float4 bv = *reinterpret_cast<const float4*>(bl + 32 * t + 8 * rq + 4 * hl);
          const float be[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            x[t][4 * rq + e] = fmaf(x[t][4 * rq + e], a.scale_log2, be[e]);
        }
      if (CAUSAL && k0 + kAKT - 1 > qb0 + wid * 32) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hl;
            if (key > q) x[t][r] = -INFINITY;
          }
      }
      float tmax = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, x[t][r]);
      tmax = max_halves(tmax);
      const float mnew = fmaxf(m, tmax);
      const float msafe = mnew == -INFINITY ? 0.f : mnew;
      grow = __any(mnew != m);
      alpha = grow ? fexp2(m - msafe) : 1.f;
      m = mnew;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = fexp2(x[t][r] - msafe);
          psum += p;
          x[t][r] = p;
        }
    } else if (AMASK && !full) {
      // mixed tile (wave-uniform): -inf where the lane's bit of the pair is clear (bits past
      // Sq / Sk are clear), then the key-mask path's -inf-safe running max
      const uint2 w = pair_word(Kl + KV, wid * 32 + c32, hl);
      float tmax = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          x[t][r] = pair_bit(w, t, r) ? x[t][r] * a.scale_log2 : -INFINITY;
          tmax = fmaxf(tmax, x[t][r]);
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
        for (int r = 0; r < 16; ++r) {
          const float p = fexp2(x[t][r] - msafe);
          psum += p;
          x[t][r] = p;
        }
    } else {
      // mask (boundary / diagonal tiles only: wave-uniform test), running max on the raw
      // scores, then one fma + exp2 per score in log2 units; an AMASK tile that gets here is
      // full, which puts it inside Sq x Sk
      const bool need_mask =
          !AMASK && ((k0 + kAKT > Sk) || (CAUSAL && k0 + kAKT - 1 > qb0 + wid * 32));
      if (need_mask) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hl;
            if (key >= Sk || (CAUSAL && key > q)) x[t][r] = -INFINITY;
          }
      }
      float tmax = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, x[t][r]);
      tmax = max_halves(tmax);
      const float mnew = fmaxf(m, tmax * a.scale_log2);
      grow = __any(mnew != m);  // the O / l rescale is skipped while no max of the wave rose
      alpha = grow ? fexp2(m - mnew) : 1.f;
      m = mnew;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = fexp2(fmaf(x[t][r], a.scale_log2, -mnew));
          psum += p;
          x[t][r] = p;
        }
    }
    l = l * alpha + psum;
    if (grow) {
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
    }
    if (DROP) {  // dropped P (the 1/(1-p) factor is applied to O once, at the store)
      const uint32_t tb = dbase + (uint32_t)(k0 >> 2) * kDropK;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          // key quad (k0 + 32t + 8rq + 4hl) >> 2 (keys + r & 3): a literal lattice step
          const uint32_t hsh = drop_mix(tb + (uint32_t)(8 * t + 2 * rq) * kDropK);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            x[t][4 * rq + e] = drop_keep8(hsh, e, a.thr8) ? x[t][4 * rq + e] : 0.f;
        }
    }
    // O^T[d][q] += V^T[d][key] . P^T[key][q]: d tile dt lives in V half image dt >> 1
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const v8 pf = acc_frag<T>(x[t], s);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          o[dt] = mfma32<T>(lds_tr8<T>(Vl + (dt >> 1) * kImg, vlo[dt & 1][t][s], vhi[dt & 1][t][s]),
                            pf, o[dt]);
      }
  };
  if constexpr (KMASK) {
    LiveTiles lt(a.klive + (int64_t)b * (kstride / kAKT), nkt, lane);
    int kt = lt.next();
    if (kt < nkt) issue(kt, 0);
    settle(qf);
    for (int slot = 0; kt < nkt; slot ^= 1) {
      const int nx = lt.next();
      step(kt, slot, nx);
      kt = nx;
    }
  } else if constexpr (AMASK) {
    PairTiles pt(a.cq + b * a.mqs + (int64_t)tile * nkt, nkt, lane);
    int kt = pt.next();
    if (kt < nkt) issue(kt, 0);
    settle(qf);
    for (int slot = 0; kt < nkt; slot ^= 1) {
      full = pt.full;
      const int nx = pt.next();
      step(kt, slot, nx);
      kt = nx;
    }
  } else {
    issue(0, 0);
    settle(qf);
    for (int kt = 0; kt < nkt; ++kt) step(kt, kt & 1, 0);
  }

  const float lt = l + __shfl_xor(l, 32);
  const float inv = lt > 0.f ? (DROP ? a.inv_keep : 1.f) / lt : 0.f;
  if (q < Sq) {
    const int64_t orow = VARLEN ? (int64_t)s0 + q : (int64_t)b * Sq + q;
    store_dT128<T>(static_cast<T*>(a.o) + (orow * a.H + hh) * kD, o, hl, inv);
    if (hl == 0) a.lse[(int64_t)bh * a.lse_stride + q] = m + log2f(lt);
  }
}

// ---------------------------------------------------------------------------- backward
// dK / dV: S[q][key] = Q . K^T unswapped with the wave's K^T / V^T fragments in registers,
// dV^T = dO^T . P and dK^T = Q^T . dS from the accumulators (attention.hip); one workgroup
// per CU, see the header for the register and LDS budget.
template <typename T, bool CAUSAL, bool DROP, bool KMASK, bool VARLEN, bool AMASK, bool GQA>
__global__ void __launch_bounds__(kAT, 1) attn128_bwd_dkdv_k(AttnBwdArgs a) {
  int Sq = a.Sq, Sk = CAUSAL ? a.Sq : a.Sk;
  [[maybe_unused]] const int kstride = CAUSAL ? a.lse_stride : a.key_stride;
  typedef typename Frag<T>::v8 v8;
  // Q rows, Q tr, dO rows, dO tr, {lse, D}: 65 KiB[, AMASK: the tile's 128 mask words: 66]
  constexpr int BUF = 4 * kTile + 1024 + (AMASK ? 1024 : 0);
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hl = lane >> 5, c32 = lane & 31;
  int tile, bh;
  tile_of_block(CAUSAL, false, tile, bh);
  // GQA: the grid's rows are (b, key/value head).  hh is that head, the owner of K, V, dK and
  // dV; bhq is the first of the a.G query heads that read it, whose Q / dO / lse / D rows and
  // dropout hashes the loop below walks member by member.
  const int nh = GQA ? a.H / a.G : a.H;
  const int b = bh / nh, hh = bh - b * nh;
  const int qh = GQA ? hh * a.G : hh;
  const int bhq = GQA ? b * a.H + qh : bh;
  const int kb0 = tile * 128;
  [[maybe_unused]] int s0 = 0;
  if constexpr (VARLEN) {
    if (!varlen_seq(a.cu, b, a.T, a.Sq, kb0, s0, Sq)) return;
    Sk = Sq;
  }
  const int kw0 = kb0 + wid * 32;
  const int key = kw0 + c32;
  const int kk = key < Sk ? key : Sk - 1;
  float kbias = 0.f;
  bool wave_dead = false;
  if constexpr (KMASK) {
    const int nlt = kstride / kAKT;
    const unsigned char* lv = a.klive + (int64_t)b * nlt;
    const int t0 = kb0 / kAKT;
    if (lv[t0] == 0 && (t0 + 1 >= nlt || lv[t0 + 1] == 0)) {  // 128 dead keys: zeros
      if (key < Sk) {
        T* dvp = static_cast<T*>(a.dv) + b * a.dvsb + (int64_t)key * a.dvss + hh * a.dvsh;
        T* dkp = static_cast<T*>(a.dk) + b * a.dksb + (int64_t)key * a.dkss + hh * a.dksh;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          *reinterpret_cast<uint4*>(dvp + 64 * hl + 8 * i) = uint4{0u, 0u, 0u, 0u};
          *reinterpret_cast<uint4*>(dkp + 64 * hl + 8 * i) = uint4{0u, 0u, 0u, 0u};
        }
      }
      return;
    }
    kbias = key < Sk ? a.kbias[(int64_t)b * kstride + key] : -INFINITY;
    wave_dead = !__any(kbias > -INFINITY);
  }
  // dropout lattice point of (query key & 3, this lane's key quad)
  uint32_t kdrop = DROP ? drop_base(a.seed, (uint32_t)bhq) + (uint32_t)(key >> 2) * kDropK +
                              (uint32_t)(key & 3) * kDropQ
                        : 0u;
  const T* Q = static_cast<const T*>(a.q) + seq_off<VARLEN>(b, s0, a.qsb, a.qss) + qh * a.qsh;
  const T* dO = static_cast<const T*>(a.dout) + seq_off<VARLEN>(b, s0, a.dsb, a.dss) + qh * a.dsh;
  // KMASK / AMASK: the guarded copy of lse that the dQ kernel left behind D
  const float* lse = (KMASK || AMASK ? a.D + (int64_t)a.B * a.H * a.lse_stride : a.lse) +
                     (int64_t)bhq * a.lse_stride;
  const float* Dr = a.D + (int64_t)bhq * a.lse_stride;

  // K^T / V^T fragments (B operands): key = this lane's column, d = 16s + 8hl + j
  v8 kf[8], vf[8];
  {
    const T* K = static_cast<const T*>(a.k) + seq_off<VARLEN>(b, s0, a.ksb, a.kss) + hh * a.ksh +
                 (int64_t)kk * a.kss;
    const T* V = static_cast<const T*>(a.v) + seq_off<VARLEN>(b, s0, a.vsb, a.vss) + hh * a.vsh +
                 (int64_t)kk * a.vss;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      kf[s] = *reinterpret_cast<const v8*>(K + 16 * s + 8 * hl);
      vf[s] = *reinterpret_cast<const v8*>(V + 16 * s + 8 * hl);
    }
  }

  const int nqt = (Sq + kAKT - 1) / kAKT;
  const int qt0 = CAUSAL ? kb0 / kAKT : 0;
  const int lrow = lane >> 3, pch = lane & 7;
  uint32_t qro[2], qto[2], dro[2], dto[2];  // full tiles: the forward's scalar-base form
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (wid * 2 + i) * 8 + lrow;
    const int chr = (swz_rows(row, pch) - row * kARow) >> 4;
    const int cht = (swz_tr(row, pch) - row * kARow) >> 4;
    qro[i] = row_off<T>(row, a.qss, chr);
    qto[i] = row_off<T>(row, a.qss, cht);
    dro[i] = row_off<T>(row, a.dss, chr);
    dto[i] = row_off<T>(row, a.dss, cht);
  }
  // images per slot: 0 = Q rows, 1 = Q transposed, 2 = dO rows, 3 = dO transposed, then
  // {lse, D}; a wave issues 16 x 1 KiB of tile DMA per slot.  With 512 registers the eight
  // offsets of the scalar-base form fit (at D = 64 they spilled, so that kernel forms
  // per-lane addresses always); only a tile that reaches past Sq takes the clamped path.
  // AMASK: row `tile` of this batch element's transposed mask words, 1 KiB per query tile
  const unsigned long long* wrow = AMASK ? a.wk + (b * a.mks + (int64_t)tile * nqt) * 128 : nullptr;
  auto issue = [&](int qt, int buf) {
    unsigned char* base = lds + buf * BUF;
    if constexpr (AMASK) {  // two words per lane: the tile's 128 keys
      if (wid == 1) glds16(wrow + qt * 128 + lane * 2, base + 4 * kTile + 1024);
    }
    if (wid == 0) {  // lanes 0-15: lse[q0 .. q0+63], 16-31: D[...], 32-63: pad (lse again)
      const int seg = (lane >> 4) & 1, part = lane & 15;
      const float* src = (seg ? Dr : lse) + qt * kAKT + part * 4;
      glds16(src, base + 4 * kTile);
    }
    if ((qt + 1) * kAKT <= Sq) {
      const T* qb = tile_base(Q, qt * kAKT, a.qss);
      const T* db = tile_base(dO, qt * kAKT, a.dss);
      dma_tile<T>(qb, qro, base, wid);
      dma_tile<T>(qb, qto, base + kTile, wid);
      dma_tile<T>(db, dro, base + 2 * kTile, wid);
      dma_tile<T>(db, dto, base + 3 * kTile, wid);
      return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (wid * 2 + i) * 8 + lrow;
      const int qr = qt * kAKT + row;
      const int qc = qr < Sq ? qr : Sq - 1;
      const int chr = (swz_rows(row, pch) - row * kARow) >> 4;
      const int cht = (swz_tr(row, pch) - row * kARow) >> 4;
      const T* qrow = Q + (int64_t)qc * a.qss;
      const T* drow = dO + (int64_t)qc * a.dss;
      dma_row<T>(qrow, chr, base, wid, i);
      dma_row<T>(qrow, cht, base + kTile, wid, i);
      dma_row<T>(drow, chr, base + 2 * kTile, wid, i);
      dma_row<T>(drow, cht, base + 3 * kTile, wid, i);
    }
  };

  f32x16_t dv[4], dk[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) dv[dt][i] = dk[dt][i] = 0.f;

  int roff[2][4];  // [query half][d step & 3]: row 32h + c32, chunk 2s + hl
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int s = 0; s < 4; ++s) roff[h][s] = swz_rows(32 * h + c32, 2 * s + hl);
  int tlo[2][2][2], thi[2][2][2];  // [d tile & 1][query half][k step]
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int r0 = 32 * h + 16 * s + 4 * hl;
        const int c0 = 32 * dt + ((lane >> 4) & 1) * 16;
        tlo[dt][h][s] = tr_addr(r0, c0, lane);
        thi[dt][h][s] = tr_addr(r0 + 8, c0, lane);
      }

  // AMASK: qt walks the non-dead query tiles of this key tile's row of classes (nx = the
  // one after qt, `full` the class of qt), the ring slot alternates
  PairTiles pt(AMASK ? a.ck + b * a.mks + (int64_t)tile * nqt : nullptr, nqt, lane);
  [[maybe_unused]] int nx = 0, slot = 0;
  [[maybe_unused]] bool full = false;
  // GQA: the workgroup serves the a.G query heads of its key/value head one after the other,
  // against the same K^T / V^T fragments and into the same accumulators: the flattened
  // sequence of (member g, query tile qt), every member from its own qt0.  The ring runs
  // through the head boundary: when a member's last tile is in hand its successor's first is
  // prefetched, for which next_member() moves what issue() reads - wave-uniform bases, which
  // stay in SGPRs - one head on; next_tile() then moves the math (g, the dropout lattice
  // base, qt) when it gets there.
  [[maybe_unused]] int g = 0;
  [[maybe_unused]] auto next_member = [&]() {
    Q += a.qsh;
    dO += a.dsh;
    lse += a.lse_stride;
    Dr += a.lse_stride;
  };
  [[maybe_unused]] auto next_tile = [&](int qt) {
    if (qt + 1 < nqt || g + 1 >= a.G) return qt + 1;
    ++g;
    // the lane's lattice point moves by the difference of the two heads' bases: scalar work
    // and one add, no second per-lane term kept alive through the loop
    if (DROP)
      kdrop += drop_base(a.seed, (uint32_t)(bhq + g)) - drop_base(a.seed, (uint32_t)(bhq + g - 1));
    return qt0;
  };
  if constexpr (AMASK) {
    nx = pt.next();
    if (nx < nqt) issue(nx, 0);
  } else {
    if (qt0 < nqt) issue(qt0, 0);
  }
  settle(kf);
  settle(vf);
  for (int qt = AMASK ? nx : qt0; qt < nqt; qt = AMASK ? nx : GQA ? next_tile(qt) : qt + 1) {
    if constexpr (AMASK) {
      full = pt.full;
      nx = pt.next();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (AMASK) {
      if (nx < nqt) issue(nx, slot ^ 1);
    } else if constexpr (GQA) {
      if (qt + 1 < nqt) {
        issue(qt + 1, slot ^ 1);
      } else if (g + 1 < a.G) {
        next_member();
        issue(qt0, slot ^ 1);
      }
    } else {
      if (qt + 1 < nqt) issue(qt + 1, (qt + 1 - qt0) & 1);
    }
    const unsigned char* base = lds + (AMASK || GQA ? slot : ((qt - qt0) & 1)) * BUF;
    if constexpr (AMASK || GQA) slot ^= 1;
    const unsigned char* Qr = base;
    const unsigned char* Qt = base + kTile;
    const unsigned char* Or = base + 2 * kTile;
    const unsigned char* Ot = base + 3 * kTile;
    const float* st_lse = reinterpret_cast<const float*>(base + 4 * kTile);
    const float* st_D = st_lse + 64;
    const int q0 = qt * kAKT;
    if (KMASK && wave_dead) continue;  // wave-uniform: dk = dv = 0 for all 32 keys
    // the four stages of one 32-query half h
    auto sdp = [&](int h, f32x16_t& sc, f32x16_t& dp) {
#pragma unroll
      for (int i = 0; i < 16; ++i) sc[i] = dp[i] = 0.f;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        sc = mfma32<T>(row_frag<T>(Qr, roff[h], s), kf[s], sc);
        dp = mfma32<T>(row_frag<T>(Or, roff[h], s), vf[s], dp);
      }
    };
    auto softmax_bwd = [&](int h, f32x16_t& sc, f32x16_t& dp) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int li = 32 * h + 8 * g + 4 * hl;  // local query of register 4g
        const float4 lv = *reinterpret_cast<const float4*>(st_lse + li);
        const float4 dd = *reinterpret_cast<const float4*>(st_D + li);
        const float lsev[4] = {lv.x, lv.y, lv.z, lv.w};
        const float Dv[4] = {dd.x, dd.y, dd.z, dd.w};
        // one hash per (query, key quad): each lane of a key quad hashes one of the
        // group's 4 queries and reads the other three over DPP (attention.hip)
        uint32_t hq[4];
        if (DROP) {
          const uint32_t qhb = kdrop + (uint32_t)(q0 + 32 * h + 4 * hl) * kDropQ;
          const uint32_t v = drop_mix(qhb + (uint32_t)(8 * g) * kDropQ);
          hq[0] = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x00, 0xF, 0xF, false);
          hq[1] = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x55, 0xF, 0xF, false);
          hq[2] = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xAA, 0xF, 0xF, false);
          hq[3] = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xFF, 0xF, 0xF, false);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          bool keep = true;
          if (DROP) keep = drop_keep8(hq[e], key & 3, a.thr8);
          float p;
          if constexpr (KMASK) p = fexp2(fmaf(sc[r], a.scale_log2, kbias - lsev[e]));
          else p = fexp2(fmaf(sc[r], a.scale_log2, -lsev[e]));
          // dropped dP scaled by 1/(1-p); the dropped P feeding dV^T stays unscaled (the
          // factor is applied to dV once, at the store)
          const float dpz = DROP ? (keep ? dp[r] * a.inv_keep : 0.f) : dp[r];
          sc[r] = (DROP && !keep) ? 0.f : p;
          dp[r] = p * (dpz - Dv[e]);
        }
      }
    };
    auto mask = [&](int h, f32x16_t& sc, f32x16_t& dp) {
      if constexpr (AMASK) {  // this lane's key against the half's 32 queries (0 past Sq)
        const uint2 w = pair_word(base + 4 * kTile + 1024, wid * 32 + c32, hl);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!pair_bit(w, h, r)) sc[r] = dp[r] = 0.f;
        return;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q = q0 + 32 * h + 8 * (r >> 2) + 4 * hl + (r & 3);
        if (!(q < Sq && !(CAUSAL && key > q))) sc[r] = dp[r] = 0.f;
      }
    };
    auto accum = [&](int h, const f32x16_t& sc, const f32x16_t& dp) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const v8 pf = acc_frag<T>(sc, s);
        const v8 sf = acc_frag<T>(dp, s);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const int ho = (dt >> 1) * kImg;  // d tile dt: half image dt >> 1
          dv[dt] = mfma32<T>(lds_tr8<T>(Ot + ho, tlo[dt & 1][h][s], thi[dt & 1][h][s]), pf, dv[dt]);
          dk[dt] = mfma32<T>(lds_tr8<T>(Qt + ho, tlo[dt & 1][h][s], thi[dt & 1][h][s]), sf, dk[dt]);
        }
      }
    };
    // wave-uniform: no (query, key) of the 64 x 32 tile needs a mask - both halves run as
    // ONE straight-line block (half 1's S / dP MFMAs beside half 0's softmax VALU).
    // KMASK goes half by half, as at D = 64: with the bias and the dead-wave branch the
    // straight-line block filled all 512 registers and spilled ~70 more.
    // AMASK: a full tile is clean, a mixed one masks both halves by its bits.
    const bool clean = AMASK ? full : (q0 + kAKT <= Sq) && (!CAUSAL || kw0 + 31 <= q0);
    if (!KMASK && clean) {
      f32x16_t sc0, dp0, sc1, dp1;
      sdp(0, sc0, dp0);
      sdp(1, sc1, dp1);
      softmax_bwd(0, sc0, dp0);
      accum(0, sc0, dp0);
      softmax_bwd(1, sc1, dp1);
      accum(1, sc1, dp1);
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int qh0 = q0 + 32 * h;
        if (CAUSAL && qh0 + 31 < kw0) continue;  // every query of this half precedes every key
        f32x16_t sc, dp;
        sdp(h, sc, dp);
        softmax_bwd(h, sc, dp);
        if (AMASK || (qh0 + 31 >= Sq) || (CAUSAL && kw0 + 31 > qh0)) mask(h, sc, dp);
        accum(h, sc, dp);
      }
    }
  }

  if (key < Sk) {
    store_dT128<T>(static_cast<T*>(a.dv) + seq_off<VARLEN>(b, s0, a.dvsb, a.dvss) +
                       (int64_t)key * a.dvss + hh * a.dvsh,
                   dv, hl, DROP ? a.inv_keep : 1.f);
    store_dT128<T>(static_cast<T*>(a.dk) + seq_off<VARLEN>(b, s0, a.dksb, a.dkss) +
                       (int64_t)key * a.dkss + hh * a.dksh,
                   dk, hl, a.scale);
  }
}

// dQ: workgroup = 128 queries, loop over 64-key tiles in the forward's swapped orientation
// (a lane's lse / D are scalars, dQ^T = K^T . dS^T from the accumulator); it also forms
// D = rowsum(dO * O) and, under a key mask, leaves the guarded lse and the refined D for
// the dK/dV kernel (attention.hip).  One workgroup per CU, see the header.
template <typename T, bool CAUSAL, bool DROP, bool KMASK, bool VARLEN, bool AMASK, bool GQA>
__global__ void __launch_bounds__(kAT, 1) attn128_bwd_dq_k(AttnBwdArgs a) {
  int Sq = a.Sq, Sk = CAUSAL ? a.Sq : a.Sk;
  [[maybe_unused]] const int kstride = CAUSAL ? a.lse_stride : a.key_stride;
  typedef typename Frag<T>::v8 v8;
  // K rows, K tr, V rows: 48 KiB[, KMASK: the bias; AMASK: the tile's 128 mask words]
  constexpr int BUF = 3 * kTile + (KMASK || AMASK ? 1024 : 0);
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hl = lane >> 5, c32 = lane & 31;
  int tile, bh;
  tile_of_block(CAUSAL, true, tile, bh);
  const int b = bh / a.H, hh = bh - b * a.H;
  const int hk = GQA ? hh / a.G : hh;  // the key/value head this query head reads
  const int qb0 = tile * 128;
  [[maybe_unused]] int s0 = 0;
  if constexpr (VARLEN) {
    if (!varlen_seq(a.cu, b, a.T, a.Sq, qb0, s0, Sq)) return;
    Sk = Sq;
  }
  const int q = qb0 + wid * 32 + c32;
  const int qq = q < Sq ? q : Sq - 1;
  const uint32_t dbase = DROP ? drop_base(a.seed, (uint32_t)bh) + (uint32_t)q * kDropQ +
                                    (uint32_t)hl * kDropK
                              : 0u;
  const T* K = static_cast<const T*>(a.k) + seq_off<VARLEN>(b, s0, a.ksb, a.kss) + hk * a.ksh;
  const T* V = static_cast<const T*>(a.v) + seq_off<VARLEN>(b, s0, a.vsb, a.vss) + hk * a.vsh;

  v8 qf[8], of[8];
  {
    const T* Qp = static_cast<const T*>(a.q) + seq_off<VARLEN>(b, s0, a.qsb, a.qss) + hh * a.qsh +
                  (int64_t)qq * a.qss;
    const T* Op = static_cast<const T*>(a.dout) + seq_off<VARLEN>(b, s0, a.dsb, a.dss) +
                  hh * a.dsh + (int64_t)qq * a.dss;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      qf[s] = *reinterpret_cast<const v8*>(Qp + 16 * s + 8 * hl);
      of[s] = *reinterpret_cast<const v8*>(Op + 16 * s + 8 * hl);
    }
  }
  const float lse_q = KMASK || AMASK ? lse_guard(a.lse[(int64_t)bh * a.lse_stride + qq])
                            : a.lse[(int64_t)bh * a.lse_stride + qq];
  // D = rowsum(dO * O) of this lane's query from the dO fragments already in registers
  // (the two 32-lane halves hold complementary d ranges), written for the dK/dV kernel
  float D_q;
  {
    const T* Opr = static_cast<const T*>(a.o) + seq_off<VARLEN>(b, s0, a.osb, a.oss) + hh * a.osh +
                   (int64_t)qq * a.oss;
    float part = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const v8 ov = *reinterpret_cast<const v8*>(Opr + 16 * s + 8 * hl);
#pragma unroll
      for (int j = 0; j < 8; ++j) part = fmaf((float)of[s][j], (float)ov[j], part);
    }
    D_q = part + __shfl_xor(part, 32);
    if constexpr (KMASK || AMASK) {  // D itself: refined at the end; here the guarded lse
      if (hl == 0 && q < Sq) a.D[((int64_t)a.B * a.H + bh) * a.lse_stride + q] = lse_q;
    } else {
      if (hl == 0 && q < Sq) a.D[(int64_t)bh * a.lse_stride + q] = D_q;
    }
  }

  int nkt = (Sk + kAKT - 1) / kAKT;
  if (CAUSAL) {
    const int last = (qb0 + 127 < Sq ? qb0 + 127 : Sq - 1) / kAKT + 1;
    nkt = last < nkt ? last : nkt;
  }
  const int lrow = lane >> 3, pch = lane & 7;
  uint32_t kro[2], kto[2], vro[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (wid * 2 + i) * 8 + lrow;
    const int chr = (swz_rows(row, pch) - row * kARow) >> 4;
    kro[i] = row_off<T>(row, a.kss, chr);
    kto[i] = row_off<T>(row, a.kss, (swz_tr(row, pch) - row * kARow) >> 4);
    vro[i] = row_off<T>(row, a.vss, chr);
  }
  // images per slot: 0 = K rows, 1 = K transposed, 2 = V rows[, bias]
  const float* kbias = KMASK ? a.kbias + (int64_t)b * kstride : nullptr;
  // AMASK: row `tile` of this batch element's mask words, 1 KiB per key tile
  const unsigned long long* wrow = AMASK ? a.wq + (b * a.mqs + (int64_t)tile * nkt) * 128 : nullptr;
  auto issue = [&](int kt, int buf) {
    unsigned char* base = lds + buf * BUF;
    if constexpr (KMASK) {  // lanes 0-15: bias[k0 .. k0+63], the rest pad (bias again)
      if (wid == 0) glds16(kbias + kt * kAKT + (lane & 15) * 4, base + 3 * kTile);
    }
    if constexpr (AMASK) {  // two words per lane: the tile's 128 queries
      if (wid == 0) glds16(wrow + kt * 128 + lane * 2, base + 3 * kTile);
    }
    if ((kt + 1) * kAKT <= Sk) {
      const T* kb = tile_base(K, kt * kAKT, a.kss);
      dma_tile<T>(kb, kro, base, wid);
      dma_tile<T>(kb, kto, base + kTile, wid);
      dma_tile<T>(tile_base(V, kt * kAKT, a.vss), vro, base + 2 * kTile, wid);
      return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (wid * 2 + i) * 8 + lrow;
      const int kr = kt * kAKT + row;
      const int kc = kr < Sk ? kr : Sk - 1;
      const int chr = (swz_rows(row, pch) - row * kARow) >> 4;
      const int cht = (swz_tr(row, pch) - row * kARow) >> 4;
      const T* krow = K + (int64_t)kc * a.kss;
      dma_row<T>(krow, chr, base, wid, i);
      dma_row<T>(krow, cht, base + kTile, wid, i);
      dma_row<T>(V + (int64_t)kc * a.vss, chr, base + 2 * kTile, wid, i);
    }
  };

  f32x16_t dq[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[dt][i] = 0.f;
  // KMASK: the sum over keys of this lane's dS, which refines the D handed to the dK/dV
  // kernel (attention.hip explains why)
  [[maybe_unused]] float dsum = 0.f;
  int koff[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 4; ++s) koff[t][s] = swz_rows(32 * t + c32, 2 * s + hl);
  int tlo[2][2][2], thi[2][2][2];  // [d tile & 1][key half][k step]
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int r0 = 32 * t + 16 * s + 4 * hl;
        const int c0 = 32 * dt + ((lane >> 4) & 1) * 16;
        tlo[dt][t][s] = tr_addr(r0, c0, lane);
        thi[dt][t][s] = tr_addr(r0 + 8, c0, lane);
      }

  // KMASK: kt walks the live tiles only (nx = the one after kt), the ring slot alternates;
  // AMASK: the same over the non-dead tiles of the classes, `full` the class of kt
  constexpr bool WALK = KMASK || AMASK;
  LiveTiles lt(KMASK ? a.klive + (int64_t)b * (kstride / kAKT) : nullptr, nkt, lane);
  PairTiles pt(AMASK ? a.cq + b * a.mqs + (int64_t)tile * nkt : nullptr, nkt, lane);
  [[maybe_unused]] bool full = false;
  auto next_tile = [&]() {
    if constexpr (AMASK) return pt.next();
    else return lt.next();
  };
  int nx = 0, slot = 0;
  if constexpr (WALK) {
    nx = next_tile();
    if (nx < nkt) issue(nx, 0);
  } else {
    issue(0, 0);
  }
  settle(qf);
  settle(of);
  for (int kt = WALK ? nx : 0; kt < nkt; kt = WALK ? nx : kt + 1) {
    if constexpr (AMASK) full = pt.full;
    if constexpr (WALK) nx = next_tile();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (WALK) {
      if (nx < nkt) issue(nx, slot ^ 1);
    } else {
      if (kt + 1 < nkt) issue(kt + 1, (kt + 1) & 1);
    }
    const unsigned char* base = lds + (WALK ? slot : (kt & 1)) * BUF;
    if constexpr (WALK) slot ^= 1;
    const unsigned char* Kr = base;
    const unsigned char* Kt = base + kTile;
    const unsigned char* Vr = base + 2 * kTile;
    const int k0 = kt * kAKT;
    if (CAUSAL && k0 > qb0 + wid * 32 + 31) continue;
    const uint32_t tb = dbase + (uint32_t)(k0 >> 2) * kDropK;
    // stages of one 32-key half t: S^T / dP^T products, dS^T, mask, dQ^T product
    auto sdp = [&](int t, f32x16_t& sc, f32x16_t& dp) {
#pragma unroll
      for (int i = 0; i < 16; ++i) sc[i] = dp[i] = 0.f;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        sc = mfma32<T>(row_frag<T>(Kr, koff[t], s), qf[s], sc);
        dp = mfma32<T>(row_frag<T>(Vr, koff[t], s), of[s], dp);
      }
    };
    auto dsoft = [&](int t, f32x16_t& sc, const f32x16_t& dp) {
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        uint32_t hsh = 0;
        // key quad (k0 + 32t + 8rq + 4hl) >> 2: a literal lattice step
        if (DROP) hsh = drop_mix(tb + (uint32_t)(8 * t + 2 * rq) * kDropK);
        float be[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (KMASK) {
          const float4 bv = *reinterpret_cast<const float4*>(
              reinterpret_cast<const float*>(base + 3 * kTile) + 32 * t + 8 * rq + 4 * hl);
          be[0] = bv.x; be[1] = bv.y; be[2] = bv.z; be[3] = bv.w;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * rq + e;
          float dpr = dp[r];
          if (DROP) dpr = drop_keep8(hsh, e, a.thr8) ? dpr * a.inv_keep : 0.f;
          if constexpr (KMASK) sc[r] = fexp2(fmaf(sc[r], a.scale_log2, be[e] - lse_q)) * (dpr - D_q);
          else sc[r] = fexp2(fmaf(sc[r], a.scale_log2, -lse_q)) * (dpr - D_q);
        }
      }
    };
    auto mask = [&](int t, f32x16_t& sc) {
      if constexpr (AMASK) {  // this lane's query against the half's 32 keys (0 past Sk)
        const uint2 w = pair_word(base + 3 * kTile, wid * 32 + c32, hl);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (!pair_bit(w, t, r)) sc[r] = 0.f;
        return;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = k0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hl;
        if (!(key < Sk && !(CAUSAL && key > q))) sc[r] = 0.f;
      }
    };
    auto accum = [&](int t, const f32x16_t& sc) {
      if constexpr (KMASK || AMASK) {
#pragma unroll
        for (int r = 0; r < 16; ++r) dsum += sc[r];
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const v8 sf = acc_frag<T>(sc, s);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          dq[dt] = mfma32<T>(lds_tr8<T>(Kt + (dt >> 1) * kImg, tlo[dt & 1][t][s], thi[dt & 1][t][s]),
                             sf, dq[dt]);
      }
    };
    f32x16_t sc0, dp0, sc1, dp1;
    sdp(0, sc0, dp0);
    sdp(1, sc1, dp1);
    // wave-uniform; unmasked tiles run as one straight-line block (half 0's dQ MFMAs
    // beside half 1's softmax VALU)
    // (AMASK: a full tile needs none, a mixed one is masked by its bits)
    const bool need_mask =
        AMASK ? !full : (k0 + kAKT > Sk) || (CAUSAL && k0 + kAKT - 1 > qb0 + wid * 32);
    if (!need_mask) {
      dsoft(0, sc0, dp0);
      accum(0, sc0);
      dsoft(1, sc1, dp1);
      accum(1, sc1);
    } else {
      dsoft(0, sc0, dp0);
      dsoft(1, sc1, dp1);
      mask(0, sc0);
      mask(1, sc1);
      accum(0, sc0);
      accum(1, sc1);
    }
  }
  if constexpr (KMASK || AMASK) {
    const float dD = dsum + __shfl_xor(dsum, 32);  // the two halves hold 32 keys each per tile
    if (hl == 0 && q < Sq) a.D[(int64_t)bh * a.lse_stride + q] = D_q + dD;
  }
  if (q < Sq)
    store_dT128<T>(static_cast<T*>(a.dq) + seq_off<VARLEN>(b, s0, a.dqsb, a.dqss) +
                       (int64_t)q * a.dqss + hh * a.dqsh,
                   dq, hl, a.scale);
}

}  // namespace

#ifndef ATTN_KERNELS_ONLY  // attention_gqa.hip includes this file for the kernels alone
void attn_fwd_d128(const AttnProblem& p, void* o, float* lse, hipStream_t st) {
  AttnArgs a = kernel_args<AttnArgs>("attn_fwd", p);
  a.o = o; a.lse = lse;
  dim3 grid((p.Sq + 127) / 128, p.B * p.H), block(kAT);
  if (p.wq != nullptr) {
    dispatch_amask(p, a.thr8 != 0, [&](auto t, auto d) {
      hipLaunchKernelGGL((ATTN_AMASK_KERNEL(attn128_fwd_k)), grid, block, 0, st, a);
    });
    return;
  }
  dispatch(p, a.thr8 != 0, [&](auto t, auto c, auto d, auto m, auto vl) {
    hipLaunchKernelGGL((ATTN_KERNEL(attn128_fwd_k)), grid, block, 0, st, a);
  });
}

void attn_bwd_d128(const AttnProblem& p, const AttnBwd& g, hipStream_t st) {
  AttnBwdArgs a = bwd_kernel_args("attn_bwd", p, g);
  // dQ owns 128-query tiles, dK/dV 128-key tiles; dQ first (it writes D), then dK/dV
  dim3 qgrid((p.Sq + 127) / 128, p.B * p.H), kgrid((p.Sk + 127) / 128, p.B * p.H), block(kAT);
  if (p.wq != nullptr) {
    dispatch_amask(p, a.thr8 != 0, [&](auto t, auto d) {
      hipLaunchKernelGGL((ATTN_AMASK_KERNEL(attn128_bwd_dq_k)), qgrid, block, 0, st, a);
      hipLaunchKernelGGL((ATTN_AMASK_KERNEL(attn128_bwd_dkdv_k)), kgrid, block, 0, st, a);
    });
    return;
  }
  dispatch(p, a.thr8 != 0, [&](auto t, auto c, auto d, auto m, auto vl) {
    hipLaunchKernelGGL((ATTN_KERNEL(attn128_bwd_dq_k)), qgrid, block, 0, st, a);
    hipLaunchKernelGGL((ATTN_KERNEL(attn128_bwd_dkdv_k)), kgrid, block, 0, st, a);
  });
}
#undef ATTN_KERNEL
#undef ATTN_AMASK_KERNEL
#undef ATTN_GQA_KERNEL
#endif  // ATTN_KERNELS_ONLY

}  // namespace amd
