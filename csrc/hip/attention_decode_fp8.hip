// Fused attention decode step over an FP8 (OCP e4m3, torch.float8_e4m3fn) KV cache with one
// fp32 scale per (batch element, key/value head, key), for gfx950 (head dim 64 / 128, q and o
// in bf16 / fp16, forward only).  Key j of head hk is k_cache[b][j][hk][:] * k_scale[b][hk][j],
// values alike.  A decode step is bound by K/V bytes (attention_decode.hip); this file halves
// them.  The work split is that kernel's - the R = G * Sq rows of a (batch element, key/value
// head) are the 32 columns of the swapped S^T = K . Q^T MFMA, four waves stream their own slot
// tiles on per-wave global_load_lds slots ordered by wave-local s_waitcnt (no workgroup barrier
// in the key loop), nsplit workgroups per cache write fp32 partials that attn_decode_combine
// joins in split order, lengths are read on the device, no atomics - and so are the softmax,
// the wave merge and the epilogue.  What is this file's own:
//
// Slot geometry.  A row is D bytes, so the 8 KiB K image and the 8 KiB V image of a slot hold
//   KS = 128 keys at D = 64 and 64 keys at D = 128: twice the keys in flight per wave for the
//   same LDS.  Both images are plain [KS][D bytes] rows (at D = 64 a 64-byte-row image) whose
//   16-byte chunks are permuted per key (below).  One global_load_lds_dwordx4 fills 1024
//   bytes (16 rows at D = 64, 8 at D = 128): 8 per image.  Behind the images a slot carries
//   the tile's K and V scales, KS floats each, one global_load_lds_dword per 64 keys (lane =
//   key).  NDMA = 16 + 2 KS / 64 = 20 (D = 64) / 18 (D = 128) instructions per slot is what
//   the loop's s_waitcnt vmcnt(NDMA) counts; no other vector load stands in the loop.
//   4 waves x 2 slots x (16 KiB + 8 KS) = 136 / 132 KiB of the CU's 160.
// Split ranges.  Splits own 64-key tiles exactly as in attn_decode_k (the host's split choice
//   and the workspace are shared), so a 128-key slot can reach past its split's end kend =
//   min(te * 64, L).  Every slot is bounded at kend, not at L: rows at or past kend are
//   loaded from row kend - 1 (bytes and scales; no byte at or past L is ever read, so a NaN
//   byte 0x7F or a NaN scale in the tail cannot reach o) and masked: a row's last key is
//   min(L - Sq + i, kend - 1).  A key is counted by the one split whose tile range holds it.
// Operands.  Q and P stay 16-bit and the MFMAs are v_mfma_f32_32x32x16_{bf16,f16}; FP8
//   becomes T in registers after the LDS read with v_cvt_scalef32_pk_{bf16,f16}_fp8 at scale
//   1.0 (exact: 3 mantissa bits, |x| <= 448), one VALU instruction per pair.
//   K: a lane reads 16 consecutive bytes of its key (ds_read_b128) and feeds two MFMA steps,
//   so MFMA step 2u + v of lane half hl holds d = 32u + 16hl + 8v + j; the Q fragments are
//   loaded in that order.  Chunk c of key r lies at chunk c ^ ((r >> 2) & 3) (D = 64) or
//   c ^ ((r >> 1) & 7) (D = 128): the 16 lanes of a ds_read_b128 pass (16 consecutive keys,
//   one logical chunk) then cover all 64 banks.
//   V: read transposed with ds_read_tr8_b64 (ds_read_b64_tr_b8), chosen over row reads plus
//   byte permutes because it delivers the A fragment as is: 16 reads per slot instead of 128
//   byte gathers.  Its lane mapping differs from ds_read_tr16_b64's and was measured on an
//   MI355X: within a 16-lane group the lanes' 8-byte pieces form an 8 x 16 byte matrix, lane
//   2r + h supplying columns 8h .. 8h + 7 of row r, and lane i receives column i, rows 0 .. 7.
//   The 8 rows are the keys of a P fragment (acc_frag: 16s + 4hl + {0..3, 8..11}), each
//   supplied from its own address, so P needs no shuffle.  Chunk c of key r lies at
//   c ^ (2 * ((r >> 3) & 1)) (D = 64) or c ^ (2 * ((r >> 1) & 1) + 4 * ((r >> 3) & 1)) (D =
//   128), which spreads the 8 keys x 2 chunks of a 32-lane pass over distinct banks (reasoned
//   from the bank layout, not measured).
// Scales.  A lane owns one row's scores and a register is a key; registers 4g .. 4g + 3 are 4
//   consecutive keys, so a slot's scales are read as broadcast ds_read_b128.  The K scale
//   times scale_log2 multiplies the score (one multiply per key and lane folds the two); the
//   V scale multiplies p after psum is taken and before acc_frag rounds to 16 bits.
// Append.  attn_fp8_append_k quantises k_new / v_new [B, Sn, Hkv, D] into rows
//   cache_seqlens[b] + i (rows outside [0, Smax) are skipped): D / 8 lanes per row, one
//   16-byte load each, a cross-lane max, scale = amax / 448 (IEEE division; 1.0 for an
//   all-zero row), byte = e4m3_rne(clamp(x / scale, -448, 448)) by v_cvt_pk_fp8_f32 with the
//   clamp in plain C++ before it, one 8-byte store per lane and one scale store per row.
//   torch's (x.float() / s).clamp(-448, 448).to(float8_e4m3fn) gives the same bytes.
//
// Resources (hipcc -O3 gfx950 resource report) and timings: docs/PERF.md, "Attention: decode
// over an FP8 KV cache".
#include "attention_common.h"

namespace amd {

namespace {

struct Fp8Args {
  const void* q;
  const unsigned char* k;
  const unsigned char* v;
  const float* ks;
  const float* vs;
  int64_t qsb, qss, qsh;                    // element strides
  int64_t ksb, kss, ksh, vsb, vss, vsh;     // byte strides
  int64_t kcb, kch, vcb, vch;               // scale strides (floats): batch, head
  const int* lens;   // [B] keys in the cache before the call
  int append;        // 1: the Sq new rows are in the cache behind lens[b]
  void* o;           // [B][Sq][H][D], written when nsplit == 1
  float* lse;        // [B][H][Sq], written when nsplit == 1
  float* o_part;     // [nsplit][B][Sq][H][D] normalised fp32 partials (nsplit > 1)
  float* lse_part;   // [nsplit][B][H][Sq]
  int B, H, Hkv, G, Sq, Smax, R;  // R = G * Sq rows per (b, key/value head)
  float scale_log2;
};

// attention_decode.hip's decode_len: the visible length, clipped to the rows the views hold
__device__ __forceinline__ int fp8_len(const int* lens, int b, int append, int Sq, int Smax) {
  int l = lens[b];
  l = l < 0 ? 0 : (l > Smax ? Smax : l);
  l += append ? Sq : 0;
  return l > Smax ? Smax : l;
}

template <typename T, int D>
__global__ void __launch_bounds__(kAT) attn_decode_fp8_k(Fp8Args a) {
  typedef typename Frag<T>::v8 v8;
  constexpr int IMG = 8192;              // bytes of the K (or V) image of a slot tile
  constexpr int KS = IMG / D;            // keys per slot tile: 128 (D = 64), 64 (D = 128)
  constexpr int NT = KS / 32;            // score accumulators per slot tile
  constexpr int NC = D / 16;             // 16-byte chunks per row
  constexpr int RPI = 1024 / D;          // rows one dwordx4 DMA instruction fills
  constexpr int NKV = IMG / 1024;        // ... and instructions per image: 8
  constexpr int NSC = KS / 64;           // dword DMA instructions per scale row
  constexpr int SLOT = 2 * IMG + 2 * KS * 4;  // K, V, K scales, V scales
  constexpr int NDMA = 2 * NKV + 2 * NSC;     // DMA instructions per slot tile
  static_assert(NDMA == (D == 64 ? 20 : 18) && NDMA < 64,
                "the s_waitcnt vmcnt(NDMA) below counts one slot and fits the 6-bit counter");
  constexpr int WAVE = 2 * SLOT;         // a wave's two slots
  static_assert(WAVE >= (D * 32 + 64) * 4, "a wave's merge state fits its own slots");
  static_assert(4 * WAVE <= 160 * 1024, "four waves' slots fit the CU's LDS");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[4 * WAVE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hl = lane >> 5, c32 = lane & 31;
  const int split = blockIdx.x, nsplit = gridDim.x;
  const int b = blockIdx.z / a.Hkv, hk = blockIdx.z - b * a.Hkv;
  const int Sq = a.Sq, R = a.R;
  const int L = fp8_len(a.lens, b, a.append, Sq, a.Smax);

  // this split's 64-key tiles [tb, te) of the ceil(L / 64): attn_decode_k's ranges
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
  const int kbeg = tb * kAKT;
  const int kend = te * kAKT < L ? te * kAKT : L;  // >= 1: the bound of every load and score

  // this lane's row in the key loop (clamped: rows past R repeat row R - 1, never stored)
  const int r = blockIdx.y * 32 + c32;
  const int rr = r < R ? r : R - 1;
  const int g = rr / Sq, qi = rr - g * Sq;
  const int lim = L - Sq + qi < kend - 1 ? L - Sq + qi : kend - 1;  // the last key this row counts
  const int mfree = L - Sq < kend - 1 ? L - Sq : kend - 1;  // keys up to here: no row masks them
  const T* Q = static_cast<const T*>(a.q) + b * a.qsb + (int64_t)qi * a.qss + (hk * a.G + g) * a.qsh;
  const unsigned char* K = a.k + b * a.ksb + hk * a.ksh;
  const unsigned char* V = a.v + b * a.vsb + hk * a.vsh;
  const float* KSc = a.ks + b * a.kcb + hk * a.kch;
  const float* VSc = a.vs + b * a.vcb + hk * a.vch;

  v8 qf[D / 16];  // Q^T fragments, loaded behind the first slot's DMA (below)

  // DMA: instruction i fills bytes [1024 i, 1024 i + 1024) of an image; lane = (row in the RPI,
  // physical chunk), which holds the row's logical chunk pch ^ swizzle(row)
  const int drow = lane / NC, pch = lane % NC;
  uint32_t kof[NKV], vof[NKV];
#pragma unroll
  for (int i = 0; i < NKV; ++i) {
    const int row = RPI * i + drow;
    kof[i] = (uint32_t)row * (uint32_t)a.kss + (uint32_t)(swz_k8<D>(row, pch) - row * D);
    vof[i] = (uint32_t)row * (uint32_t)a.vss + (uint32_t)(swz_v8<D>(row, pch) - row * D);
  }
  unsigned char* const wlds = lds + wid * WAVE;
  auto issue = [&](int k0, int slot) {  // keys k0 .. k0 + KS - 1 -> slot, bounded at kend
    unsigned char* Kl = wlds + slot * SLOT;
    unsigned char* Vl = Kl + IMG;
    unsigned char* Sl = Vl + IMG;  // KS K scales, then KS V scales
#pragma unroll
    for (int j = 0; j < NSC; ++j) {  // lane = key; at or past kend: key kend - 1's scale
      const int key = k0 + 64 * j + lane;
      const uint32_t off = (uint32_t)(key < kend ? key : kend - 1) * 4u;
      glds4o(KSc, off, Sl + 256 * j);
      glds4o(VSc, off, Sl + KS * 4 + 256 * j);
    }
    if (k0 + KS <= kend) {
      const unsigned char* kb = K + (int64_t)k0 * a.kss;
      const unsigned char* vb = V + (int64_t)k0 * a.vss;
#pragma unroll
      for (int i = 0; i < NKV; ++i) {
        glds16o(kb, kof[i], Kl + i * 1024);
        glds16o(vb, vof[i], Vl + i * 1024);
      }
      return;
    }
    // the tile reaches past kend: rows at or past it read row kend - 1
#pragma unroll
    for (int i = 0; i < NKV; ++i) {
      const int row = RPI * i + drow;
      const int key = k0 + row;
      const int kk = key < kend ? key : kend - 1;
      glds16(K + (int64_t)kk * a.kss + (swz_k8<D>(row, pch) - row * D), Kl + i * 1024);
      glds16(V + (int64_t)kk * a.vss + (swz_v8<D>(row, pch) - row * D), Vl + i * 1024);
    }
  };

  f32x16_t o[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
  float m = -INFINITY, l = 0.f;

  // loop-invariant LDS offsets.  K: key 32t + c32, chunk 2u + hl (the swizzle does not see
  // 32t).  V: the piece this lane supplies to its 16-lane group's transposed read of keys
  // 32t + 16s + 4hl + {0..3, 8..11} x d columns 32dt + 16 (lane / 16 % 2) + 0 .. 15: row
  // (lane % 16) / 2 of the 8, bytes 8 (lane % 2) .. + 7 (the swizzle does not see 32t + 16s)
  int koff[D / 32], voff[D / 32];
#pragma unroll
  for (int u = 0; u < D / 32; ++u) koff[u] = swz_k8<D>(c32, 2 * u + hl);
  {
    const int i = lane & 15, q = i >> 1;
    const int key = 4 * hl + (q & 3) + 8 * (q >> 2);
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
      voff[dt] = swz_v8<D>(key, 2 * dt + ((lane >> 4) & 1)) + 8 * (i & 1);
  }

  auto step = [&](int k0, int slot) {
    const unsigned char* Kl = wlds + slot * SLOT;
    const unsigned char* Vl = Kl + IMG;
    const unsigned char* Sl = Vl + IMG;
    f32x16_t x[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int i = 0; i < 16; ++i) x[t][i] = 0.f;
#pragma unroll
      for (int u = 0; u < D / 32; ++u) {
        const uint4 kw = *reinterpret_cast<const uint4*>(Kl + koff[u] + 32 * t * D);
        x[t] = mfma32<T>(fp8_frag<T>(kw.x, kw.y), qf[2 * u], x[t]);
        x[t] = mfma32<T>(fp8_frag<T>(kw.z, kw.w), qf[2 * u + 1], x[t]);
      }
    }
    // scores in log2 units, times the key's scale; only a tile that reaches past key
    // min(L - Sq, kend - 1) tests the mask (wave-uniform)
    const bool need_mask = k0 + KS - 1 > mfree;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const float4 sc = *reinterpret_cast<const float4*>(Sl + (32 * t + 8 * gq + 4 * hl) * 4);
        const float s4[4] = {sc.x, sc.y, sc.z, sc.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int key = k0 + 32 * t + 8 * gq + 4 * hl + e;
          const int rg = 4 * gq + e;
          x[t][rg] = need_mask && key > lim ? -INFINITY : x[t][rg] * (s4[e] * a.scale_log2);
        }
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
    // p times the value's scale (a masked key: 0 times a loaded, finite scale)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const float4 sc =
            *reinterpret_cast<const float4*>(Sl + (KS + 32 * t + 8 * gq + 4 * hl) * 4);
        x[t][4 * gq] *= sc.x;
        x[t][4 * gq + 1] *= sc.y;
        x[t][4 * gq + 2] *= sc.z;
        x[t][4 * gq + 3] *= sc.w;
      }
    // O^T[d][row] += V^T[d][key] . P^T[key][row]
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const v8 pf = acc_frag<T>(x[t], s);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) {
          const v2i_t vw = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
              (__attribute__((address_space(3))) v2i_t*)(Vl + voff[dt] + (32 * t + 16 * s) * D));
          o[dt] = mfma32<T>(fp8_frag<T>((uint32_t)vw.x, (uint32_t)vw.y), pf, o[dt]);
        }
      }
  };

  // this wave's slot tiles: k0 = kbeg + (wid + 4 n) KS below kend, double buffered; a slot's
  // NDMA DMA instructions retire in order, so vmcnt(NDMA) is "the older slot has landed"
  int k0 = kbeg + wid * KS;
  if (k0 < kend) issue(k0, 0);
  // Q^T fragments (B operand of S^T = K . Q^T) in the K reads' order: step 2u + v holds d =
  // 32u + 16hl + 8v + j.  The empty asm is a use the compiler must wait for HERE, once: left to
  // itself it waits for these loads inside the loop, and its vmcnt(0) there also waits out the
  // slot that was just issued.
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    qf[s] = *reinterpret_cast<const v8*>(Q + 32 * (s >> 1) + 16 * hl + 8 * (s & 1));
#pragma unroll
  for (int s = 0; s < D / 16; ++s) asm volatile("" : "+v"(qf[s]));
  for (int slot = 0; k0 < kend; k0 += 4 * KS, slot ^= 1) {
    if (k0 + 4 * KS < kend) {
      issue(k0 + 4 * KS, slot ^ 1);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");
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

struct Fp8AppendArgs {
  const void* kn;
  const void* vn;
  unsigned char* kc;
  unsigned char* vc;
  float* ks;
  float* vs;
  int64_t knsb, knss, knsh, vnsb, vnss, vnsh;  // element strides
  int64_t kcsb, kcss, kcsh, vcsb, vcss, vcsh;  // byte strides
  int64_t kcb, kch, vcb, vch;                  // scale strides (floats): batch, head
  const int* lens;
  int B, Sn, Hkv, Smax;
};

// One row by LPR lanes of 8 elements each: the row's amax across the lanes, its scale, this
// lane's 8 bytes.  The arithmetic is the one torch mirrors (header): IEEE divisions, the clamp
// in C++, round-to-nearest-even in the convert.
template <typename T, int LPR>
__device__ __forceinline__ void fp8_quant_row(const T* src, unsigned char* dst, float* scale,
                                              bool first) {
  const typename Frag<T>::v8 xv = *reinterpret_cast<const typename Frag<T>::v8*>(src);
  float x[8], amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    x[j] = (float)xv[j];
    amax = fmaxf(amax, fabsf(x[j]));
  }
#pragma unroll
  for (int mask = LPR / 2; mask > 0; mask >>= 1) amax = fmaxf(amax, __shfl_xor(amax, mask));
  const float s = amax > 0.f ? __fdiv_rn(amax, 448.f) : 1.f;
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) y[j] = fminf(fmaxf(__fdiv_rn(x[j], s), -448.f), 448.f);
  uint2 w;
  w.x = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  w.x = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], (int)w.x, true);
  w.y = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
  w.y = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], (int)w.y, true);
  *reinterpret_cast<uint2*>(dst) = w;
  if (first) *scale = s;
}

// D / 8 threads per new K and V row: k_new[b][i][h] -> k_cache[b][lens[b] + i][h] and
// k_scale[b][h][lens[b] + i].  A row's threads are an aligned lane group of one wave and leave
// together.
template <typename T, int D>
__global__ void __launch_bounds__(256) attn_fp8_append_k(Fp8AppendArgs a) {
  constexpr int LPR = D / 8;
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = id / LPR;  // (b * Sn + i) * Hkv + h
  if (row >= (int64_t)a.B * a.Sn * a.Hkv) return;
  const int c = (int)(id - row * LPR) * 8;
  const int h = (int)(row % a.Hkv);
  const int64_t bi = row / a.Hkv;
  const int i = (int)(bi % a.Sn), b = (int)(bi / a.Sn);
  const int len = a.lens[b];
  if (len < 0 || len >= a.Smax - i) return;  // the row lies outside the cache views
  const int pos = len + i;
  fp8_quant_row<T, LPR>(static_cast<const T*>(a.kn) + b * a.knsb + i * a.knss + h * a.knsh + c,
                        a.kc + b * a.kcsb + (int64_t)pos * a.kcss + h * a.kcsh + c,
                        a.ks + b * a.kcb + h * a.kch + pos, c == 0);
  fp8_quant_row<T, LPR>(static_cast<const T*>(a.vn) + b * a.vnsb + i * a.vnss + h * a.vnsh + c,
                        a.vc + b * a.vcsb + (int64_t)pos * a.vcss + h * a.vcsh + c,
                        a.vs + b * a.vcb + h * a.vch + pos, c == 0);
}

template <typename T, int D>
void launch_fp8(const AttnDecode& p, const Fp8Args& a, hipStream_t st) {
  const int nyb = (a.R + 31) / 32;
  dim3 grid((unsigned)p.nsplit, (unsigned)nyb, (unsigned)(p.B * p.Hkv)), block(kAT);
  hipLaunchKernelGGL((attn_decode_fp8_k<T, D>), grid, block, 0, st, a);
}

template <typename T, int D>
void launch_fp8_append(const Fp8AppendArgs& c, hipStream_t st) {
  const int64_t threads = (int64_t)c.B * c.Sn * c.Hkv * (D / 8);
  dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  hipLaunchKernelGGL((attn_fp8_append_k<T, D>), grid, block, 0, st, c);
}

}  // namespace

void attn_fp8_append(const AttnDecodeFp8& p, int Sn, hipStream_t st) {
  const AttnDecode& d = p.d;
  if ((d.D != 64 && d.D != 128) || d.k_new.p == nullptr || d.v_new.p == nullptr ||
      p.k_scale == nullptr || p.v_scale == nullptr ||
      (d.dtype != DType::BF16 && d.dtype != DType::F16)) {
    fprintf(stderr, "attn_fp8_append: head dim 64 or 128, bf16 / fp16 rows, both new tensors and "
                    "both scale tensors, got D = %d\n", d.D);
    abort();
  }
  if (d.B <= 0 || Sn <= 0 || d.Hkv <= 0) return;
  Fp8AppendArgs c{};
  c.kn = d.k_new.p; c.knsb = d.k_new.sb; c.knss = d.k_new.ss; c.knsh = d.k_new.sh;
  c.vn = d.v_new.p; c.vnsb = d.v_new.sb; c.vnss = d.v_new.ss; c.vnsh = d.v_new.sh;
  c.kc = static_cast<unsigned char*>(d.k.p); c.kcsb = d.k.sb; c.kcss = d.k.ss; c.kcsh = d.k.sh;
  c.vc = static_cast<unsigned char*>(d.v.p); c.vcsb = d.v.sb; c.vcss = d.v.ss; c.vcsh = d.v.sh;
  c.ks = p.k_scale; c.kcb = p.ks_sb; c.kch = p.ks_sh;
  c.vs = p.v_scale; c.vcb = p.vs_sb; c.vch = p.vs_sh;
  c.lens = d.cache_seqlens;
  c.B = d.B; c.Sn = Sn; c.Hkv = d.Hkv; c.Smax = d.Smax;
  if (d.dtype == DType::BF16) {
    if (d.D == 64) launch_fp8_append<bf16_t, 64>(c, st);
    else launch_fp8_append<bf16_t, 128>(c, st);
  } else {
    if (d.D == 64) launch_fp8_append<half_t, 64>(c, st);
    else launch_fp8_append<half_t, 128>(c, st);
  }
}

void attn_decode_fp8(const AttnDecodeFp8& p, void* o, float* lse, hipStream_t st) {
  const AttnDecode& d = p.d;
  if (d.D != 64 && d.D != 128) {
    fprintf(stderr, "attn_decode_fp8: head dim must be 64 or 128, got %d\n", d.D);
    abort();
  }
  if (d.Hkv <= 0 || d.H % d.Hkv != 0) {
    fprintf(stderr, "attn_decode_fp8: %d query heads do not split over %d key/value heads\n",
            d.H, d.Hkv);
    abort();
  }
  if (p.k_scale == nullptr || p.v_scale == nullptr) {
    fprintf(stderr, "attn_decode_fp8: an FP8 cache comes with its k_scale and v_scale\n");
    abort();
  }
  if (d.nsplit < 1 || d.nsplit > kAttnDecodeMaxSplits ||
      (d.nsplit > 1 && (d.o_part == nullptr || d.lse_part == nullptr))) {
    fprintf(stderr, "attn_decode_fp8: nsplit = %d needs 1 .. %d and, above 1, the workspace\n",
            d.nsplit, kAttnDecodeMaxSplits);
    abort();
  }
  if (d.B <= 0 || d.Sq <= 0) return;
  if (d.k_new.p != nullptr) attn_fp8_append(p, d.Sq, st);
  Fp8Args a{};
  a.q = d.q.p; a.qsb = d.q.sb; a.qss = d.q.ss; a.qsh = d.q.sh;
  a.k = static_cast<const unsigned char*>(d.k.p); a.ksb = d.k.sb; a.kss = d.k.ss; a.ksh = d.k.sh;
  a.v = static_cast<const unsigned char*>(d.v.p); a.vsb = d.v.sb; a.vss = d.v.ss; a.vsh = d.v.sh;
  a.ks = p.k_scale; a.kcb = p.ks_sb; a.kch = p.ks_sh;
  a.vs = p.v_scale; a.vcb = p.vs_sb; a.vch = p.vs_sh;
  a.lens = d.cache_seqlens;
  a.append = d.k_new.p != nullptr ? 1 : 0;
  a.o = o; a.lse = lse; a.o_part = d.o_part; a.lse_part = d.lse_part;
  a.B = d.B; a.H = d.H; a.Hkv = d.Hkv; a.G = d.H / d.Hkv; a.Sq = d.Sq; a.Smax = d.Smax;
  a.R = a.G * d.Sq;
  a.scale_log2 = d.scale * 1.4426950408889634f;
  if (d.dtype == DType::BF16) {
    if (d.D == 64) launch_fp8<bf16_t, 64>(d, a, st);
    else launch_fp8<bf16_t, 128>(d, a, st);
  } else {
    if (d.D == 64) launch_fp8<half_t, 64>(d, a, st);
    else launch_fp8<half_t, 128>(d, a, st);
  }
  if (d.nsplit > 1)
    attn_decode_combine(d.dtype, d.D, d.B, d.H, d.Sq, d.nsplit, d.o_part, d.lse_part, o, lse, st);
}

}  // namespace amd
