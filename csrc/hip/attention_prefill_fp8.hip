// Fused attention of a chunk of new tokens over an FP8 (OCP e4m3, torch.float8_e4m3fn) KV cache
// with one fp32 scale per (batch element, key/value head, key), for gfx950 (head dim 64 / 128, q
// and o in bf16 / fp16, forward only): chunked prefill, the next turn of a conversation, a prompt
// behind a shared prefix over the cache that attention_decode_fp8.hip decodes from.  Two files
// meet here; read their headers first.
//
// The row side is attn_prefill_k's (attention_prefill.hip): the R = G * Sq rows of a (batch
//   element, key/value head) token-major, r = i * G + g, 128 per workgroup, one row per lane
//   (the 32 columns of the swapped S^T = K . Q^T on v_mfma_f32_32x32x16); a workgroup's key loop
//   ends at the last key of its last token, a wave stops computing at its own last token's last
//   key (it keeps feeding the ring), only tiles that reach past the last key of the wave's first
//   row test the mask; a workgroup none of whose rows sees a key writes o = 0, lse = -inf and
//   returns before any DMA or barrier; grid (ceil(R / 128), Hkv, B) flattened with the heavy row
//   tiles first; one launch, no workspace, no atomics, bitwise reproducible.
// The operand side is attn_decode_fp8_k's: the cache contract (e4m3 bytes [B, Smax, Hkv, D] with
//   byte strides that are multiples of 16, scales [B, Hkv, Smax], key j of head hk = bytes *
//   k_scale[b, hk, j]), the per-key chunk permutations swz_k8 / swz_v8, K read as ds_read_b128
//   feeding two MFMA steps (so the Q fragments load in the order d = 32u + 16hl + 8v + j), V read
//   transposed with ds_read_tr8_b64 in the lane mapping that header documents, e4m3 -> T in
//   registers by fp8_frag (exact), 16-bit MFMAs, scales read as broadcast ds_read_b128, the K
//   scale times scale_log2 on the score, the V scale on p after psum and before acc_frag rounds.
//
// What is this file's own:
//
// Shared byte tiles.  The four waves share each 64-key tile.  An operand's tile is one plain
//   [64][D bytes] image (4 KiB at D = 64, 8 KiB at D = 128); behind the K and the V image a
//   buffer carries the tile's 64 K scales and 64 V scales (512 B).  Double buffered: 17 KiB /
//   33 KiB of LDS, about half of attn_prefill_k's 32 / 64 KiB.  Each wave fills rows 16 wid ..
//   16 wid + 15 of both images with global_load_lds_dwordx4 (1024 bytes each: one instruction
//   per operand at D = 64, two at D = 128); wave 0 adds the K scales and wave 1 the V scales
//   with one global_load_lds_dword each (lane = key).  The ring is attn_prefill_k's: s_waitcnt
//   vmcnt(0) + one barrier per tile, the refill of the other buffer after the barrier.
// Conversions.  Every wave converts the whole K and V tile for its own 32 rows (D / 2 + D / 2
//   v_cvt_scalef32_pk per lane and tile, four times what one cooperative pass into a 16-bit LDS
//   tile would take, which in turn costs an LDS round trip and a barrier).  Only this variant is
//   built; docs/PERF.md, "Attention: chunked prefill over an FP8 KV cache".
// Softmax.  The scales differ per key, so attn_prefill_k's unmasked fast path (max on the raw
//   scores, one fma per score) does not carry over: an unmasked tile multiplies, takes the max
//   and exponentiates; a masked tile tests key > lim as well and takes the -inf-safe offset.
// Tail.  A tile that reaches past L_b clamps the row addresses AND the scale addresses to L_b -
//   1, and the mask covers those keys (every row's last key lies below L_b).  No byte or scale
//   at or past L_b is ever loaded: a NaN byte 0x7F or a NaN scale there cannot reach o.
// Append.  attn_fp8_append (attention_decode_fp8.hip) quantises k_new / v_new first, on the same
//   stream; the chunk then attends the quantised rows, its own included.
//
// Resources (hipcc -O3 gfx950 resource report) and timings: docs/PERF.md, same section.
#include "attention_common.h"

namespace amd {

namespace {

struct PrefillFp8Args {
  const void* q;
  const unsigned char* k;
  const unsigned char* v;
  const float* ks;
  const float* vs;
  int64_t qsb, qss, qsh;                 // element strides
  int64_t ksb, kss, ksh, vsb, vss, vsh;  // byte strides
  int64_t kcb, kch, vcb, vch;            // scale strides (floats): batch, head
  const int* lens;  // [B] keys in the cache before the call
  int append;       // 1: the Sq new rows are in the cache behind lens[b]
  void* o;          // [B][Sq][H][D]
  float* lse;       // [B][H][Sq]
  int H, Hkv, G, Sq, Smax, R;  // R = G * Sq rows per (b, key/value head)
  float scale_log2;
};

// attention_decode.hip's decode_len: the visible length, clipped to the rows the views hold
__device__ __forceinline__ int prefill_fp8_len(const int* lens, int b, int append, int Sq,
                                               int Smax) {
  int l = lens[b];
  l = l < 0 ? 0 : (l > Smax ? Smax : l);
  l += append ? Sq : 0;
  return l > Smax ? Smax : l;
}

template <typename T, int D>
__global__ void __launch_bounds__(kAT, 2) attn_prefill_fp8_k(PrefillFp8Args a) {
  typedef typename Frag<T>::v8 v8;
  constexpr int IMG = kAKT * D;          // bytes of the K (or V) image of a tile
  constexpr int NC = D / 16;             // 16-byte chunks per row
  constexpr int RPI = 1024 / D;          // rows one dwordx4 DMA instruction fills
  constexpr int NW = 16 / RPI;           // ... and instructions per wave and image: 1 / 2
  constexpr int BUF = 2 * IMG + 2 * kAKT * 4;  // K, V, K scales, V scales
  static_assert(2 * BUF == (D == 64 ? 17 : 33) * 1024, "the header's LDS figure");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * BUF];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hl = lane >> 5, c32 = lane & 31;
  // block -> (row tile, b, key/value head), heavy tiles first (attention_prefill.hip, "Launch")
  const int nt = gridDim.x, nbh = gridDim.y * gridDim.z;
  const int id = blockIdx.x + nt * (blockIdx.y + gridDim.y * blockIdx.z);
  const int td = id / nbh, bh = id - td * nbh;
  const int tile = nt - 1 - td;
  const int b = bh / a.Hkv, hk = bh - b * a.Hkv;
  const int Sq = a.Sq, R = a.R, G = a.G;
  const int L = prefill_fp8_len(a.lens, b, a.append, Sq, a.Smax);

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
  const unsigned char* K = a.k + b * a.ksb + hk * a.ksh;
  const unsigned char* V = a.v + b * a.vsb + hk * a.vsh;
  const float* KSc = a.ks + b * a.kcb + hk * a.kch;
  const float* VSc = a.vs + b * a.vcb + hk * a.vch;

  // DMA: this wave's instruction i fills bytes [1024 (NW wid + i), + 1024) of an image, rows 16
  // wid + RPI i .. + RPI - 1; lane = (row in the RPI, physical chunk), which holds the row's
  // logical chunk pch ^ swizzle(row)
  const int drow = lane / NC, pch = lane % NC;
  uint32_t kof[NW], vof[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int row = 16 * wid + RPI * i + drow;
    kof[i] = (uint32_t)row * (uint32_t)a.kss + (uint32_t)(swz_k8<D>(row, pch) - row * D);
    vof[i] = (uint32_t)row * (uint32_t)a.vss + (uint32_t)(swz_v8<D>(row, pch) - row * D);
  }
  auto issue = [&](int kt, int buf) {
    unsigned char* Kl = lds + buf * BUF;
    unsigned char* Vl = Kl + IMG;
    unsigned char* Sl = Vl + IMG;  // 64 K scales, then 64 V scales
    const int k0 = kt * kAKT;
    if (wid < 2) {  // lane = key; at or past L: key L - 1's scale (L >= kend >= 1 here)
      const int key = k0 + lane;
      const uint32_t off = (uint32_t)(key < L ? key : L - 1) * 4u;
      if (wid == 0) glds4o(KSc, off, Sl);
      else glds4o(VSc, off, Sl + kAKT * 4);
    }
    if (k0 + kAKT <= L) {
      const unsigned char* kb = K + (int64_t)k0 * a.kss;
      const unsigned char* vb = V + (int64_t)k0 * a.vss;
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        glds16o(kb, kof[i], Kl + (NW * wid + i) * 1024);
        glds16o(vb, vof[i], Vl + (NW * wid + i) * 1024);
      }
      return;
    }
    // the tile reaches past L: rows at or past L read row L - 1
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int row = 16 * wid + RPI * i + drow;
      const int key = k0 + row;
      const int kk = key < L ? key : L - 1;
      glds16(K + (int64_t)kk * a.kss + (swz_k8<D>(row, pch) - row * D),
             Kl + (NW * wid + i) * 1024);
      glds16(V + (int64_t)kk * a.vss + (swz_v8<D>(row, pch) - row * D),
             Vl + (NW * wid + i) * 1024);
    }
  };

  f32x16_t o[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
  float m = -INFINITY, l = 0.f;

  // loop-invariant LDS offsets, attn_decode_fp8_k's.  K: key 32t + c32, chunk 2u + hl (the
  // swizzle does not see 32t).  V: the piece this lane supplies to its 16-lane group's
  // transposed read of keys 32t + 16s + 4hl + {0..3, 8..11} x d columns 32dt + 16 (lane / 16 %
  // 2) + 0 .. 15: row (lane % 16) / 2 of the 8, bytes 8 (lane % 2) .. + 7 (the swizzle does not
  // see 32t + 16s)
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

  v8 qf[D / 16];  // Q^T fragments, loaded behind the first tile's DMA (below)

  auto step = [&](int kt, int buf) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nkt) issue(kt + 1, buf ^ 1);
    const int k0 = kt * kAKT;
    if (k0 > wlast) return;  // past this wave's last visible key
    const unsigned char* Kl = lds + buf * BUF;
    const unsigned char* Vl = Kl + IMG;
    const unsigned char* Sl = Vl + IMG;

    f32x16_t x[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int i = 0; i < 16; ++i) x[t][i] = 0.f;
#pragma unroll
      for (int u = 0; u < D / 32; ++u) {
        const uint4 kw = *reinterpret_cast<const uint4*>(Kl + koff[u] + 32 * t * D);
        x[t] = mfma32<T>(fp8_frag<T>(kw.x, kw.y), qf[2 * u], x[t]);
        x[t] = mfma32<T>(fp8_frag<T>(kw.z, kw.w), qf[2 * u + 1], x[t]);
      }
    }
    // scores in log2 units, times the key's scale; registers 4gq .. 4gq + 3 are 4 consecutive
    // keys.  masked (a compile-time switch): a tile past the first row's last key tests key > lim
    auto scores = [&](auto masked) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const float4 sc = *reinterpret_cast<const float4*>(Sl + (32 * t + 8 * gq + 4 * hl) * 4);
          const float s4[4] = {sc.x, sc.y, sc.z, sc.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int key = k0 + 32 * t + 8 * gq + 4 * hl + e;
            const int rg = 4 * gq + e;
            const float y = x[t][rg] * (s4[e] * a.scale_log2);
            x[t][rg] = decltype(masked)::value && key > lim ? -INFINITY : y;
          }
        }
    };
    if (k0 + kAKT - 1 > wfull) scores(std::true_type{});  // wave-uniform
    else scores(std::false_type{});
    float tmax = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t)
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
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) {
        const float p = fexp2(x[t][rg] - msafe);
        psum += p;
        x[t][rg] = p;
      }
    l = l * alpha + psum;
    if (grow) {  // skipped while no row of the wave raised its max (alpha == 1 exactly)
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
    }
    // p times the value's scale (a masked key: 0 times a loaded, finite scale)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const float4 sc =
            *reinterpret_cast<const float4*>(Sl + (kAKT + 32 * t + 8 * gq + 4 * hl) * 4);
        x[t][4 * gq] *= sc.x;
        x[t][4 * gq + 1] *= sc.y;
        x[t][4 * gq + 2] *= sc.z;
        x[t][4 * gq + 3] *= sc.w;
      }
    // O^T[d][row] += V^T[d][key] . P^T[key][row]
#pragma unroll
    for (int t = 0; t < 2; ++t)
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

  issue(0, 0);
  // Q^T fragments (B operand of S^T = K . Q^T) in the K reads' order: step 2u + v holds d =
  // 32u + 16hl + 8v + j.  The empty asm is a use the compiler must wait for HERE, once: left to
  // itself it waits for these loads inside the loop, and its vmcnt(0) there also waits out the
  // tile that was just issued.
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    qf[s] = *reinterpret_cast<const v8*>(Q + 32 * (s >> 1) + 16 * hl + 8 * (s & 1));
#pragma unroll
  for (int s = 0; s < D / 16; ++s) asm volatile("" : "+v"(qf[s]));
  for (int kt = 0; kt < nkt; ++kt) step(kt, kt & 1);

  if (r >= R) return;
  const float lt = l + __shfl_xor(l, 32);
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
#pragma unroll
  for (int h = 0; h < D / kAD; ++h)
    store_dT<T>(orow + kAD * h, reinterpret_cast<const f32x16_t(&)[2]>(o[2 * h]), hl, inv);
  if (hl == 0) *lrow = lt > 0.f ? m + log2f(lt) : -INFINITY;
}

}  // namespace

void attn_prefill_fp8(const AttnDecodeFp8& pp, void* o, float* lse, hipStream_t st) {
  const AttnDecode& p = pp.d;
  if (p.D != 64 && p.D != 128) {
    fprintf(stderr, "attn_prefill_fp8: head dim must be 64 or 128, got %d\n", p.D);
    abort();
  }
  if (p.Hkv <= 0 || p.H % p.Hkv != 0) {
    fprintf(stderr, "attn_prefill_fp8: %d query heads do not split over %d key/value heads\n",
            p.H, p.Hkv);
    abort();
  }
  if (pp.k_scale == nullptr || pp.v_scale == nullptr) {
    fprintf(stderr, "attn_prefill_fp8: an FP8 cache comes with its k_scale and v_scale\n");
    abort();
  }
  if (p.B <= 0 || p.Sq <= 0) return;
  const int64_t R = (int64_t)(p.H / p.Hkv) * p.Sq, tiles = (R + 127) / 128;
  if (p.Hkv > 65535 || p.B > 65535 || tiles > (1 << 23) || tiles * p.Hkv * p.B > 0x7fffffff) {
    fprintf(stderr, "attn_prefill_fp8: %lld row tiles x %d key/value heads x batch %d exceed a "
                    "launch grid\n", (long long)tiles, p.Hkv, p.B);
    abort();
  }
  if (p.k_new.p != nullptr) attn_fp8_append(pp, p.Sq, st);
  PrefillFp8Args a{};
  a.q = p.q.p; a.qsb = p.q.sb; a.qss = p.q.ss; a.qsh = p.q.sh;
  a.k = static_cast<const unsigned char*>(p.k.p); a.ksb = p.k.sb; a.kss = p.k.ss; a.ksh = p.k.sh;
  a.v = static_cast<const unsigned char*>(p.v.p); a.vsb = p.v.sb; a.vss = p.v.ss; a.vsh = p.v.sh;
  a.ks = pp.k_scale; a.kcb = pp.ks_sb; a.kch = pp.ks_sh;
  a.vs = pp.v_scale; a.vcb = pp.vs_sb; a.vch = pp.vs_sh;
  a.lens = p.cache_seqlens;
  a.append = p.k_new.p != nullptr ? 1 : 0;
  a.o = o; a.lse = lse;
  a.H = p.H; a.Hkv = p.Hkv; a.G = p.H / p.Hkv; a.Sq = p.Sq; a.Smax = p.Smax; a.R = (int)R;
  a.scale_log2 = p.scale * 1.4426950408889634f;
  const dim3 grid((unsigned)tiles, (unsigned)p.Hkv, (unsigned)p.B), block(kAT);
  if (p.dtype == DType::BF16) {
    if (p.D == 64) hipLaunchKernelGGL((attn_prefill_fp8_k<bf16_t, 64>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((attn_prefill_fp8_k<bf16_t, 128>), grid, block, 0, st, a);
  } else {
    if (p.D == 64) hipLaunchKernelGGL((attn_prefill_fp8_k<half_t, 64>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((attn_prefill_fp8_k<half_t, 128>), grid, block, 0, st, a);
  }
}

}  // namespace amd
