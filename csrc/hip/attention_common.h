// What the fused attention kernels of attention.hip (head dim 64) and attention_d128.hip
// (head dim 128) share: MFMA / LDS-DMA wrappers, the swizzled LDS images of a
// [64 rows][64 d] 16-bit tile (a 128-wide tile is two of them side by side), the dropout
// lattice, key-mask and packed-sequence helpers, the kernel argument blocks and the host
// dispatch over a problem's dtype and options.  None of it depends on the head dim.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "amd_dev.h"
#include "amd_kernels.h"

namespace amd {

namespace {

typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef short v4s_t __attribute__((ext_vector_type(4)));

constexpr int kAD = 64;          // d columns of one LDS image (= the head dim in attention.hip;
                                 // attention_d128.hip keeps two images per tile, kD = 128)
constexpr int kAT = 256;         // threads
constexpr int kAKT = 64;         // keys per K/V tile
constexpr int kARow = kAD * 2;   // 128 B per row

template <typename T> struct Frag;
template <> struct Frag<bf16_t> { typedef bf16_t v8 __attribute__((ext_vector_type(8))); };
template <> struct Frag<half_t> { typedef half_t v8 __attribute__((ext_vector_type(8))); };

template <typename T>
__device__ __forceinline__ f32x16_t mfma32(typename Frag<T>::v8 a, typename Frag<T>::v8 b,
                                           f32x16_t c) {
  if constexpr (std::is_same<T, bf16_t>::value)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// LDS DMA (16 bytes per lane into M0 + 16 * lane) as inline asm, NOT the builtin: the
// compiler cannot tell which LDS bytes a pending builtin DMA writes, so it put an
// s_waitcnt vmcnt(0) in front of LDS reads of the CURRENT tile that follow the next
// tile's issue (ISA of the round-5 build: one per forward loop, one to two per dQ / dK-dV
// loop) - every iteration waited out the prefetch it had just started.  Every kernel here
// orders the ring itself (s_waitcnt vmcnt(0) + barrier before a slot is read, the refill
// after the barrier), so the compiler need not know about these writes.
__device__ __forceinline__ uint32_t lds_addr32(const void* l) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)l;
}
__device__ __forceinline__ void glds16(const void* g, unsigned char* l) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("global_load_lds_dwordx4 %0, off" : : "v"(g), "{m0}"(lds_addr32(l)) : "memory");
#endif
}

// Tile DMA addressing: a wave-uniform tile base (SGPRs, one scalar multiply-add per
// tile) plus a loop-invariant per-lane 32-bit byte offset (row * row stride + swizzled
// chunk), which selects the saddr form of global_load_lds.  Computing the 64-bit
// address per tile and lane instead (clamped row * stride) cost 8 v_mul_lo_u32 + 4
// v_mad_u64_u32 per forward tile - quarter-rate VALU, ~1/5 of the no-dropout forward's
// VALU cycles.  Only a tile that reaches past S takes the clamped per-lane path.  The
// binding keeps row strides below 2^24 elements so the offsets fit 32 bits.
__device__ __forceinline__ void glds16o(const void* tile_base, uint32_t off, unsigned char* l) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("global_load_lds_dwordx4 %0, %1" : : "v"(off), "s"(tile_base), "{m0}"(lds_addr32(l))
               : "memory");
#endif
}

template <typename T>
__device__ __forceinline__ uint32_t row_off(int row, int64_t stride, int chunk) {
  return (uint32_t)row * (uint32_t)stride * (uint32_t)sizeof(T) + (uint32_t)chunk * 16u;
}

template <typename T>
__device__ __forceinline__ const T* tile_base(const T* p, int row0, int64_t stride) {
  return p + (int64_t)row0 * stride;
}

// LDS images of a [64 rows][64 d] 16-bit tile (128-B rows)
__device__ __forceinline__ int swz_rows(int row, int chunk) {   // for ds_read_b128 row reads
  return row * kARow + ((chunk ^ ((row >> 1) & 7)) << 4);
}
__device__ __forceinline__ int swz_tr(int row, int chunk) {     // for transposed reads
  return row * kARow + ((chunk ^ (((row >> 1) & 1) << 2)) << 4);
}

template <typename T>
__device__ __forceinline__ typename Frag<T>::v8 lds_row8(const unsigned char* base, int off) {
  return *reinterpret_cast<const typename Frag<T>::v8*>(base + off);
}

// transposed fragment: element j of this lane = column `col` of rows r0+j (j<4) and
// r1+j-4 (j>=4), rows/cols as the lane's 16-lane group addresses them
template <typename T>
__device__ __forceinline__ typename Frag<T>::v8 lds_tr8(const unsigned char* base, int lo,
                                                        int hi) {
  v4s_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)(base + lo));
  v4s_t b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s_t*)(base + hi));
  typename Frag<T>::v8 f;
  v4s_t* fp = reinterpret_cast<v4s_t*>(&f);
  fp[0] = a;
  fp[1] = b;
  return f;
}

// byte offset of the 8-byte piece a lane supplies for a transposed read of rows
// [r0, r0+4) x columns [c0, c0+16) of a swz_tr image
__device__ __forceinline__ int tr_addr(int r0, int c0, int lane) {
  const int i = lane & 15, q = i >> 2, p = i & 3;
  const int col = c0 + 4 * p;
  return swz_tr(r0 + q, col >> 3) + ((col >> 2) & 1) * 8;
}

// Counter-based dropout bits: one 32-bit hash per (query, key QUAD), one byte per key:
// key k keeps its score iff byte (k & 3) of the hash is >= thr8 = round(256 p) (so p is
// quantised to 1/256 and the kept scores are scaled by 256 / (256 - thr8), unbiased for
// the quantised rate).  One hash per four scores instead of per two: the hash was ~half of
// the forward's VALU (267 of 520 per tile, docs/PERF.md round 4).  The hash input is a
// point of a Weyl lattice, base(seed, b*H+h) + q*kDropQ + (key>>2)*kDropK (mod 2^32), so
// a kernel steps from one (query, key quad) to the next with ONE add whose lattice offset
// is a compile-time literal; the mixer uses the full-rate 24-bit multiply
// (v_mul_u32_u24) where the classic 32-bit finalizers need the quarter-rate v_mul_lo_u32.
// tests/test_attention_gpu.py mirrors it bit for bit; tests/test_dropout_hash_cpu.py
// checks the keep rate, byte uniformity and neighbour correlations of the mirror.
constexpr uint32_t kDropQ = 0x85EBCA77u, kDropK = 0xC2B2AE3Du;

__device__ __forceinline__ uint32_t drop_base(uint32_t seed, uint32_t bh) {
  uint32_t x = seed ^ (bh * 0x9E3779B1u);
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ uint32_t drop_mix(uint32_t x) {
  x ^= x >> 16;
  x = __umul24(x, 0xE9846Bu) ^ (x >> 24);
  x ^= x >> 13;
  x = __umul24(x, 0x8B3C2Du) ^ (x >> 24);
  x ^= x >> 16;
  return x;
}

// the closed form; the kernels' incremental lattice steps compute exactly this
[[maybe_unused]] __device__ __forceinline__ uint32_t drop_hash(uint32_t seed, uint32_t bh, uint32_t q,
                                              uint32_t kquad) {
  return drop_mix(drop_base(seed, bh) + q * kDropQ + kquad * kDropK);
}

// raw v_exp_f32: exp2f() expands to a denormal-safe sequence (compare, select, ldexp:
// 5-6 VALU per score); softmax arguments are <= 0 and a result below 2^-126 may flush
__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }
// keep decision of byte e (= key & 3) of a (query, key quad) hash
__device__ __forceinline__ bool drop_keep8(uint32_t h, int e, uint32_t thr8) {
  return ((h >> (8 * e)) & 0xffu) >= thr8;
}

// one v_cvt_pk_{bf16,f16}_f32 per pair (converting the two floats separately and
// merging the halves cost 4 VALU per pair: ~50 of the forward's ~215 VALU per tile)
template <typename T>
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef T t2 __attribute__((ext_vector_type(2)));
  const f2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, t2));
}

// registers 8s..8s+7 of a 32x32 accumulator as a 16-bit MFMA fragment
template <typename T>
__device__ __forceinline__ typename Frag<T>::v8 acc_frag(const f32x16_t& x, int s) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = pack2<T>(x[8 * s + 2 * i], x[8 * s + 2 * i + 1]);
  return __builtin_bit_cast(typename Frag<T>::v8, *reinterpret_cast<uint4*>(w));
}

// a 32(d) x 32(col) transposed accumulator pair (d = 32dt + row) as the 64 values
// of 64 consecutive d of a 16-bit output row (a whole D = 64 row, half a D = 128 one),
// times `mul`
template <typename T>
__device__ __forceinline__ void store_dT(T* row_ptr, const f32x16_t (&acc)[2], int hl, float mul) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = 32 * dt + 8 * g + 4 * hl;
      uint2 w;
      w.x = pack2<T>(acc[dt][4 * g] * mul, acc[dt][4 * g + 1] * mul);
      w.y = pack2<T>(acc[dt][4 * g + 2] * mul, acc[dt][4 * g + 3] * mul);
      *reinterpret_cast<uint2*>(row_ptr + d) = w;
    }
}

// ---- FP8 (e4m3) K / V tiles: what attention_decode_fp8.hip and attention_prefill_fp8.hip share;
// the layouts are documented in attention_decode_fp8.hip's header ("Operands") ----

// LDS DMA of 4 bytes per lane into M0 + 4 * lane (glds16o's form: wave-uniform base, per-lane
// 32-bit byte offset)
__device__ __forceinline__ void glds4o(const void* base, uint32_t off, unsigned char* l) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("global_load_lds_dword %0, %1" : : "v"(off), "s"(base), "{m0}"(lds_addr32(l))
               : "memory");
#endif
}

// byte offset of 16-byte chunk c of key r in a [KS][D bytes] image (header: K, V)
template <int D>
__device__ __forceinline__ int swz_k8(int r, int c) {
  return r * D + ((c ^ (D == 64 ? (r >> 2) & 3 : (r >> 1) & 7)) << 4);
}
template <int D>
__device__ __forceinline__ int swz_v8(int r, int c) {
  const int x = D == 64 ? ((r >> 3) & 1) << 1 : (((r >> 1) & 1) << 1) | (((r >> 3) & 1) << 2);
  return r * D + ((c ^ x) << 4);
}

// 8 e4m3 bytes (lo: elements 0 .. 3, hi: 4 .. 7) as a 16-bit MFMA fragment, exact
template <typename T>
__device__ __forceinline__ typename Frag<T>::v8 fp8_frag(uint32_t lo, uint32_t hi) {
  uint32_t w[4];
  if constexpr (std::is_same<T, bf16_t>::value) {
    w[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.f, false));
    w[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.f, true));
    w[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.f, false));
    w[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.f, true));
  } else {
    w[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.f, false));
    w[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.f, true));
    w[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.f, false));
    w[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.f, true));
  }
  return __builtin_bit_cast(typename Frag<T>::v8, *reinterpret_cast<uint4*>(w));
}

typedef int v2i_t __attribute__((ext_vector_type(2)));

struct AttnArgs {
  const void* q;
  const void* k;
  const void* v;
  int64_t qsb, qss, qsh, ksb, kss, ksh, vsb, vss, vsh;  // element strides
  void* o;           // [B][Sq][H][D]
  float* lse;        // [B][H][lse_stride]
  int B, H, Sq, Sk;  // query / key lengths (wave-uniform; causal: Sq == Sk)
  int lse_stride;    // attn_lse_stride(Sq): rows of lse
  int key_stride;    // attn_lse_stride(Sk): rows of kbias, 64 x the rows of klive
  float scale_log2;  // softmax scale * log2(e)
  uint32_t thr8;     // dropout threshold round(p * 256) on a hash byte, 0 = no dropout
  float inv_keep;    // 256 / (256 - thr8): 1 / (1 - p) at the quantised rate
  uint32_t seed;
  const float* kbias;          // KMASK: [B][key_stride] log2-unit key bias
  const unsigned char* klive;  // KMASK: [B][key_stride / 64] tile liveness
  const int* cu;               // VARLEN: [B + 1] first token row of each sequence
  int T;                       // VARLEN: rows of the packed views
  int G;                       // GQA: query heads per key/value head (H / Hkv), else 1
  // AMASK: the prepared pair mask (amd_kernels.h), batch strides in tiles (0 = shared)
  const unsigned long long* wq;
  const unsigned char* cq;
  const unsigned long long* wk;
  const unsigned char* ck;
  int64_t mqs, mks;
};

// The live key tiles of one batch element, in order: ballots 64 liveness bytes at a time
// (the only plain global load, once per 4096 keys, taken right before the ring's own
// vmcnt(0) so it drains nothing) and steps through the set bits, so dead tiles cost
// neither DMA nor compute wherever they lie (padding on either side, holes).
struct LiveTiles {
  const unsigned char* live;
  int nkt, lane, c0;
  unsigned long long lm;
  __device__ __forceinline__ LiveTiles(const unsigned char* live_, int nkt_, int lane_)
      : live(live_), nkt(nkt_), lane(lane_), c0(-64), lm(0) {}
  // the next live tile; nkt when none is left
  __device__ __forceinline__ int next() {
    while (lm == 0) {
      c0 += 64;
      if (c0 >= nkt) return nkt;
      const int t = c0 + lane;
      lm = __ballot(t < nkt && live[t] != 0);
    }
    const int kt = c0 + __builtin_ctzll(lm);
    lm &= lm - 1;
    return kt;
  }
};

// AMASK: the non-dead tiles of one row of tile classes (cq: the key tiles of a 128-query
// tile; ck: the query tiles of a 128-key tile), in order, as LiveTiles walks liveness bytes;
// the same load and a second ballot tell whether the tile is full (class 2: every pair
// attends, the mask-free math serves) or mixed (class 1: the lane tests its bits).
struct PairTiles {
  const unsigned char* cls;
  int n, lane, c0;
  unsigned long long lm, fm;
  bool full;  // the class of the tile next() returned last
  __device__ __forceinline__ PairTiles(const unsigned char* cls_, int n_, int lane_)
      : cls(cls_), n(n_), lane(lane_), c0(-64), lm(0), fm(0), full(false) {}
  __device__ __forceinline__ int next() {
    while (lm == 0) {
      c0 += 64;
      if (c0 >= n) return n;
      const int t = c0 + lane;
      const int c = t < n ? cls[t] : 0;
      lm = __ballot(c != 0);
      fm = __ballot(c == 2);
    }
    const int i = __builtin_ctzll(lm);
    full = (fm >> i) & 1;
    lm &= lm - 1;
    return c0 + i;
  }
};
// a lane's 64-bit mask word of a tile (its query's 64 keys, or its key's 64 queries) as the
// two 32-bit halves shifted down by 4 hl: bit (r & 3) + 8 (r >> 2) of half t is then the
// pair of accumulator register r of 32-row half t, a compile-time position
__device__ __forceinline__ uint2 pair_word(const unsigned char* blk, int row, int hl) {
  const uint2 w = *reinterpret_cast<const uint2*>(blk + 8 * row);
  return uint2{w.x >> (4 * hl), w.y >> (4 * hl)};
}
__device__ __forceinline__ bool pair_bit(const uint2& w, int t, int r) {
  return (((t ? w.y : w.x) >> ((r & 3) + 8 * (r >> 2))) & 1u) != 0;
}

// VARLEN: sequence b of a packed batch, rows cu[b] .. cu[b + 1] - 1 of [T, H, D] views -
// two scalar loads, wave-uniform.  The length is clipped to the launch's max_seqlen (the
// rows lse / D have) and to the T rows the views hold, so whatever cu contains no row
// outside the views or the lse rows is touched; a workgroup whose tile starts at or past
// the length has nothing to do (false: the caller returns before any clamp, DMA or
// barrier - the row clamps index row -1 at length 0).
__device__ __forceinline__ bool varlen_seq(const int* cu, int b, int T, int max_len, int tile0,
                                           int& s0, int& len) {
  s0 = cu[b];
  int l = cu[b + 1] - s0;
  l = l < max_len ? l : max_len;
  l = l < T - s0 ? l : T - s0;
  len = l;
  return s0 >= 0 && tile0 < l;
}
// element offset of batch element b (stride sb) or, VARLEN, of the sequence whose first
// row is s0 (row stride ss)
template <bool VARLEN>
__device__ __forceinline__ int64_t seq_off(int b, int s0, int64_t sb, int64_t ss) {
  if constexpr (VARLEN) return (int64_t)s0 * ss;
  else return b * sb;
}

// Block -> (tile, b*H+h).  Dispatch order is the flattened block id (x fastest) and
// consecutive ids go to consecutive XCDs, so: (1) the tiles of one head are gridDim.y
// ids apart - the same XCD whenever B*H % 8 == 0, so that head's K/V (fwd, dQ) or
// Q/dO (dK/dV) stream through one L2 instead of up to 8; (2) under a causal mask the
// tiles with the most work are dispatched first (longest-processing-time order: the
// last query tiles in fwd / dQ, the first key tiles in dK/dV), so the light diagonal
// tiles fill the tail instead of a few heavy ones.
__device__ __forceinline__ void tile_of_block(bool causal, bool heavy_high, int& tile, int& bh) {
  const int nt = gridDim.x, nbh = gridDim.y;
  const int id = blockIdx.x + blockIdx.y * nt;
  const int t = id / nbh;
  bh = id - t * nbh;
  tile = (causal && heavy_high) ? nt - 1 - t : t;
}

// the other 32-lane half's value of x (lane ^ 32) on the VALU (v_permlane32_swap)
// instead of an LDS round trip (ds_bpermute)
__device__ __forceinline__ float max_halves(float x) {
  const unsigned u = __builtin_bit_cast(unsigned, x);
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
}

struct AttnBwdArgs {
  const void* q;
  const void* k;
  const void* v;
  const void* o;
  const void* dout;
  int64_t qsb, qss, qsh, ksb, kss, ksh, vsb, vss, vsh, osb, oss, osh, dsb, dss, dsh;
  void* dq;
  void* dk;
  void* dv;
  int64_t dqsb, dqss, dqsh, dksb, dkss, dksh, dvsb, dvss, dvsh;
  const float* lse;  // [B][H][lse_stride] log2 units
  float* D;          // [B][H][lse_stride] rowsum(dO * O); KMASK: [2][B][H][lse_stride]
  int B, H, Sq, Sk;  // query / key lengths (wave-uniform; causal: Sq == Sk)
  int lse_stride;    // attn_lse_stride(Sq): rows of lse, D and the lse copy behind D
  int key_stride;    // attn_lse_stride(Sk): rows of kbias, 64 x the rows of klive
  float scale, scale_log2;
  uint32_t thr8;
  float inv_keep;
  uint32_t seed;
  const float* kbias;          // KMASK: [B][key_stride] log2-unit key bias
  const unsigned char* klive;  // KMASK: [B][key_stride / 64] tile liveness
  const int* cu;               // VARLEN: [B + 1] first token row of each sequence
  int T;                       // VARLEN: rows of the packed views
  int G;                       // GQA: query heads per key/value head (H / Hkv), else 1
  // AMASK: the prepared pair mask (amd_kernels.h), batch strides in tiles (0 = shared)
  const unsigned long long* wq;
  const unsigned char* cq;
  const unsigned long long* wk;
  const unsigned char* ck;
  int64_t mqs, mks;
};

// A query none of whose keys is live has lse = -inf (or whatever the caller stored);
// read as +inf it makes every recomputed p = exp2(score - lse) exactly 0, where -inf
// would give exp2(-inf - -inf).
__device__ __forceinline__ float lse_guard(float lse) { return lse == -INFINITY ? INFINITY : lse; }

// host: the byte threshold of a dropout rate (round(256 p); p >= 255.5 / 256 drops all)
// keep decisions compare one hash byte with round(256 p): the rate is quantised to 1/256
// (ops/attention.py effective_dropout warns where that moves it by more than 2 %), and a
// rate below 1/512 still drops (threshold 1), never silently turns dropout off
static uint32_t drop_thr8(float p) {
  if (!(p > 0.f)) return 0u;
  const float t = p * 256.f + 0.5f;
  return t >= 256.f ? 256u : (t < 1.f ? 1u : (uint32_t)t);
}

}  // namespace

// the causal mask is defined for one shared length only (no alignment convention for
// unequal ones); the torch binding refuses the call before it gets here
static void require_no_mask_when_packed(const char* who, const AttnProblem& p) {
  if (p.cu_seqlens != nullptr && (p.kbias != nullptr || p.Sq != p.Sk || p.T < 0)) {
    fprintf(stderr, "%s: a packed problem (cu_seqlens) takes no key mask and one max_seqlen\n",
            who);
    abort();
  }
}
static void require_pair_mask_alone(const char* who, const AttnProblem& p) {
  if (p.wq == nullptr) return;
  if (p.causal || p.kbias != nullptr || p.cu_seqlens != nullptr || p.cq == nullptr ||
      p.wk == nullptr || p.ck == nullptr) {
    fprintf(stderr, "%s: a pair mask comes whole (wq, cq, wk, ck) and takes no causal flag, key "
                    "mask or cu_seqlens: its bits hold those shapes\n", who);
    abort();
  }
}
static void require_heads(const char* who, const AttnProblem& p) {
  if (p.Hkv <= 0 || p.H % p.Hkv != 0) {
    fprintf(stderr, "%s: %d query heads do not split over %d key/value heads\n", who, p.H, p.Hkv);
    abort();
  }
  if (p.Hkv != p.H && (p.cu_seqlens != nullptr || p.wq != nullptr)) {
    fprintf(stderr, "%s: grouped-query heads (H = %d, Hkv = %d) take no cu_seqlens and no pair "
                    "mask\n", who, p.H, p.Hkv);
    abort();
  }
}
static void require_causal_square(const char* who, bool causal, int Sq, int Sk) {
  if (causal && Sq != Sk) {
    fprintf(stderr, "%s: causal needs equal query and key lengths, got Sq = %d, Sk = %d\n", who,
            Sq, Sk);
    abort();
  }
}

namespace {

// The kernel arguments a problem determines, for either direction (A = AttnArgs or
// AttnBwdArgs, which name these fields alike): views, lengths, the two row strides and
// the quantised dropout.  The caller adds its direction's buffers.
template <typename A>
A kernel_args(const char* who, const AttnProblem& p) {
  require_causal_square(who, p.causal, p.Sq, p.Sk);
  require_no_mask_when_packed(who, p);
  require_pair_mask_alone(who, p);
  require_heads(who, p);
  A a{};
  a.q = p.q.p; a.qsb = p.q.sb; a.qss = p.q.ss; a.qsh = p.q.sh;
  a.k = p.k.p; a.ksb = p.k.sb; a.kss = p.k.ss; a.ksh = p.k.sh;
  a.v = p.v.p; a.vsb = p.v.sb; a.vss = p.v.ss; a.vsh = p.v.sh;
  a.B = p.B; a.H = p.H; a.Sq = p.Sq; a.Sk = p.Sk;
  a.lse_stride = attn_lse_stride(p.Sq);
  a.key_stride = attn_lse_stride(p.Sk);
  a.scale_log2 = p.scale * 1.4426950408889634f;
  a.thr8 = drop_thr8(p.dropout);
  a.inv_keep = a.thr8 >= 256u ? 0.f : 256.f / (256.f - (float)a.thr8);
  a.seed = p.seed;
  a.kbias = p.kbias; a.klive = p.klive;
  a.cu = p.cu_seqlens; a.T = p.T;
  a.G = p.H / p.Hkv;
  a.wq = p.wq; a.cq = p.cq; a.wk = p.wk; a.ck = p.ck;
  a.mqs = p.pm_sb;
  a.mks = p.pm_sb ? (int64_t)((p.Sk + 127) / 128) * ((p.Sq + kAKT - 1) / kAKT) : 0;
  return a;
}

// ... and the backward's, with its buffers
inline AttnBwdArgs bwd_kernel_args(const char* who, const AttnProblem& p, const AttnBwd& g) {
  AttnBwdArgs a = kernel_args<AttnBwdArgs>(who, p);
  a.o = g.o.p; a.osb = g.o.sb; a.oss = g.o.ss; a.osh = g.o.sh;
  a.dout = g.dout.p; a.dsb = g.dout.sb; a.dss = g.dout.ss; a.dsh = g.dout.sh;
  a.dq = g.dq.p; a.dqsb = g.dq.sb; a.dqss = g.dq.ss; a.dqsh = g.dq.sh;
  a.dk = g.dk.p; a.dksb = g.dk.sb; a.dkss = g.dk.ss; a.dksh = g.dk.sh;
  a.dv = g.dv.p; a.dvsb = g.dv.sb; a.dvss = g.dv.ss; a.dvsh = g.dv.sh;
  a.lse = g.lse; a.D = g.D;
  a.scale = p.scale;
  return a;
}

template <typename T> struct Elem { using type = T; };

// f(Elem<T>, causal, drop, kmask, varlen), the switches as std::bool_constants: the
// 2 x 2 x 2 x 3 kernel instantiations over a problem's dtype and options ({plain, key
// mask, packed}: a packed problem has no key mask)
template <typename F>
void dispatch(const AttnProblem& p, bool drop, F f) {
  auto flag = [](bool on, auto g) { on ? g(std::true_type{}) : g(std::false_type{}); };
  auto flags = [&](auto t) {
    flag(p.causal, [&](auto c) {
      flag(drop, [&](auto d) {
        if (p.cu_seqlens != nullptr) f(t, c, d, std::false_type{}, std::true_type{});
        else flag(p.kbias != nullptr, [&](auto m) { f(t, c, d, m, std::false_type{}); });
      });
    });
  };
  if (p.dtype == DType::BF16) flags(Elem<bf16_t>{});
  else flags(Elem<half_t>{});
}

// the kernel `name` instantiated for dispatch's (t, c, d, m, vl)
#define ATTN_KERNEL(name)                                                                    \
  name<typename decltype(t)::type, decltype(c)::value, decltype(d)::value, decltype(m)::value, \
       decltype(vl)::value, false, false>

// f(Elem<T>, drop): the 2 x 2 pair-mask (AMASK) instantiations, which exclude the other three
template <typename F>
void dispatch_amask(const AttnProblem& p, bool drop, F f) {
  auto flags = [&](auto t) { drop ? f(t, std::true_type{}) : f(t, std::false_type{}); };
  if (p.dtype == DType::BF16) flags(Elem<bf16_t>{});
  else flags(Elem<half_t>{});
}
#define ATTN_AMASK_KERNEL(name) \
  name<typename decltype(t)::type, false, decltype(d)::value, false, false, true, false>

// f(Elem<T>, causal, drop, kmask): the 2 x 2 x 2 x 2 grouped-query (GQA) instantiations, which
// exclude packed sequences and pair masks
template <typename F>
void dispatch_gqa(const AttnProblem& p, bool drop, F f) {
  auto flag = [](bool on, auto g) { on ? g(std::true_type{}) : g(std::false_type{}); };
  auto flags = [&](auto t) {
    flag(p.causal, [&](auto c) {
      flag(drop, [&](auto d) { flag(p.kbias != nullptr, [&](auto m) { f(t, c, d, m); }); });
    });
  };
  if (p.dtype == DType::BF16) flags(Elem<bf16_t>{});
  else flags(Elem<half_t>{});
}
#define ATTN_GQA_KERNEL(name)                                                                \
  name<typename decltype(t)::type, decltype(c)::value, decltype(d)::value, decltype(m)::value, \
       false, false, true>

}  // namespace

// the head dim 128 kernels (attention_d128.hip), reached through attn_fwd / attn_bwd
void attn_fwd_d128(const AttnProblem& p, void* o, float* lse, hipStream_t st);
void attn_bwd_d128(const AttnProblem& p, const AttnBwd& g, hipStream_t st);
// the head dim 64 kernels under a pair mask (attention_pairmask.hip compiles them)
void attn_fwd_amask64(const AttnProblem& p, void* o, float* lse, hipStream_t st);
void attn_bwd_amask64(const AttnProblem& p, const AttnBwd& g, hipStream_t st);
// both head dims with fewer key/value heads than query heads (attention_gqa.hip compiles them)
void attn_fwd_gqa(const AttnProblem& p, void* o, float* lse, hipStream_t st);
void attn_bwd_gqa(const AttnProblem& p, const AttnBwd& g, hipStream_t st);
// the fixed-order join of a decode step's split partials (attention_decode.hip), which the
// paged decode kernels (attention_decode_paged.hip) share
void attn_decode_combine(DType dtype, int D, int B, int H, int Sq, int nsplit, float* o_part,
                         float* lse_part, void* o, float* lse, hipStream_t st);
// the append of a decode step alone (attention_decode.hip; nothing without k_new / v_new), which
// the prefill kernels (attention_prefill.hip) share
void attn_decode_append(const AttnDecode& p, hipStream_t st);

}  // namespace amd
