// Torch bindings for the fused attention kernels (csrc/hip/attention.hip).
#pragma once
#include <ATen/ATen.h>
#include <c10/util/Optional.h>

#include <tuple>

namespace amd {

// q: [B, Sq, H, 64], k, v: [B, Sk, H, 64] bf16/fp16 views (head dim contiguous, 16-B
// aligned rows; one B, H and dtype, the sequence lengths may differ - cross-attention).
// Returns (o [B, Sq, H, 64] contiguous, lse [B, H, Sq] fp32 log2 units; a view of a
// row-padded [B, H, round_up(Sq, 64)] buffer).  causal needs Sq == Sk.  Sk == 0 gives
// o = 0 and lse = -inf without a launch.
// key_bias / key_live: the prepared key mask of attn_prepare_key_mask_op for S = Sk (both
// or neither).
std::tuple<at::Tensor, at::Tensor> attn_fwd_op(at::Tensor q, at::Tensor k, at::Tensor v,
                                               bool causal, double dropout, int64_t seed,
                                               double scale,
                                               c10::optional<at::Tensor> key_bias = c10::nullopt,
                                               c10::optional<at::Tensor> key_live = c10::nullopt);

// Per-batch key mask [B, S] (bool / uint8: non-zero = masked key; fp32 / fp16 / bf16:
// additive, added to the scaled scores, -inf allowed) -> (bias fp32 [B, round_up(S, 64)]
// in log2 units with -inf past S, live uint8 [B, round_up(S, 64) / 64]: 0 where a 64-key
// tile is all -inf).  One launch, no host sync; reusable by every layer that shares the
// mask and by the backward.
std::tuple<at::Tensor, at::Tensor> attn_prepare_key_mask_op(at::Tensor mask, int64_t S);

// Writes dq (shaped like q), dk and dv (shaped like k; caller-allocated strided views,
// e.g. slices of one packed dqkv or dkv buffer) from dout, the forward inputs, o and lse.
// Sk == 0 writes dq = 0, Sq == 0 writes dk = dv = 0, both without a launch.
void attn_bwd_op(at::Tensor dout, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                 at::Tensor lse, bool causal, double dropout, int64_t seed, double scale,
                 at::Tensor dq, at::Tensor dk, at::Tensor dv,
                 c10::optional<at::Tensor> key_bias = c10::nullopt,
                 c10::optional<at::Tensor> key_live = c10::nullopt);

// Boolean pair mask: bool / uint8 [Sq, Sk] or [B, Sq, Sk] (non-zero = masked), optionally
// OR-ed with a bool / uint8 [B, Sk] key-padding mask (the result is then per batch) -> the
// bit tiles of csrc/hip/attention_pairmask.hip as two flat buffers: int64 words {wq
// [Bm][ceil(Sq/128)][ceil(Sk/64)][128], wk [Bm][ceil(Sk/128)][ceil(Sq/64)][128]} and uint8
// classes {cq [Bm][ceil(Sq/128)][ceil(Sk/64)], ck [Bm][ceil(Sk/128)][ceil(Sq/64)]}.  One
// launch, no host sync; serves every layer that shares the mask, forward and backward.
std::tuple<at::Tensor, at::Tensor> attn_prepare_attn_mask_op(
    at::Tensor mask, c10::optional<at::Tensor> key_padding_mask = c10::nullopt);

// attn_fwd_op / attn_bwd_op under a prepared pair mask (no causal flag, no key mask: the
// bits hold both).  A query with no set bit gets o = 0, lse = -inf, dq = 0; a key nobody
// attends gets dk = dv = 0.
std::tuple<at::Tensor, at::Tensor> attn_fwd_amask_op(at::Tensor q, at::Tensor k, at::Tensor v,
                                                     double dropout, int64_t seed, double scale,
                                                     at::Tensor wq, at::Tensor cq, at::Tensor wk,
                                                     at::Tensor ck);
void attn_bwd_amask_op(at::Tensor dout, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                       at::Tensor lse, double dropout, int64_t seed, double scale, at::Tensor dq,
                       at::Tensor dk, at::Tensor dv, at::Tensor wq, at::Tensor cq, at::Tensor wk,
                       at::Tensor ck);

// Packed variable-length sequences.  q, k, v: [T, H, 64] bf16/fp16 views of the real
// tokens of B sequences (head dim contiguous, 16-B aligned rows, any token / head strides,
// one T, H and dtype); cu_seqlens: contiguous int32 [B + 1] on q's device, read by the
// kernels (no host copy): sequence b owns rows cu[b] .. cu[b+1]-1 and attends within
// itself (causal per sequence).  max_seqlen >= every length sizes the grid and lse; the
// results do not depend on it.  Returns (o [T, H, 64] contiguous, lse [B, H, max_seqlen]
// fp32 log2 units, rows past a sequence's length unspecified; a view of a row-padded
// [B, H, round_up(max_seqlen, 64)] buffer).  T == 0 launches nothing; B == 0 gives o = 0.
std::tuple<at::Tensor, at::Tensor> attn_fwd_varlen_op(at::Tensor q, at::Tensor k, at::Tensor v,
                                                      at::Tensor cu_seqlens, int64_t max_seqlen,
                                                      bool causal, double dropout, int64_t seed,
                                                      double scale);

// Writes rows cu[b] .. cu[b+1]-1 of dq, dk, dv (caller-allocated strided [T, H, 64] views,
// e.g. slices of one packed dqkv buffer) for every sequence b and nothing else.  B == 0
// writes zeros without a launch.
void attn_bwd_varlen_op(at::Tensor dout, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                        at::Tensor lse, at::Tensor cu_seqlens, int64_t max_seqlen, bool causal,
                        double dropout, int64_t seed, double scale, at::Tensor dq, at::Tensor dk,
                        at::Tensor dv);

// Decode step over a KV cache (csrc/hip/attention_decode.hip; forward only, no gradient).
// q: [B, Sq, H, D], the Sq newest tokens; k_cache, v_cache: [B, Smax, Hkv, D] views (any
// batch / sequence / head strides, head dim contiguous, 16-B aligned rows; H % Hkv == 0, D =
// 64 or 128, one bf16 / fp16 dtype); cache_seqlens: contiguous int32 [B] on q's device, the
// keys in the cache before the call, read by the kernels only (no host sync).  k_new / v_new
// [B, Sq, Hkv, D] (both or neither) are first written to cache rows cache_seqlens[b] + i.
// num_splits: 0 = chosen from the shapes and the device's CU count, else 1 ..
// kAttnDecodeMaxSplits.  Returns (o [B, Sq, H, D] contiguous, lse [B, H, Sq] fp32 log2 units).
// B == 0 or Sq == 0 launches nothing.
std::tuple<at::Tensor, at::Tensor> attn_decode_op(at::Tensor q, at::Tensor k_cache,
                                                  at::Tensor v_cache, at::Tensor cache_seqlens,
                                                  c10::optional<at::Tensor> k_new,
                                                  c10::optional<at::Tensor> v_new, double scale,
                                                  int64_t num_splits);

// Sq new tokens (any Sq: a prompt chunk, a turn, a draft) over a contiguous 16-bit KV cache that
// holds a prefix (csrc/hip/attention_prefill.hip; forward only, no gradient).  Tensors, lengths,
// mask, append and results are attn_decode_op's word for word; the kernels split the rows, not
// the keys: one launch, no workspace, no num_splits, bitwise reproducible.
std::tuple<at::Tensor, at::Tensor> attn_prefill_op(at::Tensor q, at::Tensor k_cache,
                                                   at::Tensor v_cache, at::Tensor cache_seqlens,
                                                   c10::optional<at::Tensor> k_new,
                                                   c10::optional<at::Tensor> v_new, double scale);

// The same step over a paged KV cache (csrc/hip/attention_decode_paged.hip).  k_pages, v_pages:
// [num_pages, P, Hkv, D] views (any page / row / head strides, head dim contiguous, 16-B
// aligned rows, P in {16, 32, 64, 128, 256}, P x row stride below 2^32 bytes); block_table:
// contiguous int32 [B, max_pages] on q's device, max_pages * P < 2^24: key j of batch element
// b is row j % P of page block_table[b][j / P].  Page ids are clamped to the pool on the device
// and entries at or past ceil(L_b / P) are never read.  Everything else as attn_decode_op,
// whose result on the same keys this one equals bit for bit at the same num_splits.
std::tuple<at::Tensor, at::Tensor> attn_decode_paged_op(
    at::Tensor q, at::Tensor k_pages, at::Tensor v_pages, at::Tensor block_table,
    at::Tensor cache_seqlens, c10::optional<at::Tensor> k_new, c10::optional<at::Tensor> v_new,
    double scale, int64_t num_splits);

// The append alone: k_new / v_new [B, Sn, Hkv, D] (any Sn) into the pages at keys
// cache_seqlens[b] + i; keys outside [0, max_pages * P) are skipped.  One launch, no host sync.
void attn_paged_append_op(at::Tensor k_new, at::Tensor v_new, at::Tensor k_pages,
                          at::Tensor v_pages, at::Tensor block_table, at::Tensor cache_seqlens);

// The decode step over an FP8 KV cache (csrc/hip/attention_decode_fp8.hip).  k_cache, v_cache:
// float8_e4m3fn [B, Smax, Hkv, D] views (any batch / sequence / head strides that are multiples
// of 16 bytes, head dim contiguous, 16-B aligned); k_scale, v_scale: fp32 [B, Hkv, Smax] views
// with the key index contiguous (any batch / head strides); q and k_new / v_new: one bf16 / fp16
// dtype.  k_new / v_new are quantised per row on their way into the cache.  Everything else as
// attn_decode_op.
std::tuple<at::Tensor, at::Tensor> attn_decode_fp8_op(
    at::Tensor q, at::Tensor k_cache, at::Tensor v_cache, at::Tensor k_scale, at::Tensor v_scale,
    at::Tensor cache_seqlens, c10::optional<at::Tensor> k_new, c10::optional<at::Tensor> v_new,
    double scale, int64_t num_splits);

// Sq new tokens over the same FP8 KV cache on the row-split kernels (csrc/hip/
// attention_prefill_fp8.hip): attn_decode_fp8_op's tensors and append, attn_prefill_op's single
// launch without num_splits, bitwise reproducible.
std::tuple<at::Tensor, at::Tensor> attn_prefill_fp8_op(
    at::Tensor q, at::Tensor k_cache, at::Tensor v_cache, at::Tensor k_scale, at::Tensor v_scale,
    at::Tensor cache_seqlens, c10::optional<at::Tensor> k_new, c10::optional<at::Tensor> v_new,
    double scale);

// The quantising append alone: k_new / v_new [B, Sn, Hkv, D] (bf16 / fp16, any Sn) into cache
// rows cache_seqlens[b] + i and their scales; rows outside [0, Smax) are skipped.  One launch,
// no host sync.
void attn_fp8_append_op(at::Tensor k_new, at::Tensor v_new, at::Tensor k_cache,
                        at::Tensor v_cache, at::Tensor k_scale, at::Tensor v_scale,
                        at::Tensor cache_seqlens);

}  // namespace amd
