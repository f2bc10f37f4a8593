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

}  // namespace amd
