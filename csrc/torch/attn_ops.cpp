// Torch bindings for the fused attention kernels (csrc/hip/attention.hip).
#include "attn_ops.h"

#include <limits>

#include "common.h"

namespace amd {

namespace {
// the alignment the kernels need of a 4-d 16-bit tensor: contiguous, 16-byte aligned rows
bool view_ok(const at::Tensor& t) {
  return t.stride(3) == 1 && ((uintptr_t)t.data_ptr() % 16) == 0 && t.stride(0) % 8 == 0 &&
         t.stride(1) % 8 == 0 && t.stride(2) % 8 == 0;
}

// the kernels' view of a [B,S,H,64] tensor, or the reason it has none
AttnView view_of(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 4 && t.size(3) == 64, "attn: ", what,
              " must be a [B,S,H,64] GPU tensor");
  TORCH_CHECK(t.stride(3) == 1, "attn: ", what, ": head dim must be contiguous");
  TORCH_CHECK(view_ok(t), "attn: ", what, ": 16-byte aligned rows required");
  // the kernels' tile DMA uses 32-bit per-lane row offsets (csrc/hip/attention.hip)
  TORCH_CHECK(t.stride(1) >= 0 && t.stride(1) < (int64_t{1} << 24), "attn: ", what,
              ": sequence stride must be below 2^24 elements");
  return {t.data_ptr(), t.stride(0), t.stride(1), t.stride(2)};
}

// q [B, Sq, H, 64], k / v [B, Sk, H, 64]: one B, H and dtype, any strides
AttnProblem make_launch(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                        bool causal, double dropout, int64_t seed, double scale) {
  AttnProblem L;
  L.q = view_of(q, "q");
  L.k = view_of(k, "k");
  L.v = view_of(v, "v");
  TORCH_CHECK(v.sizes() == k.sizes(), "attn: k and v shapes differ: ", k.sizes(), " and ",
              v.sizes());
  TORCH_CHECK(k.size(0) == q.size(0) && k.size(2) == q.size(2),
              "attn: q and k / v differ in batch or heads: q ", q.sizes(), ", k ", k.sizes(),
              " (only the sequence length may differ)");
  TORCH_CHECK(q.scalar_type() == k.scalar_type() && q.scalar_type() == v.scalar_type() &&
                  (q.scalar_type() == at::kBFloat16 || q.scalar_type() == at::kHalf),
              "attn: bf16/fp16 q,k,v of one dtype");
  TORCH_CHECK(k.device() == q.device() && v.device() == q.device(),
              "attn: q, k and v must be on one device");
  TORCH_CHECK(!causal || q.size(1) == k.size(1),
              "attn: causal is defined for equal query and key lengths only, got Sq = ",
              q.size(1), ", Sk = ", k.size(1));
  TORCH_CHECK(dropout >= 0.0 && dropout < 1.0, "attn: dropout must be in [0, 1)");
  L.B = (int)q.size(0); L.Sq = (int)q.size(1); L.Sk = (int)k.size(1); L.H = (int)q.size(2);
  L.scale = (float)scale; L.dropout = (float)dropout; L.seed = (uint32_t)seed;
  L.causal = causal; L.dtype = dtype_of(q);
  return L;
}

// the prepared key mask of attn_prepare_key_mask_op for the S = Sk keys of a call (Sp =
// attn_lse_stride(Sk)), or neither
void check_key_mask(const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& live,
                    const at::Tensor& q, int B, int Sk, const float** pb,
                    const unsigned char** pl) {
  const int Sp = attn_lse_stride(Sk);
  *pb = nullptr;
  *pl = nullptr;
  TORCH_CHECK(bias.has_value() == live.has_value(),
              "attn: key_bias and key_live come as a pair (attn.prepare_key_mask)");
  if (!bias.has_value()) return;
  const at::Tensor& kb = *bias;
  const at::Tensor& kl = *live;
  TORCH_CHECK(kb.is_cuda() && kl.is_cuda() && kb.device() == q.device() &&
                  kl.device() == q.device(),
              "attn: the prepared key mask must be on q's device");
  TORCH_CHECK(kb.scalar_type() == at::kFloat && kb.dim() == 2 && kb.size(0) == B &&
                  kb.size(1) == Sp && kb.is_contiguous(),
              "attn: key_bias must be a contiguous fp32 [B, round_up(S, 64)] tensor, got ",
              kb.sizes(), " for B = ", B, ", S = ", Sk, " keys");
  TORCH_CHECK(kl.scalar_type() == at::kByte && kl.dim() == 2 && kl.size(0) == B &&
                  kl.size(1) == Sp / 64 && kl.is_contiguous(),
              "attn: key_live must be a contiguous uint8 [B, round_up(S, 64) / 64] tensor, got ",
              kl.sizes());
  TORCH_CHECK(((uintptr_t)kb.data_ptr() % 16) == 0, "attn: key_bias must be 16-byte aligned");
  *pb = kb.data_ptr<float>();
  *pl = kl.data_ptr<unsigned char>();
}

// ---- packed variable-length sequences: [T, H, 64] views and an int32 offsets vector
bool view3_ok(const at::Tensor& t) {
  return t.stride(2) == 1 && ((uintptr_t)t.data_ptr() % 16) == 0 && t.stride(0) % 8 == 0 &&
         t.stride(1) % 8 == 0;
}

// the kernels' view of a packed [T,H,64] tensor (no batch stride), or the reason it has none
AttnView view3_of(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 3 && t.size(2) == 64, "attn varlen: ", what,
              " must be a [T,H,64] GPU tensor");
  TORCH_CHECK(t.stride(2) == 1, "attn varlen: ", what, ": head dim must be contiguous");
  TORCH_CHECK(view3_ok(t), "attn varlen: ", what, ": 16-byte aligned rows required");
  TORCH_CHECK(t.stride(0) >= 0 && t.stride(0) < (int64_t{1} << 24), "attn varlen: ", what,
              ": token stride must be below 2^24 elements");
  return {t.data_ptr(), 0, t.stride(0), t.stride(1)};
}

// q, k, v [T, H, 64] of one T, H and dtype, any token / head strides; cu_seqlens int32
// [B + 1] on q's device; Sq = Sk = max_seqlen
AttnProblem make_varlen_launch(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                               const at::Tensor& cu, int64_t max_seqlen, bool causal,
                               double dropout, int64_t seed, double scale) {
  AttnProblem L;
  L.q = view3_of(q, "q");
  L.k = view3_of(k, "k");
  L.v = view3_of(v, "v");
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes(),
              "attn varlen: q, k and v differ in tokens or heads: q ", q.sizes(), ", k ",
              k.sizes(), ", v ", v.sizes());
  TORCH_CHECK(q.scalar_type() == k.scalar_type() && q.scalar_type() == v.scalar_type() &&
                  (q.scalar_type() == at::kBFloat16 || q.scalar_type() == at::kHalf),
              "attn varlen: bf16/fp16 q,k,v of one dtype");
  TORCH_CHECK(k.device() == q.device() && v.device() == q.device(),
              "attn varlen: q, k and v must be on one device");
  TORCH_CHECK(cu.is_cuda() && cu.device() == q.device(),
              "attn varlen: cu_seqlens must be on q's device");
  TORCH_CHECK(cu.scalar_type() == at::kInt && cu.dim() == 1 && cu.size(0) >= 1 &&
                  cu.is_contiguous(),
              "attn varlen: cu_seqlens must be a contiguous int32 [B + 1] tensor, got ",
              cu.scalar_type(), " ", cu.sizes());
  TORCH_CHECK(max_seqlen > 0 && max_seqlen < (int64_t{1} << 24),
              "attn varlen: max_seqlen must be in (0, 2^24), got ", max_seqlen);
  TORCH_CHECK(q.size(0) < (int64_t{1} << 31), "attn varlen: too many tokens: ", q.size(0));
  TORCH_CHECK(dropout >= 0.0 && dropout < 1.0, "attn: dropout must be in [0, 1)");
  L.B = (int)cu.size(0) - 1; L.H = (int)q.size(1);
  TORCH_CHECK((int64_t)L.B * L.H <= 65535, "attn varlen: sequences x heads = ",
              (int64_t)L.B * L.H, " exceeds the 65535 rows of a launch grid");
  L.Sq = L.Sk = (int)max_seqlen;
  L.scale = (float)scale; L.dropout = (float)dropout; L.seed = (uint32_t)seed;
  L.causal = causal; L.dtype = dtype_of(q);
  L.cu_seqlens = cu.data_ptr<int32_t>();
  L.T = (int)q.size(0);
  return L;
}
}  // namespace

std::tuple<at::Tensor, at::Tensor> attn_prepare_key_mask_op(at::Tensor mask, int64_t S) {
  c10::NoGradGuard no_grad_;
  TORCH_CHECK(mask.is_cuda(), "attn.prepare_key_mask: the key mask must be a GPU tensor");
  TORCH_CHECK(mask.dim() == 2 && mask.size(1) == S,
              "attn.prepare_key_mask: the key mask must be [B, S] with S = ", S, ", got ",
              mask.sizes());
  TORCH_CHECK(mask.is_contiguous(), "attn.prepare_key_mask: the key mask must be contiguous");
  TORCH_CHECK(S > 0 && S < (int64_t{1} << 24), "attn.prepare_key_mask: S out of range");
  AttnMaskKind kind;
  switch (mask.scalar_type()) {
    case at::kBool:
    case at::kByte: kind = AttnMaskKind::Bool8; break;
    case at::kFloat: kind = AttnMaskKind::F32; break;
    case at::kHalf: kind = AttnMaskKind::F16; break;
    case at::kBFloat16: kind = AttnMaskKind::BF16; break;
    default:
      TORCH_CHECK(false, "attn.prepare_key_mask: bool / uint8 (non-zero = masked) or fp32 / "
                         "fp16 / bf16 (additive) mask expected, got ", mask.scalar_type());
  }
  const int B = (int)mask.size(0), Sp = attn_lse_stride((int)S);
  at::Tensor bias = at::empty({B, Sp}, mask.options().dtype(at::kFloat));
  at::Tensor live = at::empty({B, Sp / 64}, mask.options().dtype(at::kByte));
  if (B > 0)
    attn_prepare_key_mask(mask.data_ptr(), kind, B, (int)S, bias.data_ptr<float>(),
                          live.data_ptr<unsigned char>(), cur_stream());
  return {bias, live};
}

std::tuple<at::Tensor, at::Tensor> attn_fwd_op(at::Tensor q, at::Tensor k, at::Tensor v,
                                               bool causal, double dropout, int64_t seed,
                                               double scale, c10::optional<at::Tensor> key_bias,
                                               c10::optional<at::Tensor> key_live) {
  c10::NoGradGuard no_grad_;
  AttnProblem L = make_launch(q, k, v, causal, dropout, seed, scale);
  check_key_mask(key_bias, key_live, q, L.B, L.Sk, &L.kbias, &L.klive);
  const int Sp = attn_lse_stride(L.Sq);
  at::Tensor o = at::empty({L.B, L.Sq, L.H, 64}, q.options());
  at::Tensor lse = at::empty({L.B, L.H, Sp}, q.options().dtype(at::kFloat));
  if (L.Sk == 0) {  // no key to attend to: o = 0, lse = log2(0), no launch
    o.zero_();
    lse.fill_(-std::numeric_limits<float>::infinity());
  } else if (L.Sq > 0 && L.B * L.H > 0) {
    attn_fwd(L, o.data_ptr(), lse.data_ptr<float>(), cur_stream());
  }
  return {o, Sp == L.Sq ? lse : lse.narrow(2, 0, L.Sq)};
}

void attn_bwd_op(at::Tensor dout, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                 at::Tensor lse, bool causal, double dropout, int64_t seed, double scale,
                 at::Tensor dq, at::Tensor dk, at::Tensor dv, c10::optional<at::Tensor> key_bias,
                 c10::optional<at::Tensor> key_live) {
  c10::NoGradGuard no_grad_;
  AttnProblem F = make_launch(q, k, v, causal, dropout, seed, scale);
  check_key_mask(key_bias, key_live, q, F.B, F.Sk, &F.kbias, &F.klive);
  if (!(dout.dim() == 4 && view_ok(dout))) dout = dout.contiguous();
  if (!(o.dim() == 4 && view_ok(o))) o = o.contiguous();
  AttnBwd G;
  G.dout = view_of(dout, "dout");
  G.o = view_of(o, "o");
  G.dq = view_of(dq, "dq");
  G.dk = view_of(dk, "dk");
  G.dv = view_of(dv, "dv");
  for (const at::Tensor* t : {&dout, &o, &dq}) {
    TORCH_CHECK(t->sizes() == q.sizes(), "attn bwd: shape mismatch: o, dout and dq must be "
                "shaped like q ", q.sizes(), ", got ", t->sizes());
    TORCH_CHECK(t->scalar_type() == q.scalar_type(), "attn bwd: dtype mismatch");
  }
  for (const at::Tensor* t : {&dk, &dv}) {
    TORCH_CHECK(t->sizes() == k.sizes(), "attn bwd: shape mismatch: dk and dv must be shaped "
                "like k ", k.sizes(), ", got ", t->sizes());
    TORCH_CHECK(t->scalar_type() == q.scalar_type(), "attn bwd: dtype mismatch");
  }
  for (const at::Tensor* t : {&dout, &o, &dq, &dk, &dv})
    TORCH_CHECK(t->device() == q.device(), "attn bwd: every tensor must be on q's device");
  const int B = F.B, H = F.H, S = F.Sq, Sp = attn_lse_stride(F.Sq);
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.dim() == 3 && lse.size(0) == B &&
                  lse.size(1) == H && lse.size(2) == S && lse.device() == q.device(),
              "attn bwd: lse must be fp32 [B, H, Sq] on q's device");
  if (!(lse.stride(2) == 1 && lse.stride(1) == Sp && lse.stride(0) == (int64_t)H * Sp &&
        ((uintptr_t)lse.data_ptr() % 16) == 0)) {
    at::Tensor padded = at::empty({B, H, Sp}, lse.options());
    padded.narrow(2, 0, S).copy_(lse);
    lse = padded;
  }
  // masked: D is followed by the dQ kernel's guarded copy of lse for the dK/dV kernel
  at::Tensor D = at::empty({F.kbias ? 2 : 1, B, H, Sp}, lse.options());
  if (B * H == 0) return;
  if (F.Sk == 0) {  // no key: nothing reaches q
    dq.zero_();
    return;
  }
  if (S == 0) {  // no query: nothing reaches k / v
    dk.zero_();
    dv.zero_();
    return;
  }
  G.lse = lse.data_ptr<float>();
  G.D = D.data_ptr<float>();
  attn_bwd(F, G, cur_stream());
}

std::tuple<at::Tensor, at::Tensor> attn_fwd_varlen_op(at::Tensor q, at::Tensor k, at::Tensor v,
                                                      at::Tensor cu_seqlens, int64_t max_seqlen,
                                                      bool causal, double dropout, int64_t seed,
                                                      double scale) {
  c10::NoGradGuard no_grad_;
  AttnProblem L = make_varlen_launch(q, k, v, cu_seqlens, max_seqlen, causal, dropout, seed, scale);
  const int Sp = attn_lse_stride(L.Sq);
  at::Tensor o = at::empty({L.T, L.H, 64}, q.options());
  at::Tensor lse = at::empty({L.B, L.H, Sp}, q.options().dtype(at::kFloat));
  if (L.B == 0) o.zero_();  // no sequence owns any row
  else if (L.T > 0 && L.H > 0) attn_fwd(L, o.data_ptr(), lse.data_ptr<float>(), cur_stream());
  return {o, Sp == L.Sq ? lse : lse.narrow(2, 0, L.Sq)};
}

void attn_bwd_varlen_op(at::Tensor dout, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                        at::Tensor lse, at::Tensor cu_seqlens, int64_t max_seqlen, bool causal,
                        double dropout, int64_t seed, double scale, at::Tensor dq, at::Tensor dk,
                        at::Tensor dv) {
  c10::NoGradGuard no_grad_;
  AttnProblem F = make_varlen_launch(q, k, v, cu_seqlens, max_seqlen, causal, dropout, seed, scale);
  if (!(dout.dim() == 3 && view3_ok(dout))) dout = dout.contiguous();
  if (!(o.dim() == 3 && view3_ok(o))) o = o.contiguous();
  AttnBwd G;
  G.dout = view3_of(dout, "dout");
  G.o = view3_of(o, "o");
  G.dq = view3_of(dq, "dq");
  G.dk = view3_of(dk, "dk");
  G.dv = view3_of(dv, "dv");
  for (const at::Tensor* t : {&dout, &o, &dq, &dk, &dv}) {
    TORCH_CHECK(t->sizes() == q.sizes(), "attn varlen bwd: shape mismatch: o, dout, dq, dk and "
                "dv must be shaped like q ", q.sizes(), ", got ", t->sizes());
    TORCH_CHECK(t->scalar_type() == q.scalar_type(), "attn varlen bwd: dtype mismatch");
    TORCH_CHECK(t->device() == q.device(),
                "attn varlen bwd: every tensor must be on q's device");
  }
  const int B = F.B, H = F.H, S = F.Sq, Sp = attn_lse_stride(F.Sq);
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.dim() == 3 && lse.size(0) == B &&
                  lse.size(1) == H && lse.size(2) == S && lse.device() == q.device(),
              "attn varlen bwd: lse must be fp32 [B, H, max_seqlen] on q's device");
  if (!(lse.stride(2) == 1 && lse.stride(1) == Sp && lse.stride(0) == (int64_t)H * Sp &&
        ((uintptr_t)lse.data_ptr() % 16) == 0)) {
    at::Tensor padded = at::empty({B, H, Sp}, lse.options());
    padded.narrow(2, 0, S).copy_(lse);
    lse = padded;
  }
  at::Tensor D = at::empty({B, H, Sp}, lse.options());
  if (B == 0) {  // no sequence owns any row
    dq.zero_();
    dk.zero_();
    dv.zero_();
    return;
  }
  if (F.T == 0 || H == 0) return;
  G.lse = lse.data_ptr<float>();
  G.D = D.data_ptr<float>();
  attn_bwd(F, G, cur_stream());
}

}  // namespace amd
