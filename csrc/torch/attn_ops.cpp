// Torch bindings for the fused attention kernels (csrc/hip/attention.hip at head dim 64,
// csrc/hip/attention_d128.hip at 128).
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

// the head dims that have kernels
bool head_dim_ok(int64_t D) { return D == 64 || D == 128; }

// the kernels' view of a [B,S,H,D] tensor (D = 64 or 128), or the reason it has none
AttnView view_of(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 4 && head_dim_ok(t.size(3)), "attn: ", what,
              " must be a [B,S,H,64] or [B,S,H,128] GPU tensor, got ", t.sizes());
  TORCH_CHECK(t.stride(3) == 1, "attn: ", what, ": head dim must be contiguous");
  TORCH_CHECK(view_ok(t), "attn: ", what, ": 16-byte aligned rows required");
  // the kernels' tile DMA uses 32-bit per-lane row offsets (csrc/hip/attention.hip)
  TORCH_CHECK(t.stride(1) >= 0 && t.stride(1) < (int64_t{1} << 24), "attn: ", what,
              ": sequence stride must be below 2^24 elements");
  return {t.data_ptr(), t.stride(0), t.stride(1), t.stride(2)};
}

// q [B, Sq, H, D], k / v [B, Sk, Hkv, D]: one B, D and dtype, any strides; Hkv divides H
// (grouped-query heads: query head h reads key/value head h / (H / Hkv))
AttnProblem make_launch(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                        bool causal, double dropout, int64_t seed, double scale) {
  AttnProblem L;
  L.q = view_of(q, "q");
  L.k = view_of(k, "k");
  L.v = view_of(v, "v");
  TORCH_CHECK(v.sizes() == k.sizes(), "attn: k and v shapes differ: ", k.sizes(), " and ",
              v.sizes());
  const int64_t H = q.size(2), Hkv = k.size(2);
  TORCH_CHECK(k.size(0) == q.size(0) && k.size(3) == q.size(3) &&
                  (Hkv == H || (Hkv > 0 && H % Hkv == 0)),
              "attn: q and k / v differ in batch or heads (or head dim): q ", q.sizes(), ", k ",
              k.sizes(), " (the sequence length may differ, and H = ", H,
              " query heads may share Hkv = ", Hkv, " key/value heads where Hkv divides H)");
  TORCH_CHECK(q.scalar_type() == k.scalar_type() && q.scalar_type() == v.scalar_type() &&
                  (q.scalar_type() == at::kBFloat16 || q.scalar_type() == at::kHalf),
              "attn: bf16/fp16 q,k,v of one dtype");
  TORCH_CHECK(k.device() == q.device() && v.device() == q.device(),
              "attn: q, k and v must be on one device");
  TORCH_CHECK(!causal || q.size(1) == k.size(1),
              "attn: causal is defined for equal query and key lengths only, got Sq = ",
              q.size(1), ", Sk = ", k.size(1));
  TORCH_CHECK(dropout >= 0.0 && dropout < 1.0, "attn: dropout must be in [0, 1)");
  L.B = (int)q.size(0); L.Sq = (int)q.size(1); L.Sk = (int)k.size(1); L.H = (int)H;
  L.Hkv = (int)Hkv; L.D = (int)q.size(3);
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

// the prepared pair mask of attn_prepare_attn_mask_op for a call's (B, Sq, Sk), shared
// (leading dim 1) or per batch element
void check_pair_mask(const at::Tensor& wq, const at::Tensor& cq, const at::Tensor& wk,
                     const at::Tensor& ck, const at::Tensor& q, AttnProblem& L) {
  TORCH_CHECK(L.Hkv == L.H, "attn: a pair mask is not combined with grouped-query heads (H = ",
              L.H, ", Hkv = ", L.Hkv, ")");
  const int64_t nq128 = (L.Sq + 127) / 128, nq64 = (L.Sq + 63) / 64;
  const int64_t nk128 = (L.Sk + 127) / 128, nk64 = (L.Sk + 63) / 64;
  const int64_t Bm = cq.dim() == 3 ? cq.size(0) : -1;
  TORCH_CHECK(Bm == 1 || Bm == L.B, "attn: the pair mask must be shared or hold B = ", L.B,
              " masks, got cq ", cq.sizes());
  auto ok = [&](const at::Tensor& t, at::ScalarType ty, std::initializer_list<int64_t> shape) {
    const bool word = t.scalar_type() == at::kUInt64 || t.scalar_type() == at::kLong;
    return t.is_cuda() && t.device() == q.device() && (ty == at::kLong ? word : t.scalar_type() == ty) &&
           t.sizes() == at::IntArrayRef(shape) && t.is_contiguous() &&
           (ty != at::kLong || ((uintptr_t)t.data_ptr() % 16) == 0);  // the words are DMA'd
  };
  TORCH_CHECK(ok(wq, at::kLong, {Bm, nq128, nk64, 128}) && ok(cq, at::kByte, {Bm, nq128, nk64}) &&
                  ok(wk, at::kLong, {Bm, nk128, nq64, 128}) && ok(ck, at::kByte, {Bm, nk128, nq64}),
              "attn: not the prepared pair mask (attn.prepare_attn_mask) of Sq = ", L.Sq,
              ", Sk = ", L.Sk, " on q's device: wq ", wq.sizes(), ", cq ", cq.sizes(), ", wk ",
              wk.sizes(), ", ck ", ck.sizes());
  L.wq = static_cast<const unsigned long long*>(wq.data_ptr());
  L.wk = static_cast<const unsigned long long*>(wk.data_ptr());
  L.cq = cq.data_ptr<unsigned char>();
  L.ck = ck.data_ptr<unsigned char>();
  L.pm_sb = Bm == 1 ? 0 : nq128 * nk64;
}

// ---- packed variable-length sequences: [T, H, D] views and an int32 offsets vector
bool view3_ok(const at::Tensor& t) {
  return t.stride(2) == 1 && ((uintptr_t)t.data_ptr() % 16) == 0 && t.stride(0) % 8 == 0 &&
         t.stride(1) % 8 == 0;
}

// the kernels' view of a packed [T,H,D] tensor (no batch stride), or the reason it has none
AttnView view3_of(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 3 && head_dim_ok(t.size(2)), "attn varlen: ", what,
              " must be a [T,H,64] or [T,H,128] GPU tensor, got ", t.sizes());
  TORCH_CHECK(t.stride(2) == 1, "attn varlen: ", what, ": head dim must be contiguous");
  TORCH_CHECK(view3_ok(t), "attn varlen: ", what, ": 16-byte aligned rows required");
  TORCH_CHECK(t.stride(0) >= 0 && t.stride(0) < (int64_t{1} << 24), "attn varlen: ", what,
              ": token stride must be below 2^24 elements");
  return {t.data_ptr(), 0, t.stride(0), t.stride(1)};
}

// q, k, v [T, H, D] of one T, H, D and dtype, any token / head strides; cu_seqlens int32
// [B + 1] on q's device; Sq = Sk = max_seqlen
AttnProblem make_varlen_launch(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                               const at::Tensor& cu, int64_t max_seqlen, bool causal,
                               double dropout, int64_t seed, double scale) {
  AttnProblem L;
  L.q = view3_of(q, "q");
  L.k = view3_of(k, "k");
  L.v = view3_of(v, "v");
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes(),
              "attn varlen: q, k and v differ in tokens or heads (or head dim): q ", q.sizes(), ", k ",
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
  L.B = (int)cu.size(0) - 1; L.H = L.Hkv = (int)q.size(1); L.D = (int)q.size(2);
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

std::tuple<at::Tensor, at::Tensor> attn_prepare_attn_mask_op(
    at::Tensor mask, c10::optional<at::Tensor> key_padding_mask) {
  c10::NoGradGuard no_grad_;
  auto bytes = [](const at::Tensor& t) {
    return t.scalar_type() == at::kBool || t.scalar_type() == at::kByte;
  };
  TORCH_CHECK(mask.is_cuda() && bytes(mask) && (mask.dim() == 2 || mask.dim() == 3) &&
                  mask.is_contiguous(),
              "attn.prepare_attn_mask: a contiguous bool / uint8 [Sq, Sk] or [B, Sq, Sk] GPU "
              "mask expected (non-zero = masked), got ", mask.scalar_type(), " ", mask.sizes());
  const int64_t Sq = mask.size(-2), Sk = mask.size(-1);
  TORCH_CHECK(Sq > 0 && Sk > 0 && Sq < (int64_t{1} << 24) && Sk < (int64_t{1} << 24),
              "attn.prepare_attn_mask: Sq, Sk must be in (0, 2^24), got ", mask.sizes());
  int64_t Bm = mask.dim() == 3 ? mask.size(0) : 1;
  const unsigned char* kpm = nullptr;
  if (key_padding_mask.has_value()) {
    const at::Tensor& kp = *key_padding_mask;
    TORCH_CHECK(kp.is_cuda() && kp.device() == mask.device() && bytes(kp) && kp.dim() == 2 &&
                    kp.size(1) == Sk && kp.is_contiguous() &&
                    (mask.dim() == 2 || kp.size(0) == Bm),
                "attn.prepare_attn_mask: key_padding_mask must be a contiguous bool / uint8 "
                "[B, Sk] tensor on the mask's device, got ", kp.scalar_type(), " ", kp.sizes());
    Bm = kp.size(0);
    kpm = static_cast<const unsigned char*>(kp.data_ptr());
  }
  TORCH_CHECK(Bm <= 65535, "attn.prepare_attn_mask: at most 65535 masks, got ", Bm);
  const int64_t nq128 = (Sq + 127) / 128, nq64 = (Sq + 63) / 64;
  const int64_t nk128 = (Sk + 127) / 128, nk64 = (Sk + 63) / 64;
  // one int64 buffer {wq, wk} and one uint8 buffer {cq, ck}; the Python side views them
  at::Tensor words = at::empty({Bm * 128 * (nq128 * nk64 + nk128 * nq64)},
                               mask.options().dtype(at::kLong));
  at::Tensor cls = at::empty({Bm * (nq128 * nk64 + nk128 * nq64)}, mask.options().dtype(at::kByte));
  if (Bm > 0) {
    auto* w = reinterpret_cast<unsigned long long*>(words.data_ptr<int64_t>());
    unsigned char* c = cls.data_ptr<unsigned char>();
    attn_prepare_pair_mask(static_cast<const unsigned char*>(mask.data_ptr()),
                           mask.dim() == 3 ? Sq * Sk : 0, kpm, (int)Bm, (int)Sq, (int)Sk, w, c,
                           w + Bm * 128 * nq128 * nk64, c + Bm * nq128 * nk64, cur_stream());
  }
  return {words, cls};
}

namespace {
std::tuple<at::Tensor, at::Tensor> run_fwd(AttnProblem& L, const at::Tensor& q);
void run_bwd(AttnProblem& F, at::Tensor dout, const at::Tensor& q, const at::Tensor& k,
             at::Tensor o, at::Tensor lse, at::Tensor dq, at::Tensor dk, at::Tensor dv);
}  // namespace

std::tuple<at::Tensor, at::Tensor> attn_fwd_amask_op(at::Tensor q, at::Tensor k, at::Tensor v,
                                                     double dropout, int64_t seed, double scale,
                                                     at::Tensor wq, at::Tensor cq, at::Tensor wk,
                                                     at::Tensor ck) {
  c10::NoGradGuard no_grad_;
  AttnProblem L = make_launch(q, k, v, false, dropout, seed, scale);
  check_pair_mask(wq, cq, wk, ck, q, L);
  return run_fwd(L, q);
}

void attn_bwd_amask_op(at::Tensor dout, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                       at::Tensor lse, double dropout, int64_t seed, double scale, at::Tensor dq,
                       at::Tensor dk, at::Tensor dv, at::Tensor wq, at::Tensor cq, at::Tensor wk,
                       at::Tensor ck) {
  c10::NoGradGuard no_grad_;
  AttnProblem F = make_launch(q, k, v, false, dropout, seed, scale);
  check_pair_mask(wq, cq, wk, ck, q, F);
  run_bwd(F, dout, q, k, o, lse, dq, dk, dv);
}

std::tuple<at::Tensor, at::Tensor> attn_fwd_op(at::Tensor q, at::Tensor k, at::Tensor v,
                                               bool causal, double dropout, int64_t seed,
                                               double scale, c10::optional<at::Tensor> key_bias,
                                               c10::optional<at::Tensor> key_live) {
  c10::NoGradGuard no_grad_;
  AttnProblem L = make_launch(q, k, v, causal, dropout, seed, scale);
  check_key_mask(key_bias, key_live, q, L.B, L.Sk, &L.kbias, &L.klive);
  return run_fwd(L, q);
}

namespace {
// the forward of a checked problem: allocation, the empty cases, the launch
std::tuple<at::Tensor, at::Tensor> run_fwd(AttnProblem& L, const at::Tensor& q) {
  const int Sp = attn_lse_stride(L.Sq);
  at::Tensor o = at::empty({L.B, L.Sq, L.H, L.D}, q.options());
  at::Tensor lse = at::empty({L.B, L.H, Sp}, q.options().dtype(at::kFloat));
  if (L.Sk == 0) {  // no key to attend to: o = 0, lse = log2(0), no launch
    o.zero_();
    lse.fill_(-std::numeric_limits<float>::infinity());
  } else if (L.Sq > 0 && L.B * L.H > 0) {
    attn_fwd(L, o.data_ptr(), lse.data_ptr<float>(), cur_stream());
  }
  return {o, Sp == L.Sq ? lse : lse.narrow(2, 0, L.Sq)};
}
}  // namespace

void attn_bwd_op(at::Tensor dout, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                 at::Tensor lse, bool causal, double dropout, int64_t seed, double scale,
                 at::Tensor dq, at::Tensor dk, at::Tensor dv, c10::optional<at::Tensor> key_bias,
                 c10::optional<at::Tensor> key_live) {
  c10::NoGradGuard no_grad_;
  AttnProblem F = make_launch(q, k, v, causal, dropout, seed, scale);
  check_key_mask(key_bias, key_live, q, F.B, F.Sk, &F.kbias, &F.klive);
  run_bwd(F, dout, q, k, o, lse, dq, dk, dv);
}

namespace {
// the backward of a checked problem: the buffers' checks, the workspace, the launches
void run_bwd(AttnProblem& F, at::Tensor dout, const at::Tensor& q, const at::Tensor& k,
             at::Tensor o, at::Tensor lse, at::Tensor dq, at::Tensor dk, at::Tensor dv) {
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
  at::Tensor D = at::empty({F.kbias || F.wq ? 2 : 1, B, H, Sp}, lse.options());
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
}  // namespace

std::tuple<at::Tensor, at::Tensor> attn_fwd_varlen_op(at::Tensor q, at::Tensor k, at::Tensor v,
                                                      at::Tensor cu_seqlens, int64_t max_seqlen,
                                                      bool causal, double dropout, int64_t seed,
                                                      double scale) {
  c10::NoGradGuard no_grad_;
  AttnProblem L = make_varlen_launch(q, k, v, cu_seqlens, max_seqlen, causal, dropout, seed, scale);
  const int Sp = attn_lse_stride(L.Sq);
  at::Tensor o = at::empty({L.T, L.H, L.D}, q.options());
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

namespace {
// The problem of a call over a contiguous 16-bit KV cache (attn_decode_op, attn_prefill_op),
// checked: views, shapes, one dtype and device, the lengths tensor, paired new rows.  `who`
// opens the messages.
AttnDecode cache_problem(const char* who, const at::Tensor& q, const at::Tensor& k_cache,
                         const at::Tensor& v_cache, const at::Tensor& cache_seqlens,
                         const c10::optional<at::Tensor>& k_new,
                         const c10::optional<at::Tensor>& v_new, double scale) {
  AttnDecode P;
  P.q = view_of(q, "q");
  P.k = view_of(k_cache, "k_cache");
  P.v = view_of(v_cache, "v_cache");
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes(), who, ": k_cache and v_cache shapes "
              "differ: ", k_cache.sizes(), " and ", v_cache.sizes());
  const int64_t B = q.size(0), Sq = q.size(1), H = q.size(2), D = q.size(3);
  const int64_t Smax = k_cache.size(1), Hkv = k_cache.size(2);
  TORCH_CHECK(k_cache.size(0) == B && k_cache.size(3) == D && Hkv > 0 && H % Hkv == 0,
              who, ": q and the caches differ in batch or head dim, or the heads do not "
              "split: q ", q.sizes(), ", k_cache ", k_cache.sizes());
  auto same = [&](const at::Tensor& t) {
    return t.scalar_type() == q.scalar_type() && t.device() == q.device();
  };
  TORCH_CHECK((q.scalar_type() == at::kBFloat16 || q.scalar_type() == at::kHalf) &&
                  same(k_cache) && same(v_cache),
              who, ": bf16/fp16 q and caches of one dtype on one device");
  TORCH_CHECK(cache_seqlens.is_cuda() && cache_seqlens.device() == q.device() &&
                  cache_seqlens.scalar_type() == at::kInt && cache_seqlens.dim() == 1 &&
                  cache_seqlens.size(0) == B && cache_seqlens.is_contiguous(),
              who, ": cache_seqlens must be a contiguous int32 [B] tensor on q's device, "
              "got ", cache_seqlens.scalar_type(), " ", cache_seqlens.sizes());
  TORCH_CHECK(k_new.has_value() == v_new.has_value(), who, ": k_new and v_new come as a pair");
  if (k_new.has_value()) {
    P.k_new = view_of(*k_new, "k_new");
    P.v_new = view_of(*v_new, "v_new");
    const std::vector<int64_t> dims{B, Sq, Hkv, D};
    const at::IntArrayRef want(dims);
    TORCH_CHECK(k_new->sizes() == want && v_new->sizes() == want && same(*k_new) && same(*v_new),
                who, ": k_new and v_new must be [B, Sq, Hkv, D] = ", want,
                " of q's dtype and device, got ", k_new->sizes(), " and ", v_new->sizes());
  }
  TORCH_CHECK(Smax < (int64_t{1} << 24) && Sq < (int64_t{1} << 24),
              who, ": Smax and Sq must be below 2^24");
  P.cache_seqlens = cache_seqlens.data_ptr<int32_t>();
  P.D = (int)D; P.B = (int)B; P.H = (int)H; P.Hkv = (int)Hkv; P.Sq = (int)Sq; P.Smax = (int)Smax;
  P.scale = (float)scale;
  P.dtype = dtype_of(q);
  return P;
}
}  // namespace

std::tuple<at::Tensor, at::Tensor> attn_decode_op(at::Tensor q, at::Tensor k_cache,
                                                  at::Tensor v_cache, at::Tensor cache_seqlens,
                                                  c10::optional<at::Tensor> k_new,
                                                  c10::optional<at::Tensor> v_new, double scale,
                                                  int64_t num_splits) {
  c10::NoGradGuard no_grad_;
  AttnDecode P = cache_problem("attn decode", q, k_cache, v_cache, cache_seqlens, k_new, v_new,
                               scale);
  const int64_t B = P.B, Sq = P.Sq, H = P.H, D = P.D, Hkv = P.Hkv;
  const int64_t R = H / Hkv * Sq;
  TORCH_CHECK(B * Hkv <= 65535 && (R + 31) / 32 <= 65535,
              "attn decode: batch x key/value heads = ", B * Hkv, " or rows per group = ", R,
              " exceeds a launch grid");
  TORCH_CHECK(num_splits >= 0 && num_splits <= kAttnDecodeMaxSplits,
              "attn decode: num_splits must be in [1, ", kAttnDecodeMaxSplits, "], got ",
              num_splits);
  at::Tensor o = at::empty({B, Sq, H, D}, q.options());
  at::Tensor lse = at::empty({B, H, Sq}, q.options().dtype(at::kFloat));
  if (B == 0 || Sq == 0) return {o, lse};
  int cus = 0;
  TORCH_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                    q.get_device()) == hipSuccess,
              "attn decode: cannot read the device's CU count");
  P.nsplit = num_splits > 0 ? (int)num_splits
                            : attn_decode_splits(P.B, P.Hkv, (int)R, P.Smax, cus);
  at::Tensor o_part, lse_part;
  if (P.nsplit > 1) {
    o_part = at::empty({P.nsplit, B, Sq, H, D}, q.options().dtype(at::kFloat));
    lse_part = at::empty({P.nsplit, B, H, Sq}, q.options().dtype(at::kFloat));
    P.o_part = o_part.data_ptr<float>();
    P.lse_part = lse_part.data_ptr<float>();
  }
  attn_decode(P, o.data_ptr(), lse.data_ptr<float>(), cur_stream());
  return {o, lse};
}

std::tuple<at::Tensor, at::Tensor> attn_prefill_op(at::Tensor q, at::Tensor k_cache,
                                                   at::Tensor v_cache, at::Tensor cache_seqlens,
                                                   c10::optional<at::Tensor> k_new,
                                                   c10::optional<at::Tensor> v_new, double scale) {
  c10::NoGradGuard no_grad_;
  AttnPrefill P;
  P.d = cache_problem("attn prefill", q, k_cache, v_cache, cache_seqlens, k_new, v_new, scale);
  const int64_t B = P.d.B, Sq = P.d.Sq, H = P.d.H, D = P.d.D, Hkv = P.d.Hkv;
  const int64_t tiles = (H / Hkv * Sq + 127) / 128;  // 128 rows of a key/value head's group each
  TORCH_CHECK(B <= 65535 && Hkv <= 65535 && tiles <= (int64_t{1} << 23) &&
                  tiles * Hkv * B < (int64_t{1} << 31),
              "attn prefill: batch ", B, ", ", Hkv, " key/value heads or their product with the ",
              tiles, " row tiles exceeds a launch grid");
  at::Tensor o = at::empty({B, Sq, H, D}, q.options());
  at::Tensor lse = at::empty({B, H, Sq}, q.options().dtype(at::kFloat));
  if (B == 0 || Sq == 0) return {o, lse};
  attn_prefill(P, o.data_ptr(), lse.data_ptr<float>(), cur_stream());
  return {o, lse};
}

namespace {
// The page pools and the table of a paged call, checked against B batch elements, Hkv heads
// and head dim D of `like`'s dtype and device: P.d.k / v (sb = the page stride), the table
// and the three page counts.  Returns Smax = max_pages * P.
int64_t paged_views(AttnDecodePaged& P, const at::Tensor& k_pages, const at::Tensor& v_pages,
                    const at::Tensor& block_table, const at::Tensor& like, int64_t B,
                    const char* who) {
  P.d.k = view_of(k_pages, "k_pages");
  P.d.v = view_of(v_pages, "v_pages");
  TORCH_CHECK(v_pages.sizes() == k_pages.sizes(), who, ": k_pages and v_pages shapes differ: ",
              k_pages.sizes(), " and ", v_pages.sizes());
  auto same = [&](const at::Tensor& t) {
    return t.scalar_type() == like.scalar_type() && t.device() == like.device();
  };
  TORCH_CHECK((like.scalar_type() == at::kBFloat16 || like.scalar_type() == at::kHalf) &&
                  same(k_pages) && same(v_pages),
              who, ": bf16/fp16 tensors and pages of one dtype on one device");
  const int64_t num_pages = k_pages.size(0), page = k_pages.size(1);
  TORCH_CHECK(page == 16 || page == 32 || page == 64 || page == 128 || page == 256, who,
              ": the page size must be 16, 32, 64, 128 or 256 rows, got ", page);
  TORCH_CHECK(num_pages > 0 && num_pages < (int64_t{1} << 31), who, ": the pool holds ",
              num_pages, " pages");
  TORCH_CHECK(block_table.is_cuda() && block_table.device() == like.device() &&
                  block_table.scalar_type() == at::kInt && block_table.dim() == 2 &&
                  block_table.size(0) == B && block_table.size(1) > 0 &&
                  block_table.is_contiguous(),
              who, ": block_table must be a contiguous int32 [B, max_pages] tensor on q's "
              "device, got ", block_table.scalar_type(), " ", block_table.sizes());
  const int64_t max_pages = block_table.size(1), Smax = max_pages * page;
  TORCH_CHECK(Smax < (int64_t{1} << 24), who, ": max_pages * page size must be below 2^24");
  // the kernels' per-lane byte offsets within a page are 32-bit
  TORCH_CHECK(page * k_pages.stride(1) * 2 < (int64_t{1} << 32) &&
                  page * v_pages.stride(1) * 2 < (int64_t{1} << 32),
              who, ": page size x row stride must stay below 2^32 bytes");
  P.block_table = block_table.data_ptr<int32_t>();
  P.num_pages = (int)num_pages;
  P.max_pages = (int)max_pages;
  P.log2_page = 0;
  while ((int64_t{1} << P.log2_page) < page) ++P.log2_page;
  return Smax;
}
}  // namespace

std::tuple<at::Tensor, at::Tensor> attn_decode_paged_op(
    at::Tensor q, at::Tensor k_pages, at::Tensor v_pages, at::Tensor block_table,
    at::Tensor cache_seqlens, c10::optional<at::Tensor> k_new, c10::optional<at::Tensor> v_new,
    double scale, int64_t num_splits) {
  c10::NoGradGuard no_grad_;
  AttnDecodePaged PP;
  AttnDecode& P = PP.d;
  P.q = view_of(q, "q");
  const int64_t B = q.size(0), Sq = q.size(1), H = q.size(2), D = q.size(3);
  TORCH_CHECK(k_pages.dim() == 4 && k_pages.size(3) == D && k_pages.size(2) > 0 &&
                  H % k_pages.size(2) == 0,
              "attn decode paged: q and the pages differ in head dim, or the heads do not "
              "split: q ", q.sizes(), ", k_pages ", k_pages.sizes());
  const int64_t Hkv = k_pages.size(2);
  const int64_t Smax = paged_views(PP, k_pages, v_pages, block_table, q, B, "attn decode paged");
  auto same = [&](const at::Tensor& t) {
    return t.scalar_type() == q.scalar_type() && t.device() == q.device();
  };
  TORCH_CHECK(cache_seqlens.is_cuda() && cache_seqlens.device() == q.device() &&
                  cache_seqlens.scalar_type() == at::kInt && cache_seqlens.dim() == 1 &&
                  cache_seqlens.size(0) == B && cache_seqlens.is_contiguous(),
              "attn decode paged: cache_seqlens must be a contiguous int32 [B] tensor on q's "
              "device, got ", cache_seqlens.scalar_type(), " ", cache_seqlens.sizes());
  TORCH_CHECK(k_new.has_value() == v_new.has_value(),
              "attn decode paged: k_new and v_new come as a pair");
  if (k_new.has_value()) {
    P.k_new = view_of(*k_new, "k_new");
    P.v_new = view_of(*v_new, "v_new");
    const std::vector<int64_t> dims{B, Sq, Hkv, D};
    const at::IntArrayRef want(dims);
    TORCH_CHECK(k_new->sizes() == want && v_new->sizes() == want && same(*k_new) && same(*v_new),
                "attn decode paged: k_new and v_new must be [B, Sq, Hkv, D] = ", want,
                " of q's dtype and device, got ", k_new->sizes(), " and ", v_new->sizes());
  }
  TORCH_CHECK(Sq < (int64_t{1} << 24), "attn decode paged: Sq must be below 2^24");
  const int64_t R = H / Hkv * Sq;
  TORCH_CHECK(B * Hkv <= 65535 && (R + 31) / 32 <= 65535,
              "attn decode paged: batch x key/value heads = ", B * Hkv, " or rows per group = ",
              R, " exceeds a launch grid");
  TORCH_CHECK(num_splits >= 0 && num_splits <= kAttnDecodeMaxSplits,
              "attn decode paged: num_splits must be in [1, ", kAttnDecodeMaxSplits, "], got ",
              num_splits);
  P.cache_seqlens = cache_seqlens.data_ptr<int32_t>();
  P.D = (int)D; P.B = (int)B; P.H = (int)H; P.Hkv = (int)Hkv; P.Sq = (int)Sq; P.Smax = (int)Smax;
  P.scale = (float)scale;
  P.dtype = dtype_of(q);
  at::Tensor o = at::empty({B, Sq, H, D}, q.options());
  at::Tensor lse = at::empty({B, H, Sq}, q.options().dtype(at::kFloat));
  if (B == 0 || Sq == 0) return {o, lse};
  int cus = 0;
  TORCH_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                    q.get_device()) == hipSuccess,
              "attn decode paged: cannot read the device's CU count");
  P.nsplit = num_splits > 0 ? (int)num_splits
                            : attn_decode_splits(P.B, P.Hkv, (int)R, P.Smax, cus);
  at::Tensor o_part, lse_part;
  if (P.nsplit > 1) {
    o_part = at::empty({P.nsplit, B, Sq, H, D}, q.options().dtype(at::kFloat));
    lse_part = at::empty({P.nsplit, B, H, Sq}, q.options().dtype(at::kFloat));
    P.o_part = o_part.data_ptr<float>();
    P.lse_part = lse_part.data_ptr<float>();
  }
  attn_decode_paged(PP, o.data_ptr(), lse.data_ptr<float>(), cur_stream());
  return {o, lse};
}

void attn_paged_append_op(at::Tensor k_new, at::Tensor v_new, at::Tensor k_pages,
                          at::Tensor v_pages, at::Tensor block_table, at::Tensor cache_seqlens) {
  c10::NoGradGuard no_grad_;
  AttnDecodePaged PP;
  AttnDecode& P = PP.d;
  P.k_new = view_of(k_new, "k_new");
  P.v_new = view_of(v_new, "v_new");
  const int64_t B = k_new.size(0), Sn = k_new.size(1), Hkv = k_new.size(2), D = k_new.size(3);
  TORCH_CHECK(v_new.sizes() == k_new.sizes() && v_new.scalar_type() == k_new.scalar_type() &&
                  v_new.device() == k_new.device(),
              "attn paged append: k_new and v_new differ: ", k_new.sizes(), " and ",
              v_new.sizes());
  TORCH_CHECK(k_pages.dim() == 4 && k_pages.size(2) == Hkv && k_pages.size(3) == D,
              "attn paged append: the new rows and the pages differ in heads or head dim: ",
              k_new.sizes(), " and ", k_pages.sizes());
  paged_views(PP, k_pages, v_pages, block_table, k_new, B, "attn paged append");
  TORCH_CHECK(cache_seqlens.is_cuda() && cache_seqlens.device() == k_new.device() &&
                  cache_seqlens.scalar_type() == at::kInt && cache_seqlens.dim() == 1 &&
                  cache_seqlens.size(0) == B && cache_seqlens.is_contiguous(),
              "attn paged append: cache_seqlens must be a contiguous int32 [B] tensor on the "
              "rows' device, got ", cache_seqlens.scalar_type(), " ", cache_seqlens.sizes());
  TORCH_CHECK(Sn < (int64_t{1} << 24) && B * Sn * Hkv * (D / 8) < (int64_t{1} << 39),
              "attn paged append: too many rows for one launch");
  P.cache_seqlens = cache_seqlens.data_ptr<int32_t>();
  P.D = (int)D; P.B = (int)B; P.Hkv = (int)Hkv;
  P.dtype = dtype_of(k_new);
  if (B == 0 || Sn == 0) return;
  attn_paged_append(PP, (int)Sn, cur_stream());
}

namespace {
// The FP8 caches and their scales, checked against B batch elements, Hkv heads and head dim D
// on `like`'s device: P.d.k / v (byte strides), the scale pointers and strides.  Returns Smax.
int64_t fp8_views(AttnDecodeFp8& P, const at::Tensor& k_cache, const at::Tensor& v_cache,
                  const at::Tensor& k_scale, const at::Tensor& v_scale, const at::Tensor& like,
                  int64_t B, int64_t Hkv, int64_t D, const char* who) {
  for (const at::Tensor* t : {&k_cache, &v_cache}) {
    TORCH_CHECK(t->is_cuda() && t->device() == like.device() && t->dim() == 4 &&
                    t->scalar_type() == at::kFloat8_e4m3fn,
                who, ": the caches must be float8_e4m3fn [B, Smax, Hkv, D] tensors on the GPU");
    TORCH_CHECK(t->stride(3) == 1 && ((uintptr_t)t->data_ptr() % 16) == 0 &&
                    t->stride(0) % 16 == 0 && t->stride(1) % 16 == 0 && t->stride(2) % 16 == 0,
                who, ": the caches need a contiguous head dim and 16-byte aligned rows");
    TORCH_CHECK(t->stride(1) >= 0 && t->stride(1) < (int64_t{1} << 24), who,
                ": the caches' sequence stride must be below 2^24 bytes");
  }
  TORCH_CHECK(head_dim_ok(D) && k_cache.size(0) == B && k_cache.size(2) == Hkv &&
                  k_cache.size(3) == D && v_cache.sizes() == k_cache.sizes(),
              who, ": k_cache and v_cache must be [B, Smax, Hkv, D] = [", B, ", Smax, ", Hkv,
              ", ", D, "], got ", k_cache.sizes(), " and ", v_cache.sizes());
  const int64_t Smax = k_cache.size(1);
  TORCH_CHECK(Smax < (int64_t{1} << 24), who, ": Smax must be below 2^24");
  for (const at::Tensor* t : {&k_scale, &v_scale})
    TORCH_CHECK(t->is_cuda() && t->device() == like.device() &&
                    t->scalar_type() == at::kFloat && t->dim() == 3 && t->size(0) == B &&
                    t->size(1) == Hkv && t->size(2) == Smax && t->stride(2) == 1,
                who, ": k_scale and v_scale must be fp32 [B, Hkv, Smax] = [", B, ", ", Hkv, ", ",
                Smax, "] with the key index contiguous, on the caches' device, got ", t->sizes());
  P.d.k = {k_cache.data_ptr(), k_cache.stride(0), k_cache.stride(1), k_cache.stride(2)};
  P.d.v = {v_cache.data_ptr(), v_cache.stride(0), v_cache.stride(1), v_cache.stride(2)};
  P.k_scale = k_scale.data_ptr<float>(); P.ks_sb = k_scale.stride(0); P.ks_sh = k_scale.stride(1);
  P.v_scale = v_scale.data_ptr<float>(); P.vs_sb = v_scale.stride(0); P.vs_sh = v_scale.stride(1);
  return Smax;
}
// cache_problem for an FP8 cache (attn_decode_fp8_op, attn_prefill_fp8_op): 16-bit q and new
// rows, the caches and scales through fp8_views, the lengths tensor, paired new rows.
AttnDecodeFp8 fp8_cache_problem(const char* who, const at::Tensor& q, const at::Tensor& k_cache,
                                const at::Tensor& v_cache, const at::Tensor& k_scale,
                                const at::Tensor& v_scale, const at::Tensor& cache_seqlens,
                                const c10::optional<at::Tensor>& k_new,
                                const c10::optional<at::Tensor>& v_new, double scale) {
  AttnDecodeFp8 PP;
  AttnDecode& P = PP.d;
  P.q = view_of(q, "q");
  const int64_t B = q.size(0), Sq = q.size(1), H = q.size(2), D = q.size(3);
  TORCH_CHECK(q.scalar_type() == at::kBFloat16 || q.scalar_type() == at::kHalf,
              who, ": q must be bf16 or fp16");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(2) > 0 && H % k_cache.size(2) == 0,
              who, ": the heads do not split: q ", q.sizes(), ", k_cache ", k_cache.sizes());
  const int64_t Hkv = k_cache.size(2);
  const int64_t Smax = fp8_views(PP, k_cache, v_cache, k_scale, v_scale, q, B, Hkv, D, who);
  auto same = [&](const at::Tensor& t) {
    return t.scalar_type() == q.scalar_type() && t.device() == q.device();
  };
  TORCH_CHECK(cache_seqlens.is_cuda() && cache_seqlens.device() == q.device() &&
                  cache_seqlens.scalar_type() == at::kInt && cache_seqlens.dim() == 1 &&
                  cache_seqlens.size(0) == B && cache_seqlens.is_contiguous(),
              who, ": cache_seqlens must be a contiguous int32 [B] tensor on q's device, got ",
              cache_seqlens.scalar_type(), " ", cache_seqlens.sizes());
  TORCH_CHECK(k_new.has_value() == v_new.has_value(), who, ": k_new and v_new come as a pair");
  if (k_new.has_value()) {
    P.k_new = view_of(*k_new, "k_new");
    P.v_new = view_of(*v_new, "v_new");
    const std::vector<int64_t> dims{B, Sq, Hkv, D};
    const at::IntArrayRef want(dims);
    TORCH_CHECK(k_new->sizes() == want && v_new->sizes() == want && same(*k_new) && same(*v_new),
                who, ": k_new and v_new must be [B, Sq, Hkv, D] = ", want,
                " of q's dtype and device, got ", k_new->sizes(), " and ", v_new->sizes());
  }
  TORCH_CHECK(Sq < (int64_t{1} << 24), who, ": Sq must be below 2^24");
  P.cache_seqlens = cache_seqlens.data_ptr<int32_t>();
  P.D = (int)D; P.B = (int)B; P.H = (int)H; P.Hkv = (int)Hkv; P.Sq = (int)Sq; P.Smax = (int)Smax;
  P.scale = (float)scale;
  P.dtype = dtype_of(q);
  return PP;
}
}  // namespace

std::tuple<at::Tensor, at::Tensor> attn_decode_fp8_op(
    at::Tensor q, at::Tensor k_cache, at::Tensor v_cache, at::Tensor k_scale, at::Tensor v_scale,
    at::Tensor cache_seqlens, c10::optional<at::Tensor> k_new, c10::optional<at::Tensor> v_new,
    double scale, int64_t num_splits) {
  c10::NoGradGuard no_grad_;
  AttnDecodeFp8 PP = fp8_cache_problem("attn decode fp8", q, k_cache, v_cache, k_scale, v_scale,
                                       cache_seqlens, k_new, v_new, scale);
  AttnDecode& P = PP.d;
  const int64_t B = P.B, Sq = P.Sq, H = P.H, D = P.D, Hkv = P.Hkv;
  const int64_t R = H / Hkv * Sq;
  TORCH_CHECK(B * Hkv <= 65535 && (R + 31) / 32 <= 65535,
              "attn decode fp8: batch x key/value heads = ", B * Hkv, " or rows per group = ", R,
              " exceeds a launch grid");
  TORCH_CHECK(num_splits >= 0 && num_splits <= kAttnDecodeMaxSplits,
              "attn decode fp8: num_splits must be in [1, ", kAttnDecodeMaxSplits, "], got ",
              num_splits);
  at::Tensor o = at::empty({B, Sq, H, D}, q.options());
  at::Tensor lse = at::empty({B, H, Sq}, q.options().dtype(at::kFloat));
  if (B == 0 || Sq == 0) return {o, lse};
  int cus = 0;
  TORCH_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                    q.get_device()) == hipSuccess,
              "attn decode fp8: cannot read the device's CU count");
  P.nsplit = num_splits > 0 ? (int)num_splits
                            : attn_decode_splits(P.B, P.Hkv, (int)R, P.Smax, cus);
  at::Tensor o_part, lse_part;
  if (P.nsplit > 1) {
    o_part = at::empty({P.nsplit, B, Sq, H, D}, q.options().dtype(at::kFloat));
    lse_part = at::empty({P.nsplit, B, H, Sq}, q.options().dtype(at::kFloat));
    P.o_part = o_part.data_ptr<float>();
    P.lse_part = lse_part.data_ptr<float>();
  }
  attn_decode_fp8(PP, o.data_ptr(), lse.data_ptr<float>(), cur_stream());
  return {o, lse};
}

std::tuple<at::Tensor, at::Tensor> attn_prefill_fp8_op(
    at::Tensor q, at::Tensor k_cache, at::Tensor v_cache, at::Tensor k_scale, at::Tensor v_scale,
    at::Tensor cache_seqlens, c10::optional<at::Tensor> k_new, c10::optional<at::Tensor> v_new,
    double scale) {
  c10::NoGradGuard no_grad_;
  const AttnDecodeFp8 PP = fp8_cache_problem("attn prefill fp8", q, k_cache, v_cache, k_scale,
                                             v_scale, cache_seqlens, k_new, v_new, scale);
  const int64_t B = PP.d.B, Sq = PP.d.Sq, H = PP.d.H, D = PP.d.D, Hkv = PP.d.Hkv;
  const int64_t tiles = (H / Hkv * Sq + 127) / 128;  // 128 rows of a key/value head's group each
  TORCH_CHECK(B <= 65535 && Hkv <= 65535 && tiles <= (int64_t{1} << 23) &&
                  tiles * Hkv * B < (int64_t{1} << 31),
              "attn prefill fp8: batch ", B, ", ", Hkv, " key/value heads or their product with "
              "the ", tiles, " row tiles exceeds a launch grid");
  at::Tensor o = at::empty({B, Sq, H, D}, q.options());
  at::Tensor lse = at::empty({B, H, Sq}, q.options().dtype(at::kFloat));
  if (B == 0 || Sq == 0) return {o, lse};
  attn_prefill_fp8(PP, o.data_ptr(), lse.data_ptr<float>(), cur_stream());
  return {o, lse};
}

void attn_fp8_append_op(at::Tensor k_new, at::Tensor v_new, at::Tensor k_cache,
                        at::Tensor v_cache, at::Tensor k_scale, at::Tensor v_scale,
                        at::Tensor cache_seqlens) {
  c10::NoGradGuard no_grad_;
  AttnDecodeFp8 PP;
  AttnDecode& P = PP.d;
  P.k_new = view_of(k_new, "k_new");
  P.v_new = view_of(v_new, "v_new");
  const int64_t B = k_new.size(0), Sn = k_new.size(1), Hkv = k_new.size(2), D = k_new.size(3);
  TORCH_CHECK((k_new.scalar_type() == at::kBFloat16 || k_new.scalar_type() == at::kHalf) &&
                  v_new.sizes() == k_new.sizes() && v_new.scalar_type() == k_new.scalar_type() &&
                  v_new.device() == k_new.device(),
              "attn fp8 append: k_new and v_new must be bf16 / fp16 tensors of one shape, dtype "
              "and device, got ", k_new.sizes(), " and ", v_new.sizes());
  const int64_t Smax = fp8_views(PP, k_cache, v_cache, k_scale, v_scale, k_new, B, Hkv, D,
                                 "attn fp8 append");
  TORCH_CHECK(cache_seqlens.is_cuda() && cache_seqlens.device() == k_new.device() &&
                  cache_seqlens.scalar_type() == at::kInt && cache_seqlens.dim() == 1 &&
                  cache_seqlens.size(0) == B && cache_seqlens.is_contiguous(),
              "attn fp8 append: cache_seqlens must be a contiguous int32 [B] tensor on the "
              "rows' device, got ", cache_seqlens.scalar_type(), " ", cache_seqlens.sizes());
  TORCH_CHECK(Sn < (int64_t{1} << 24) && B * Sn * Hkv * (D / 8) < (int64_t{1} << 39),
              "attn fp8 append: too many rows for one launch");
  P.cache_seqlens = cache_seqlens.data_ptr<int32_t>();
  P.D = (int)D; P.B = (int)B; P.Hkv = (int)Hkv; P.Smax = (int)Smax;
  P.dtype = dtype_of(k_new);
  if (B == 0 || Sn == 0) return;
  attn_fp8_append(PP, (int)Sn, cur_stream());
}

}  // namespace amd
