"""float64 references of the fused softmax cross entropy (csrc/hip/xentropy.hip), shared
by tests/test_xent_ref_cpu.py (the references are right, the extension's CPU branch matches
them, wrong variants miss them) and tests/test_xentropy_gpu.py (the kernels match them).
Same scheme as tests/optim_ref.py, whose ``Val``, ``bound``, ``assert_within``,
``worst_ratio``, ``emulation_ratio``, ``K`` and ``EPS32`` are used as they are.

Every function takes the logits AS STORED (fp32 / fp16 / bf16 [N, V]) and upcasts:

  forward   lse = log sum_j exp(x_j);  loss = lse - (1 - eps)*x[label] - eps*mean(x);
            loss = 0 for an ignored row (label == padding_idx, < 0 or >= V); lse is defined
            there too.  Without smoothing the mean does not enter: a row with -inf logits
            (a masked vocabulary) has a finite loss as long as x[label] is finite.
  backward  dx = g*(exp(x - lse) - eps/V - (1 - eps)*onehot(label)), g = 0 for an ignored
            row, with the lse AS STORED by the forward (its error is not charged twice).

Error magnitudes, read off xent_fwd_k / xent_bwd_k (units of eps32, see optim_ref):

  lse   The kernel keeps (m, s) = (running max, sum of 2^(x*log2e - m)) per thread and
        merges pairs; lse = (M + log2 S) / log2e.  Any rounding of a running maximum
        cancels (it is subtracted inside every exponent and added back at the end), so the
        errors are: the final sum M + log2 S, rounded at its own magnitude, and log2f (2
        ulp) at |log2 S| <= (|lse| + |max x|)*log2e - this is where the magnitude
        |max x|*log2e enters; the division by log2e (|lse|); and the relative error of S.
        S: a vector's partial sum has 8 exp2f (2 ulp) and 7 additions (11 units), every
        exponent's fma one rounding at |x_j*log2e - m|, which weighted by the softmax is at
        most the row's entropy <= log V (2 log V with the merges' own m - m2); a merge
        costs exp2f, a product and a sum (7 units), and an element passes through
        ``chain`` = ceil(nvec/256) + 2 (a head and a tail step) + 6 shuffle levels + 4
        waves of them, nvec = V // 8:
                   e_lse = 4|lse| + 2|max x| + 7*chain + 11 + 2 log V
  tot   a plain fp32 sum of V terms in the same geometry (8 additions per vector step):
        chain_tot = 8*ceil(nvec/256) + 2 + 10, e = chain_tot * sum|x|.
  loss  the three terms combined in fp32 as the kernel does (Val arithmetic):
        lse - (1 - eps)*x[label] - (eps*tot)/V.
  dx    p = exp2(x*log2e - L2), L2 = lse*log2e rounded once at its own magnitude (|lse|
        relative to p), the fma's rounding and the fp32 log2e at |x - lse| (2|x - lse|),
        exp2f's 2 ulp (4): e_p = p*(|lse| + 2|x - lse| + 4) + p; then
        g*(p - eps/V - (1 - eps)*onehot) in Val arithmetic.

K stays optim_ref.K = 4.  The float32 emulation of the documented algorithm
(``online_fwd``: the same partition into 256 threads, heads, 8-vectors and tails, the same
merge, shuffle tree and wave loop, in float32 on the CPU) measures how much of the budget
the algorithm itself uses (tests/test_xent_ref_cpu.py::test_emulation_ratio asserts < 1;
worst over every row maker, type, width and head length): lse 0.16, loss 0.14; backward
(``ref_xent_bwd`` itself in float32): dx 0.45.  K = 4 leaves the emulation at about a
tenth of the bound.  Measured on an MI355X (tests/test_xentropy_gpu.py, fp32 storage, where
the rounding to the storage type does not hide it): lse 0.03, loss 0.02, dx 0.11; with
16-bit outputs the ratio is that of the final rounding, just under 1.
"""
import math

import torch

from optim_ref import (EPS32, K, Val, assert_within, bound, emulation_ratio, f32,  # noqa: F401
                       worst_ratio)

F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
THREADS = 256           # kXT
LOG2E = 1.4426950408889634


def _cdiv(a, b):
    return -(-int(a) // int(b))


def xent_chain(V):
    return float(_cdiv(V // 8, THREADS) + 2 + 6 + 4)


def tot_chain(V):
    return float(8 * _cdiv(V // 8, THREADS) + 2 + 6 + 4)


def ignored(labels, padding_idx, V):
    return (labels == padding_idx) | (labels < 0) | (labels >= V)


def row_split(ptr, V, esize, vec_ok=True):
    """xentropy.hip row_split for a row that starts at address ``ptr``: (head, nvec)."""
    if not vec_ok:
        return 0, 0
    E = 16 // esize
    mis = (ptr % 16) // esize
    head = min(E - mis if mis else 0, V)
    return head, (V - head) // 8


def row_heads(x):
    """(head, nvec) of every row of a contiguous [N, V] tensor at its real address."""
    N, V = x.shape
    es = x.element_size()
    return [row_split(x.data_ptr() + r * V * es, V, es) for r in range(N)]


# --------------------------------------------------------------------------- references
def ref_xent_fwd(x, labels, smoothing, padding_idx):
    """-> (loss, lse): Vals [N] in float64."""
    X = x.detach().to(F64)
    N, V = X.shape
    lab = labels.detach().to(torch.int64).to(X.device)
    sm = f32(smoothing)
    lse_v = torch.logsumexp(X, 1)
    mx = X.max(1).values
    e_lse = 4 * lse_v.abs() + 2 * mx.abs() + 7 * xent_chain(V) + 11 + 2 * math.log(V)
    lse = Val(lse_v, e_lse)
    ign = ignored(lab, padding_idx, V)
    safe = torch.where(ign, torch.zeros_like(lab), lab)
    xl = Val(X.gather(1, safe.unsqueeze(1)).squeeze(1))
    loss = lse - (lse.const(1.0) - sm) * xl
    if sm != 0.0:
        tot = Val(X.sum(1), tot_chain(V) * X.abs().sum(1))
        loss = loss - (tot * sm) / float(V)
    zero = torch.zeros_like(loss.v)
    return Val(torch.where(ign, zero, loss.v), torch.where(ign, zero, loss.e)), lse


def ref_xent_bwd(dloss, x, lse_stored, labels, smoothing, padding_idx, work=F64):
    """-> {"dx": Val like x}."""
    X = x.detach().to(work)
    N, V = X.shape
    lab = labels.detach().to(torch.int64).to(X.device)
    sm = f32(smoothing)
    L = lse_stored.detach().to(work).reshape(N, 1)
    ign = ignored(lab, padding_idx, V)
    g = torch.where(ign, torch.zeros(N, dtype=work, device=X.device),
                    dloss.detach().to(work).reshape(N))
    p = (X - L).exp()
    diff = torch.where(p > 0, (X - L).abs(), torch.zeros_like(p))    # exp(-inf) = 0 exactly
    P = Val(p, p * (L.abs() + 2 * diff + 4) + p)
    onehot = torch.zeros_like(X)
    safe = torch.where(ign, torch.zeros_like(lab), lab)
    onehot.scatter_(1, safe.unsqueeze(1), 1.0)
    t = P - P.const(sm) / float(V)
    on = Val(onehot) * (P.const(1.0) - sm)
    # an exact zero is subtracted exactly
    t2 = t - on
    t = Val(t2.v, torch.where(onehot > 0, t2.e, t.e))
    return {"dx": Val(g.reshape(N, 1)) * t}


# --------------------------------------------------------------------------- emulation
def _merge(m, s, m2, s2, variant):
    """lse_merge of xentropy.hip on tensors.  variant "drop_s": forgets s when m2 > m;
    "no_guard": without the -inf early returns."""
    ninf = float("-inf")
    e1 = torch.exp2(m - m2)
    e2 = torch.exp2(m2 - m)
    s_gt = s2 if variant == "drop_s" else s * e1 + s2
    s_le = s + s2 * e2
    gt = m2 > m
    ms, ss = torch.where(gt, m2, m), torch.where(gt, s_gt, s_le)
    if variant == "no_guard":
        return ms, ss
    keep = m2 == ninf
    take = (m == ninf) & ~keep
    ms = torch.where(keep, m, torch.where(take, m2, ms))
    ss = torch.where(keep, s, torch.where(take, s2, ss))
    return ms, ss


def online_fwd(x, labels, smoothing, padding_idx, heads=None, work=F32, variant="ok",
               smooth_div=None, ref=None):
    """xent_fwd_k's algorithm in ``work`` precision on the CPU: rows split at ``heads``
    (per-row (head, nvec); aligned rows by default) over 256 threads.  The values carry the
    REFERENCE's error magnitudes, so that ``emulation_ratio`` and ``worst_ratio`` apply.
    ``smooth_div``: the WRONG divisor V - 1 for the smoothing term.
    -> {"loss": Val [N], "lse": Val [N]}."""
    N, V = x.shape
    X = x.detach().to(work)
    l2e = torch.tensor(LOG2E, dtype=F32).to(work)     # kL2E, the kernel's fp32 constant
    ninf = float("-inf")
    heads = heads or [(0, V // 8)] * N
    T = THREADS
    m = torch.full((N, T), ninf, dtype=work)
    s = torch.zeros(N, T, dtype=work)
    tot = torch.zeros(N, T, dtype=work)
    for r in range(N):
        head, nvec = heads[r]
        row = X[r]
        if head:
            m[r, :head], s[r, :head], tot[r, :head] = row[:head] * l2e, 1.0, row[:head]
        body = row[head:head + nvec * 8].reshape(nvec, 8)
        for it in range(_cdiv(nvec, T)):
            v = body[it * T:(it + 1) * T]
            n = v.shape[0]
            vm = v.max(1).values
            t = tot[r, :n]
            for j in range(8):
                t = t + v[:, j]
            tot[r, :n] = t
            vm2 = vm * l2e
            ps = torch.zeros(n, dtype=work)
            for j in range(8):
                ps = ps + torch.exp2(v[:, j] * l2e - vm2)
            m[r, :n], s[r, :n] = _merge(m[r, :n].clone(), s[r, :n].clone(), vm2, ps, variant)
        tail = row[head + nvec * 8:]
        for it in range(_cdiv(tail.numel(), T)):
            v = tail[it * T:(it + 1) * T]
            n = v.numel()
            m[r, :n], s[r, :n] = _merge(m[r, :n].clone(), s[r, :n].clone(), v * l2e,
                                        torch.ones(n, dtype=work), variant)
            tot[r, :n] = tot[r, :n] + v
    idx = torch.arange(T)
    for off in (32, 16, 8, 4, 2, 1):
        partner = idx ^ off
        m, s = _merge(m, s, m[:, partner], s[:, partner], variant)
        tot = tot + tot[:, partner]
    M, S, TT = m[:, 0], s[:, 0], tot[:, 0]
    for w in range(1, T // 64):
        M, S = _merge(M, S, m[:, 64 * w], s[:, 64 * w], variant)
        TT = TT + tot[:, 64 * w]
    lse = (M + torch.log2(S)) / l2e
    lab = labels.to(torch.int64)
    ign = ignored(lab, padding_idx, V)
    safe = torch.where(ign, torch.zeros_like(lab), lab)
    xl = X.gather(1, safe.unsqueeze(1)).squeeze(1)
    sm = torch.tensor(f32(smoothing), dtype=work)
    loss = lse - (1 - sm) * xl
    if float(sm) != 0.0:
        loss = loss - sm * TT / float(smooth_div or V)
    loss = torch.where(ign, torch.zeros_like(loss), loss)
    if ref is None:
        ref = ref_xent_fwd(x, labels, smoothing, padding_idx)
    return {"loss": Val(loss, ref[0].e), "lse": Val(lse, ref[1].e)}


def naive_lse(x, work=F32):
    """The WRONG unshifted log(sum(exp(x))) in ``work`` precision."""
    return x.detach().to(work).exp().sum(1).log()


# --------------------------------------------------------------------------- row makers
def _gen(seed):
    return torch.Generator().manual_seed(7919 * seed + 17)


def randn_rows(N, V, dtype, seed=0, scale=3.0):
    return (torch.randn(N, V, generator=_gen(seed)) * scale).to(dtype)


def max_positions(V, head, nvec):
    """The positions ``max_at`` is asked for: in the head, the body, the tail, the last
    element (those that exist for this row split)."""
    pos = {V - 1, 0}
    if head:
        pos.add(head - 1)
    if nvec:
        pos.add(head + min(nvec * 8 - 1, 8 * (nvec // 2) + 3))
    if head + nvec * 8 < V:
        pos.add(head + nvec * 8)
    return sorted(pos)


def max_at(N, V, pos, dtype, seed=0):
    """randn rows whose unique maximum (by 9) sits at column ``pos``."""
    x = torch.randn(N, V, generator=_gen(seed + 1))
    x[:, pos] = 12.0
    return x.to(dtype)


def neg_inf_vectors(x, heads):
    """In place.  Row 0: one whole aligned 8-vector of -inf (the body's second vector, or
    its first).  Row 1: every element thread 1 owns (its head element, its vectors, its
    tail elements).  Row 2: all but one element.  Rows as the split ``heads`` places them;
    widths without a body get the elements they have."""
    N, V = x.shape
    ninf = float("-inf")
    for r in range(min(N, 3)):
        head, nvec = heads[r]
        keep = x[r, V // 2].clone()
        if r == 0:
            if nvec:
                i = 1 if nvec > 1 else 0
                x[r, head + 8 * i:head + 8 * i + 8] = ninf
            else:
                x[r, :V - 1] = ninf
        elif r == 1:
            t = 1
            if t < head:
                x[r, t] = ninf
            for i in range(t, nvec, THREADS):
                x[r, head + 8 * i:head + 8 * i + 8] = ninf
            for j in range(head + nvec * 8 + t, V, THREADS):
                x[r, j] = ninf
        else:
            x[r, :] = ninf
            x[r, V // 2] = keep
        if bool((x[r] == ninf).all()):
            x[r, V // 2] = keep if float(keep) != ninf else 0.0
    return x


def offset_value(dtype):
    """The largest offset at which ``dtype`` still resolves unit differences: the spacing
    of the type is eps * 2^e, which reaches 1 at 1 / eps."""
    return 1.0 / torch.finfo(dtype).eps


def offset(N, V, dtype, sign=1.0, seed=0):
    """randn + c, c = +-offset_value(dtype) (values collapse onto the integers near c)."""
    c = sign * offset_value(dtype)
    return (torch.randn(N, V, generator=_gen(seed + 2)).to(F64) + c).to(dtype)


def flat(N, V, dtype, value=1.5):
    """All elements equal: lse = value + log V exactly, loss = log V."""
    return torch.full((N, V), value).to(dtype)


def labels_for(N, V, padding_idx, seed=0):
    """Random labels with the last rows at padding_idx, -5, V and V - 1 (where N allows),
    and rows 0 / 1 at the first and the last-but-first columns (head / tail)."""
    lab = torch.randint(0, V, (N,), generator=_gen(seed + 3))
    lab[0] = 0
    if N > 1:
        lab[1] = V - 1
    special = [padding_idx, -5, V, V - 1]
    for i, v in enumerate(special[:max(N - 2, 0)]):
        lab[N - 1 - i] = v
    return lab


def finite_labels(x):
    """A label per row whose logit is finite (the row's maximum): for the -inf rows."""
    return x.detach().float().argmax(1)


def carve(x, off, device):
    """x [N, V] placed ``off`` elements into a flat buffer on ``device``."""
    N, V = x.shape
    buf = torch.empty(N * V + off, dtype=x.dtype, device=device)
    v = buf[off:].view(N, V)
    v.copy_(x)
    return v


WIDTHS = [1, 5, 7, 8, 9, 2047, 2048, 2049, 4099]
BIG_V = 50257
