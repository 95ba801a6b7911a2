"""Plain float64 references of the decode sampler and of the full-sequence attention, and the probe sets the kernel tests feed
them (tests/test_kernel_refs.py ties both to the oracle on the CPU; tests/test_gpu_kernel_sampler.py and
tests/test_gpu_kernel_attention.py compare the HIP kernels with them)."""
import numpy as np

N_LOGITS = 1025
EOS = 1024
SPL = 17                      # logits per lane of the sampler kernels: lane l owns [17 l, 17 l + 17)
P_MIN = 2.0 ** -12            # narrowest CDF interval the exact-token probes use (see test_gpu_kernel_sampler.py)


# ---- sampler --------------------------------------------------------------------------------------------------------------------
def reduce_partials(partial):
    """fp32 split-K reduction in the kernels' order ((p0 + p1) + p2) + p3; partial (splitk, 1025) float32"""
    p = np.asarray(partial, np.float32).reshape(-1, N_LOGITS)
    t = p[0].copy()
    for ks in range(1, p.shape[0]):
        t = (t + p[ks]).astype(np.float32)
    return t


def split_partials(row, splitk, rng):
    """random fp32 addends whose fp32 sum in the kernels' order is exactly `row` (-inf rides in the first addend)"""
    row = np.asarray(row, np.float32)
    if splitk == 1:
        return row[None].copy()
    fin = np.isfinite(row)
    parts = np.zeros((splitk, N_LOGITS), np.float32)
    parts[0, ~fin] = row[~fin]
    todo = fin.copy()
    for _ in range(64):
        # random leading addends; the last one closes the sum and is nudged until the fp32 sum in kernel order rounds back to `row`
        # (addends of the row's own magnitude: next to a much larger addend a small logit could not be hit to the last bit)
        parts[: splitk - 1, todo] = (rng.uniform(-0.9, 0.9, (splitk - 1, int(todo.sum()))) * row[todo]).astype(np.float32)
        parts[splitk - 1, todo] = 0.0
        for _ in range(6):
            got = reduce_partials(parts)
            bad = todo & (got != row)
            parts[splitk - 1, bad] = (parts[splitk - 1, bad] + (row[bad] - got[bad])).astype(np.float32)
        todo = fin & (reduce_partials(parts) != row)
        if not todo.any():
            return parts
    raise AssertionError("no exact split found")


def sampler_ref(logits, top_k, temperature):
    """models/vallex.py:836-853 on one reduced fp32 logit row.  The temperature quotient is fp32 (correctly rounded, as in torch and
    HIP: near-ties collapse exactly as on the device); the k-th largest is taken with multiplicity and `< kth` removed; softmax, CDF
    and log p in float64.  Returns (v fp32 after the quotient, kept bool mask, p float64, cdf float64)."""
    v = np.asarray(logits, np.float32).copy()
    if np.float32(temperature) != np.float32(1.0):
        v = (v / np.float32(temperature)).astype(np.float32)
    kept = np.ones(N_LOGITS, bool)
    if top_k > 0:
        k = min(max(int(top_k), 1), N_LOGITS)
        kth = np.sort(v)[::-1][k - 1]
        kept = ~(v < kth)
    kept &= np.isfinite(v)
    z = np.where(kept, v.astype(np.float64), -np.inf)
    e = np.exp(z - z.max())
    p = e / e.sum()
    return v, kept, p, np.cumsum(p)


def sample_token(p, cdf, u):
    """first index whose CDF exceeds u (never past the last token of non-zero probability)"""
    nz = np.flatnonzero(p > 0)
    return int(min(max(int(np.searchsorted(cdf, float(u), side="right")), nz[0]), nz[-1]))


def sampler_rows():
    """the chosen logit rows: dicts(name, logits fp32 (1025,), top_k, temperature, kept = number of kept tokens the reference's rule
    must leave (None: not pinned), filtered = at most 50 kept tokens)"""
    rows = []

    def add(name, lg, top_k, temperature=1.0, kept=None):
        rows.append(dict(name=name, logits=np.asarray(lg, np.float32), top_k=top_k, temperature=temperature, kept=kept,
                         filtered=kept is not None and kept <= 50))

    rng = np.random.default_rng(1711)
    add("all_equal", np.full(N_LOGITS, 0.75), 10, kept=N_LOGITS)
    lg = rng.permutation(np.linspace(-9.0, -1.0, N_LOGITS)).astype(np.float32)
    idx = rng.permutation(N_LOGITS)[:12]
    lg[idx[:7]] = [6.0, 5.5, 5.0, 4.5, 4.0, 3.5, 3.0]
    lg[idx[7:]] = 2.5                                                   # 8th .. 12th tie at the k-th level (k = 10)
    add("ties_at_kth", lg, 10, kept=12)
    lg = rng.permutation(np.linspace(-9.0, -1.0, N_LOGITS)).astype(np.float32)
    # the two largest of the other values sit at both ends of the row: a walk that counts the three tied maxima once keeps
    # them as 11th and 12th token, and then u = 0 and u = 1 - 2^-24 return them
    for end, val in ((0, np.float32(-1.0)), (EOS, np.sort(lg)[-2])):
        j = int(np.flatnonzero(lg == val)[0])
        lg[[end, j]] = lg[[j, end]]
    idx = 1 + rng.permutation(N_LOGITS - 2)[:10]
    lg[idx[:3]] = 4.2                                                   # 3 equal at the top, then 7 distinct: exactly 10
    lg[idx[3:]] = [3.9, 3.5, 3.1, 2.8, 2.3, 1.9, 1.4]
    add("ties_at_top", lg, 10, temperature=0.7, kept=10)
    lg = np.full(N_LOGITS, -np.inf, np.float32)
    lg[[0, 17, 1019, 1024]] = [1.0, 2.0, 0.5, 1.5]
    add("four_finite", lg, 10, kept=4)
    lg = rng.permutation(np.linspace(-9.0, -1.0, N_LOGITS)).astype(np.float32)
    lg[[0, 16, 17, 1019, 1020, 1024]] = [3.0, 3.6, 2.7, 3.3, 2.4, 3.9]
    add("lane_edges", lg, 6, kept=6)
    lg = rng.permutation(np.linspace(-9.0, -1.0, N_LOGITS)).astype(np.float32)
    lg[[5, 1024]] = 2.0
    add("two_maxima_k1", lg, 1, kept=2)
    normal = np.clip(rng.normal(0.0, 4.0, N_LOGITS), -11.0, 11.0).astype(np.float32)      # |logit / T| <= 16 down to T = 0.7
    for k in (-100, 1025, 1024):
        add(f"normal_k{k}", normal, k)
    for t in (1.0, 0.05, 100.0):
        add(f"normal_k50_T{t}", normal, 50, temperature=t, kept=50)
    return rows


def token_probes(p, cdf):
    """(token, u) for every token with p >= 2^-12: u = fp32(midpoint of its CDF interval)"""
    out = []
    for tok in np.flatnonzero(p >= P_MIN):
        lo = cdf[tok - 1] if tok else 0.0
        out.append((int(tok), np.float32(0.5 * (lo + cdf[tok]))))
    return out


# ---- LayerNorm / attention ------------------------------------------------------------------------------------------------------
def layer_norm_ref(x, g, b, eps=1e-5):
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def attention_ref(qkv, seq_len, prefix_len=None, heads=16, dh=64):
    """softmax(Q K^T / 8) V per (sequence, head) in float64 on packed rows qkv (sum len, 3 * 1024) = q | k | v.  prefix_len: keys
    < prefix are visible to every query, a query qi >= prefix also sees keys <= qi (models/vallex.py:535-549); None: no mask."""
    qkv = np.asarray(qkv, np.float64)
    d = heads * dh
    out = np.zeros((qkv.shape[0], d))
    off = 0
    for b, n in enumerate(seq_len):
        n = int(n)
        vis = np.ones((n, n), bool)
        if prefix_len is not None:
            s = int(prefix_len[b])
            qi, kj = np.arange(n)[:, None], np.arange(n)[None, :]
            vis = (kj < s) | ((qi >= s) & (kj <= qi))
        for h in range(heads):
            q = qkv[off:off + n, h * dh:(h + 1) * dh]
            k = qkv[off:off + n, d + h * dh:d + (h + 1) * dh]
            v = qkv[off:off + n, 2 * d + h * dh:2 * d + (h + 1) * dh]
            s_ = np.where(vis, q @ k.T / 8.0, -np.inf)
            e = np.exp(s_ - s_.max(-1, keepdims=True))
            out[off:off + n, h * dh:(h + 1) * dh] = (e / e.sum(-1, keepdims=True)) @ v
        off += n
    return out


def attention_fp32_yardstick(qkv, seq_len, prefix_len=None, heads=16, dh=64):
    """the reference's own arithmetic: torch-CPU fp32 softmax(Q K^T * 0.125) V with the same mask (modules/activation.py:142-167)"""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(qkv, np.float32))
    d = heads * dh
    out = torch.zeros(t.shape[0], d)
    off = 0
    for b, n in enumerate(seq_len):
        n = int(n)
        x = t[off:off + n]
        q, k, v = (x[:, i * d:(i + 1) * d].reshape(n, heads, dh).transpose(0, 1) for i in range(3))
        att = (q @ k.transpose(-2, -1)) * 0.125
        if prefix_len is not None:
            s = int(prefix_len[b])
            mask = torch.zeros(n, n, dtype=torch.bool)
            mask[:s, s:] = True
            mask[s:, s:] = torch.triu(torch.ones(n - s, n - s, dtype=torch.bool), diagonal=1)
            att = att.masked_fill(mask, float("-inf"))
        out[off:off + n] = (F.softmax(att, dim=-1) @ v).transpose(0, 1).reshape(n, d)
        off += n
    return out.numpy()


ATTN_LENS = (1, 31, 32, 33, 127, 128, 129, 161)
ATTN_PREFIX = (1, 1, 32, 33, 100, 128, 129, 64)
ATTN_QFIRST = (0, 30, 32, 1, 127, 128, 100, 129)


def attention_operands(kind, seed=5):
    """qkv (642, 3072) float32.  'uniform': uniform [-1, 1) with Q x 4 (the micro-benchmark's distribution); 'model': normal Q and K,
    V normal with per-channel gains from {0.01, 1, 30}; 'range': near the f16x2 range -- K = clipped normal x 40, V = clipped
    normal x 700, both within +-2000 (Q normal)."""
    rng = np.random.default_rng(seed)
    m = sum(ATTN_LENS)
    if kind == "uniform":
        x = rng.uniform(-1.0, 1.0, (m, 3072))
        x[:, :1024] *= 4.0
    elif kind == "model":
        x = rng.normal(0.0, 1.0, (m, 3072))
        x[:, 2048:] *= rng.choice([0.01, 1.0, 30.0], 1024)
    elif kind == "range":
        x = rng.normal(0.0, 1.0, (m, 3072))
        x[:, 1024:2048] = np.clip(x[:, 1024:2048] * 40.0, -2000.0, 2000.0)
        x[:, 2048:] = np.clip(x[:, 2048:] * 700.0, -2000.0, 2000.0)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)
