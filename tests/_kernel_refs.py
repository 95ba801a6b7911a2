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


# ---- the attention block of one decode step (dec_attn chains, csrc/decode.hip) -----------------------------------------------------
DEC_TILE = 128                # rows of one dec_attn tile
DEC_TMAX = 384                # arena rows per (slot, head) the tests ask vx_dev_dec_attn for: three tiles
DEC_ROWS = (1, 2, 3, 4, 5, 7, 8, 9, 11, 16, 17, 32)
# contexts INCLUDING the new token, long and short alternating
DEC_CTX = (300, 1, 257, 2, 130, 16, 129, 17, 128, 18, 127, 33)
DEC_KINDS = ("uniform", "model", "sharp", "new_heavy", "new_light")


def dec_geometry(nrows, identity=True, sb_fuse=1, sb_qkv_rows=4, sb_qkv_nsplit=0, fuse_out=1, fuse_split=1, att_nsplit_force=0):
    """(chain, context splits) the engine's rule picks (engine.hip decode_geometry), restated statement by statement with the switches
    a context reads (weights.hip; the names are the fields vx_dev_switches reports, fuse_out after the Tmax rule).  With no switch: the
    default table.  Chains: 'sb_qkv' (norm1 + QKV inside the attention launch, <= 4 rows), 'sb' (the small-batch chain without the fused
    QKV: unfused dec_attn, the combine in the prologue of out_proj), 'unfused' (dec_attn | combine if there are splits | out_proj),
    'split_fused' (out_proj inside dec_attn, 2 .. 4 context splits), 'fused' (out_proj inside dec_attn, one split)."""
    nsplit = max(1, min(16, 512 // (nrows * 16)))
    if 4 < nrows <= 16:
        nsplit = max(2, 256 // (nrows * 16))
    split_fused = False
    if fuse_out and fuse_split == 1 and 8 <= nrows <= 16:
        ns = min(4, 256 // (16 * ((nrows + 1) // 2)))
        if ns >= 2:
            nsplit, split_fused = ns, True
    if att_nsplit_force > 0:
        nsplit = att_nsplit_force
        split_fused = bool(fuse_out) and fuse_split != 0 and nrows > 4 and 2 <= nsplit <= 4       # any non-zero fuse_split, as the code has it
    sb_chain = sb_qkv = False
    if sb_fuse and nrows <= 4 and identity:
        nsplit, sb_chain = (16 if nrows <= 2 else 8), True              # sb_chain_supported: 16 and 8 splits are instantiated
        if nrows <= sb_qkv_rows:
            ns2 = sb_qkv_nsplit if sb_qkv_nsplit > 0 else (16, 8, 4, 4)[nrows - 1]
            if ns2 in (16, 8, 4):                                       # sb_qkv_chain_supported
                nsplit, sb_qkv = ns2, True
    chain = "sb_qkv" if sb_qkv else "sb" if sb_chain else "split_fused" if split_fused else "fused" if fuse_out and nsplit == 1 else "unfused"
    return chain, nsplit


# the switched chains (tests/test_gpu_kernel_dec_attn_switches.py): environment of a line -> {rows: (chain, context splits)}, pinned by
# hand in tests/test_kernel_refs.py; `fields`: what vx_dev_switches must report for the line (the other fields keep their defaults)
DEC_SWITCH_DEFAULTS = dict(sb_fuse=1, sb_qkv_rows=4, sb_qkv_nsplit=0, qkv_bal=1, fuse_out=1, fuse_split=1, att_nsplit_force=0, balance_rows=1,
                           nar_trim=1, graph_multi=1, gemm_mode=0, attn_x3=1, attn_h2=1)
DEC_SWITCH_LINES = {
    "sb_qkv_0": dict(env={"VX_SB_QKV": "0"}, fields=dict(sb_qkv_rows=0), rows=(1, 2, 3, 4)),
    "sb_qkv_2": dict(env={"VX_SB_QKV": "2"}, fields=dict(sb_qkv_rows=2), rows=(2, 3)),
    "sb_qkv_nsplit_4": dict(env={"VX_SB_QKV_NSPLIT": "4"}, fields=dict(sb_qkv_nsplit=4), rows=(1, 2)),
    "sb_qkv_nsplit_8": dict(env={"VX_SB_QKV_NSPLIT": "8"}, fields=dict(sb_qkv_nsplit=8), rows=(1, 2)),
    "sb_qkv_nsplit_16": dict(env={"VX_SB_QKV_NSPLIT": "16"}, fields=dict(sb_qkv_nsplit=16), rows=(1, 2)),
    "sb_qkv_nsplit_5": dict(env={"VX_SB_QKV_NSPLIT": "5"}, fields=dict(sb_qkv_nsplit=5), rows=(1,)),
    "sb_fuse_0": dict(env={"VX_SB_FUSE": "0"}, fields=dict(sb_fuse=0), rows=(1, 2, 3, 4)),
    "fuse_out_0": dict(env={"VX_FUSE_OUT": "0"}, fields=dict(fuse_out=0), rows=(8, 9, 16, 17, 32)),
    "fuse_split_0": dict(env={"VX_FUSE_SPLIT": "0"}, fields=dict(fuse_split=0), rows=(8, 11), geometry_only=(17,)),
    "att_nsplit_1": dict(env={"VX_ATT_NSPLIT": "1"}, fields=dict(att_nsplit_force=1), rows=(5, 8)),
    "att_nsplit_2": dict(env={"VX_ATT_NSPLIT": "2"}, fields=dict(att_nsplit_force=2), rows=(5, 7, 17, 32)),
    "att_nsplit_4": dict(env={"VX_ATT_NSPLIT": "4"}, fields=dict(att_nsplit_force=4), rows=(5, 7, 17, 32)),
    "att_nsplit_8": dict(env={"VX_ATT_NSPLIT": "8"}, fields=dict(att_nsplit_force=8), rows=(8, 32)),
    "att_nsplit_16": dict(env={"VX_ATT_NSPLIT": "16"}, fields=dict(att_nsplit_force=16), rows=(8, 32)),
    "att_nsplit_3_fuse_split_0": dict(env={"VX_ATT_NSPLIT": "3", "VX_FUSE_SPLIT": "0"}, fields=dict(att_nsplit_force=3, fuse_split=0), rows=(9,)),
}
_GEOM_ARGS = ("sb_fuse", "sb_qkv_rows", "sb_qkv_nsplit", "fuse_out", "fuse_split", "att_nsplit_force")


def dec_switch_geometry(line, nrows, identity=True):
    """(chain, context splits) of a line of DEC_SWITCH_LINES at a row count, by the restated rule"""
    f = DEC_SWITCH_LINES[line]["fields"]
    return dec_geometry(nrows, identity, **{k: v for k, v in f.items() if k in _GEOM_ARGS})


def dec_switch_launches(nrows):
    """[(contexts, finished row or None)] of the launches a switched chain is tested with: the launches of dec_launch_contexts, each with
    ONE finished row (active 0) from 3 rows up -- row (3 j + 1) mod nrows of launch j below 8 rows; from 8 rows up, where launch slots y
    and y + ceil(nrows / 2) share a workgroup on the fused chains, a row of the first half in even launches and of the second half in
    odd ones --, then launches in which every row is live that hold the contexts the finished rows had (filled up from DEC_CTX in order),
    so that every context of DEC_CTX still meets every split count in a live row"""
    base = dec_launch_contexts(nrows)
    if nrows < 3:
        return [(c, None) for c in base]
    gy = (nrows + 1) // 2
    fin = (lambda j: (3 * j + 1) % nrows) if nrows < 8 else (lambda j: gy + j % (nrows - gy) if j % 2 else (j + 1) % gy)
    out = [(c, fin(j)) for j, c in enumerate(base)]
    lost = [c[f] for c, f in out]
    lost += [c for c in DEC_CTX if c not in lost]
    nmore = -(-len(out) // nrows)
    for j in range(nmore):
        out.append(([lost[(j * nrows + i) % len(lost)] for i in range(nrows)], None))
    return out


def dec_split_bounds(npast, nsplit):
    """[t0, t1) of every context split over the npast cached rows: chunk = (ceil(npast / nsplit) + 15) & ~15 (decode.hip)"""
    chunk = ((npast + nsplit - 1) // nsplit + 15) & ~15
    return [(min(s * chunk, npast), min(s * chunk + chunk, npast)) for s in range(nsplit)]


def dec_launch_contexts(nrows):
    """the context lengths of the launches one row count is tested with: every context of DEC_CTX appears; from 8 rows up (two rows
    per workgroup, launch slots y and y + ceil(nrows / 2)) the pairs hold long + short, short + long and, for an even row count, one
    pair of equal contexts"""
    n12 = len(DEC_CTX)
    if nrows < 8:
        return [[DEC_CTX[(j * nrows + i) % n12] for i in range(nrows)] for j in range(-(-n12 // nrows))]
    gy = (nrows + 1) // 2
    out = []
    for j in range(-(-n12 // gy)):
        c = [DEC_CTX[(j * gy + i) % n12] for i in range(gy)] + [DEC_CTX[(j * gy + i + 1) % n12] for i in range(nrows - gy)]
        if nrows % 2 == 0:
            c[nrows - 1] = c[gy - 1]
        out.append(c)
    return out


def balance_order(ctx):
    """the engine's launch order (engine.hip ar_prefill): rows by context, the longest ceil(n / 2) first (descending, stable), then
    the rest ascending; order[y] = the row in launch slot y"""
    n = len(ctx)
    by_len = sorted(range(n), key=lambda i: -int(ctx[i]))
    first = (n + 1) // 2
    return np.array(by_len[:first] + [by_len[n - 1 - (y - first)] for y in range(first, n)], np.int32)


def dec_layer0_weights(sd):
    p = "ar_decoder.layers.0."
    return dict(in_w=sd[p + "self_attn.in_proj_weight"], in_b=sd[p + "self_attn.in_proj_bias"], out_w=sd[p + "self_attn.out_proj.weight"],
                out_b=sd[p + "self_attn.out_proj.bias"], n1_w=sd[p + "norm1.weight"], n1_b=sd[p + "norm1.bias"], l2_b=sd[p + "linear2.bias"])


def _stale(tmax=DEC_TMAX):
    """what a reused arena slot holds behind a shorter request: finite values of order 1e4, both signs"""
    if tmax not in _STALE:
        rng = np.random.default_rng(77)
        _STALE[tmax] = tuple((rng.uniform(0.5, 1.5, (16, tmax, 64)) * 1.0e4 * rng.choice([-1.0, 1.0], (16, tmax, 64))).astype(np.float32)
                             for _ in range(2))
    return _STALE[tmax]


_STALE = {}


def dec_case(kind, ctx, w, chain, seed, skp=0, balanced=False, stale=True, tmax=DEC_TMAX):
    """operands of one launch for vx_dev_dec_attn (keyword arguments of Engine.dev_dec_attn, + `kind`, `chain`).
    dec_attn chains: the q | k_new | v_new rows are chosen, then split into in_proj slabs (4, or 8 + 4 + 4 `balanced`);
    sb_qkv chain: x (skp 0) or eight linear2 slabs + the residual row (skp 8) are chosen, q / k_new / v_new follow from in_proj; there
    'uniform' is a uniform x in [-2, 2) and 'model' a normal x with per-channel gains from {0.1, 1, 4} (the sets below describe the
    cached K / V of that chain, and q | k_new | v_new of the others).
      uniform    uniform [-1, 1), q x 4          model      normal q, k; v normal with per-channel gains from {0.01, 1, 30}
      sharp      scores spread over a few hundred (q, k x 10; sb_qkv: cached keys x 300): the running-max rescale matters
      new_heavy  the new token's score ~ 16 above the cached keys' (almost all of the mass), new_light: ~ 16 below (almost none)"""
    rng = np.random.default_rng(seed)
    n = len(ctx)
    sb = chain == "sb_qkv"
    case = dict(ctx_len=np.array(ctx, np.int32), tmax=tmax, kind=kind, chain=chain, skp=skp, qkv_balanced=balanced)
    if sb:
        # the chosen row: uniform [-2, 2) for 'uniform', normal with per-channel gains from {0.1, 1, 4} for 'model', normal otherwise
        row = rng.uniform(-2.0, 2.0, (n, 1024)) if kind == "uniform" else rng.normal(0.0, 1.0, (n, 1024))
        if kind == "model":
            row = row * rng.choice([0.1, 1.0, 4.0], 1024)
        if skp:                              # ... is the residual row; the eight linear2 slabs follow its distribution at 0.4 x
            slabs = rng.uniform(-0.8, 0.8, (8, n, 1024)) if kind == "uniform" else rng.normal(0.0, 0.4, (8, n, 1024))
            x_in = np.concatenate([slabs, row[None]]).astype(np.float32)
            x = layer_norm_ref(x_in.astype(np.float64).sum(0) + w["l2_b"].astype(np.float64), w["n1_w"], w["n1_b"])
        else:
            x_in = row.astype(np.float32)
            x = x_in.astype(np.float64)
        case["x_in"] = x_in
        q = (x @ w["in_w"][:1024].astype(np.float64).T + w["in_b"][:1024]).reshape(n, 16, 64)
    else:
        if kind == "uniform":
            t = rng.uniform(-1.0, 1.0, (n, 3072))
            t[:, :1024] *= 4.0
        else:
            t = rng.normal(0.0, 1.0, (n, 3072))
        if kind == "model":
            t[:, 2048:] *= rng.choice([0.01, 1.0, 30.0], 1024)
        if kind == "sharp":
            t[:, :2048] *= 10.0
        q = t[:, :1024].reshape(n, 16, 64)
        if kind in ("new_heavy", "new_light"):
            t[:, 1024:2048] = (2.0 if kind == "new_heavy" else -2.0) * t[:, :1024]      # q . k_new / 8 = +-|q|^2 / 4 ~ +-16
        pre = t - w["in_b"].astype(np.float64)
        slabs = rng.normal(0.0, 0.5, (4, n, 3072)) * np.abs(pre).mean()
        slabs[3] = pre - slabs[:3].sum(0)
        slabs = slabs.astype(np.float32)
        if balanced:                          # q: every slab in two exact halves (eight slabs, the same sums); k, v: the same four
            b8 = np.zeros((8, n, 3072), np.float32)
            b8[:4] = slabs
            b8[:, :, :1024] = np.repeat(slabs[:, :, :1024] * np.float32(0.5), 2, axis=0)
            slabs = b8
        case["qkv"] = slabs
        case["resid"] = rng.normal(0.0, 1.0, (n, 1024)).astype(np.float32)
    k_rows, v_rows = [], []
    for r in range(n):
        p = int(ctx[r]) - 1
        if kind == "uniform":
            k, v = rng.uniform(-1.0, 1.0, (p, 16, 64)), rng.uniform(-1.0, 1.0, (p, 16, 64))
        else:
            k, v = rng.normal(0.0, 1.0, (p, 16, 64)), rng.normal(0.0, 1.0, (p, 16, 64))
        if kind == "model":
            v = v * rng.choice([0.01, 1.0, 30.0], (16, 64))
        if kind == "sharp":
            k = k * (300.0 if sb else 10.0)
        if kind in ("new_heavy", "new_light") and sb:          # k_new follows from x here: move the cached keys' scores instead
            qq = q[r] / (q[r] ** 2).sum(-1, keepdims=True)
            k = 0.1 * k + (-128.0 if kind == "new_heavy" else 128.0) * qq[None]
        k_rows.append(k.astype(np.float32))
        v_rows.append(v.astype(np.float32))
    case["k_rows"], case["v_rows"] = k_rows, v_rows
    if stale:
        sk, sv = _stale(tmax)
        case["k_fill"] = [sk[:, int(c) - 1:] for c in ctx]
        case["v_fill"] = [sv[:, int(c) - 1:] for c in ctx]
    return case


def dec_attn_block_ref(case, w, nsplit):
    """float64 reference of the block on the fp32 operands of `case`: q / k_new / v_new = sum of the slabs + bias (sb_qkv: norm1 and
    in_proj in front), softmax(q K^T / 8) over the cached rows plus the new token, out_proj.  Returns a dict of float64 arrays: qkv
    (n, 3072), attn (n, 1024), proj = W_o attn (n, 1024), h = resid + out_b + proj (dec_attn chains), and per (row, head, split)
    m (the split's largest score) and l = sum exp(score - m) over dec_split_bounds -- the last split of a dec_attn chain holds the new
    token too, the sb_qkv chain keeps it apart; empty splits: (-1e30, 0)."""
    f8 = np.float64
    ctx = case["ctx_len"]
    n = len(ctx)
    sb = case["chain"] == "sb_qkv"
    if sb:
        xi = case["x_in"].astype(f8)
        x = layer_norm_ref(xi.sum(0) + w["l2_b"].astype(f8), w["n1_w"], w["n1_b"]) if case["skp"] else xi
        qkv = x @ w["in_w"].astype(f8).T + w["in_b"].astype(f8)
    else:
        s = case["qkv"].astype(f8)
        qkv = np.concatenate([s[:, :, :1024].sum(0), s[:4, :, 1024:].sum(0)], -1) + w["in_b"].astype(f8)
    attn = np.zeros((n, 1024))
    m = np.full((n, 16, nsplit), -1.0e30)
    l = np.zeros((n, 16, nsplit))
    for r in range(n):
        q, kn, vn = (qkv[r, i * 1024:(i + 1) * 1024].reshape(16, 64) for i in range(3))
        K = np.concatenate([case["k_rows"][r].astype(f8).transpose(1, 0, 2), kn[:, None]], 1)         # (16, ctx, 64)
        V = np.concatenate([case["v_rows"][r].astype(f8).transpose(1, 0, 2), vn[:, None]], 1)
        sc = np.einsum("hd,htd->ht", q, K) / 8.0
        e = np.exp(sc - sc.max(-1, keepdims=True))
        attn[r] = np.einsum("ht,htd->hd", e / e.sum(-1, keepdims=True), V).reshape(1024)
        npast = int(ctx[r]) - 1
        for si, (t0, t1) in enumerate(dec_split_bounds(npast, nsplit)):
            part = sc[:, t0:t1]
            if si == nsplit - 1 and not sb:
                part = np.concatenate([part, sc[:, npast:]], 1)
            if part.shape[1]:
                m[r, :, si] = part.max(-1)
                l[r, :, si] = np.exp(part - part.max(-1, keepdims=True)).sum(-1)
    proj = attn @ w["out_w"].astype(f8).T
    out = dict(qkv=qkv, attn=attn, proj=proj, m=m, l=l)
    if not sb:
        out["h"] = case["resid"].astype(f8) + w["out_b"].astype(f8) + proj
    return out


def dec_attn_block_fp32(case, w, nsplit):
    """the yardstick: the same block in torch-CPU fp32 on the same fp32 operands, in the reference's formulation (F.layer_norm,
    F.linear, F.softmax and matmuls; modules/activation.py:142-167) -- the same keys as dec_attn_block_ref"""
    import torch
    import torch.nn.functional as F
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    ctx = case["ctx_len"]
    n = len(ctx)
    sb = case["chain"] == "sb_qkv"
    if sb:
        xi = T(case["x_in"])
        x = F.layer_norm(xi.sum(0) + T(w["l2_b"]), (1024,), T(w["n1_w"]), T(w["n1_b"]), 1e-5) if case["skp"] else xi
        qkv = F.linear(x, T(w["in_w"]), T(w["in_b"]))
    else:
        s = T(case["qkv"])
        qkv = torch.cat([s[:, :, :1024].sum(0), s[:4, :, 1024:].sum(0)], -1) + T(w["in_b"])
    attn = torch.zeros(n, 1024)
    m = torch.full((n, 16, nsplit), -1.0e30)
    l = torch.zeros(n, 16, nsplit)
    for r in range(n):
        q, kn, vn = (qkv[r, i * 1024:(i + 1) * 1024].reshape(16, 1, 64) for i in range(3))
        K = torch.cat([T(case["k_rows"][r]).transpose(0, 1), kn], 1)
        V = torch.cat([T(case["v_rows"][r]).transpose(0, 1), vn], 1)
        sc = (q @ K.transpose(-2, -1)) * 0.125                                                        # (16, 1, ctx)
        attn[r] = (F.softmax(sc, dim=-1) @ V).reshape(1024)
        sc = sc[:, 0]
        npast = int(ctx[r]) - 1
        for si, (t0, t1) in enumerate(dec_split_bounds(npast, nsplit)):
            part = sc[:, t0:t1]
            if si == nsplit - 1 and not sb:
                part = torch.cat([part, sc[:, npast:]], 1)
            if part.shape[1]:
                m[r, :, si] = part.max(-1).values
                l[r, :, si] = torch.exp(part - part.max(-1, keepdim=True).values).sum(-1)
    proj = F.linear(attn, T(w["out_w"]))
    out = dict(qkv=qkv.numpy(), attn=attn.numpy(), proj=proj.numpy(), m=m.numpy(), l=l.numpy())
    if not sb:
        out["h"] = (T(case["resid"]) + F.linear(attn, T(w["out_w"]), T(w["out_b"]))).numpy()
    return out


def dec_append_expected(case, w):
    """K[ctx - 1], V[ctx - 1] of every row as dec_attn_kernel appends them: the fp32 slab sum ((p0 + p1) + p2) + p3, then + bias (k and
    v have four slabs in both layouts); (n, 16, 64) each"""
    s = case["qkv"][:4]
    t = s[0].copy()
    for ks in range(1, 4):
        t = (t + s[ks]).astype(np.float32)
    t = (t + w["in_b"].astype(np.float32)).astype(np.float32)
    n = t.shape[0]
    return t[:, 1024:2048].reshape(n, 16, 64), t[:, 2048:].reshape(n, 16, 64)


# ---- the GEMM / FFN / LayerNorm half of one decode step (vx_dev_dec_op; csrc/decode.hip) -------------------------------------------
# weight -> (N, padded N, K, K slices) of the engine (engine_ctx.h: SK_QKV, SK_OUT, SK_L2, SK_PRED, PRED_NPAD)
FFN_GEMMS = {"in_proj": (3072, 3072, 1024, 4), "out_proj": (1024, 1024, 1024, 4), "linear2": (1024, 1024, 4096, 8), "predict": (1025, 1056, 1024, 4)}
FFN_ROWS = (5, 7, 16, 17, 32)             # the general kernels
FFN_SB_ROWS = (1, 2, 3, 4)                # the small-batch consumers
FFN_GEMM_SETS = ("normal", "model", "cancel")
FFN_LN_SETS = ("normal", "mean1e3", "const", "mag1e4", "slabs1e4")
FFN_FILL = np.float32(-1.0e30)            # what image / slab rows behind the last row hold: the entry's sentinel


def ffn_weights(sd, nl):
    """the AR decoder's weights of a synth state dict: w[layer][name], w['norm'], w['pred'], w['emb'], w['alpha']"""
    w = {}
    for l in range(nl):
        p = f"ar_decoder.layers.{l}."
        w[l] = dict(in_proj=sd[p + "self_attn.in_proj_weight"], in_b=sd[p + "self_attn.in_proj_bias"], out_proj=sd[p + "self_attn.out_proj.weight"],
                    out_b=sd[p + "self_attn.out_proj.bias"], linear1=sd[p + "linear1.weight"], l1_b=sd[p + "linear1.bias"],
                    linear2=sd[p + "linear2.weight"], l2_b=sd[p + "linear2.bias"], n1=(sd[p + "norm1.weight"], sd[p + "norm1.bias"]),
                    n2=(sd[p + "norm2.weight"], sd[p + "norm2.bias"]))
    w["norm"] = (sd["ar_decoder.norm.weight"], sd["ar_decoder.norm.bias"])
    w["pred"] = sd["ar_predict_layer.weight"]
    w["emb"] = sd["ar_audio_embedding.word_embeddings.weight"]
    w["alpha"] = np.float32(sd["ar_audio_position.alpha"][0])
    w["nl"] = nl
    return w


def ffn_weight(w, name, layer):
    return w["pred"] if name == "predict" else w[layer][name]


def linear_ref(x, wt, bias=None, relu=False):
    """x W^T (+ bias) (ReLU) in float64 on the fp32 operands"""
    y = np.asarray(x, np.float64) @ np.asarray(wt, np.float64).T
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    return np.maximum(y, 0.0) if relu else y


def linear_fp32(x, wt, bias=None, relu=False):
    """the yardstick: torch-CPU fp32 F.linear (F.relu)"""
    import torch
    import torch.nn.functional as F
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32))
    y = F.linear(T(x), T(wt), T(bias))
    return (F.relu(y) if relu else y).numpy()


def reduce_ln_ref(slabs, bias, resid, norm):
    """(h, LayerNorm(h)) in float64: h = resid + sum of the slabs + bias; slabs (SK, n, 1024) or None, bias or None"""
    h = np.asarray(resid, np.float64)
    if slabs is not None and len(slabs):
        h = h + np.asarray(slabs, np.float64).sum(0)
    if bias is not None:
        h = h + np.asarray(bias, np.float64)
    return h, layer_norm_ref(h, norm[0], norm[1])


def reduce_ln_fp32(slabs, bias, resid, norm):
    """the yardstick: the same in torch-CPU fp32 (sum over the slab axis, F.layer_norm)"""
    import torch
    import torch.nn.functional as F
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    h = T(resid)
    if slabs is not None and len(slabs):
        s = T(slabs).sum(0)
        h = h + (s + T(bias) if bias is not None else s)
    return h.numpy(), F.layer_norm(h, (1024,), T(norm[0]), T(norm[1]), 1e-5).numpy()


def reduce_h_exact(slabs, bias, resid):
    """h as the reduce kernels form it in fp32: resid + ((((p0 + p1) + ...) + p_last) + bias)"""
    v = np.array(slabs[0], np.float32)
    for ks in range(1, len(slabs)):
        v = (v + np.asarray(slabs[ks], np.float32)).astype(np.float32)
    if bias is not None:
        v = (v + np.asarray(bias, np.float32)).astype(np.float32)
    return (np.asarray(resid, np.float32) + v).astype(np.float32)


def embed_exact(emb, alpha, pe, tok, pos):
    """fp32(emb[tok] + fp32(alpha * pe[pos])): two roundings, what torch computes for emb + alpha * pe (modules/embedding.py:93-97)"""
    return (emb[tok] + (np.float32(alpha) * pe[pos]).astype(np.float32)).astype(np.float32)


def embed_ref(emb, alpha, pe, tok, pos):
    return emb[tok].astype(np.float64) + np.float64(alpha) * pe[pos].astype(np.float64)


# identity probes: every kernel as a reader of its own weight image
def probe_plan(K):
    """the K / 32 launches that walk every k once: row b of launch j holds 2^(b % 5 - 2) at column b * (K / 32) + j and zeros elsewhere, so
    the 32 k's of one launch spread over every K slice and every wave of a slice"""
    return [np.arange(32) * (K // 32) + j for j in range(K // 32)]


def probe_scale():
    return np.ldexp(np.float32(1.0), np.arange(32) % 5 - 2).astype(np.float32)


def probe_image(ks, K, nrows=32):
    """the un-packed x image of one probe launch; rows nrows .. 31 hold the sentinel"""
    x = np.zeros((32, K), np.float32)
    x[np.arange(32), ks] = probe_scale()
    x[nrows:] = FFN_FILL
    return x


def slab_of(n, k, K, sk):
    """the slab of skinny_gemm_kernel that owns k (every column alike): k // (K / sk)"""
    return np.asarray(k) // (K // sk) + 0 * np.asarray(n)


def slab_of_balanced(n, k):
    """skinny_qkv_bal_kernel: the q columns (n < 1024) are cut into eight K slices of 128, the k and v columns into four of 256"""
    n, k = np.asarray(n), np.asarray(k)
    return np.where(n < 1024, k // 128, k // 256)


def probe_expected(wt, ks, npad, sk, balanced=False):
    """what a GEMM probe launch must leave: (sk, 32, npad) fp32; the balanced layout's unwritten k, v columns of slabs 4 .. 7 hold
    the sentinel, padding columns hold 0"""
    N, K = wt.shape
    exp = np.zeros((sk, 32, npad), np.float32)
    if balanced:
        exp[4:, :, 1024:] = FFN_FILL
    sc = probe_scale()
    cols = np.arange(N)
    for b, k in enumerate(ks):
        s = slab_of_balanced(cols, k) if balanced else slab_of(cols, k, K, sk)
        exp[s, b, cols] = wt[:, k] * sc[b]
    return exp


def probe_expected_linear1(wt, bias, ks):
    """max(fp32(fp32(W[n][k] 2^e) + b1[n]), 0) of every row: (32, 4096)"""
    sc = probe_scale()
    return np.maximum((wt[:, ks].T * sc[:, None]).astype(np.float32) + bias[None].astype(np.float32), np.float32(0.0)).astype(np.float32)


# operand sets
def cancel_columns(name):
    """the output columns the 'cancel' set cancels on: x lies in the null space of these rows of W.  Fewer than K of them (a fixed
    weight with N >= K rows has no x that cancels on every column: the smallest singular value of a 3072 x 1024 matrix bounds
    |W x| / |x| from below), spread over every column tile"""
    N, _, K, _ = FFN_GEMMS.get(name, (4096, 4096, 1024, 1))
    return np.arange(0, N, max(1, -(-2 * N // K)))


def gemm_operands(kind, wt, name, nrows, seed):
    """x (32, K) fp32 of a GEMM set; rows nrows .. 31 hold the sentinel.  normal: unit normal; model: normal with per-channel gains from
    {0.1, 1, 4}; cancel: a unit normal projected onto the null space of the rows cancel_columns(name) of W (float64, then rounded)"""
    rng = np.random.default_rng(seed)
    K = wt.shape[1]
    x = rng.normal(0.0, 1.0, (32, K))
    if kind == "model":
        x = x * rng.choice([0.1, 1.0, 4.0], K)
    elif kind == "cancel":
        ws = wt[cancel_columns(name)].astype(np.float64)
        x = x - np.linalg.solve(ws @ ws.T, ws @ x.T).T @ ws
    elif kind != "normal":
        raise ValueError(kind)
    x = x.astype(np.float32)
    x[nrows:] = FFN_FILL
    return x


def cancellation(x, wt, cols):
    """max over the rows and the columns `cols` of |x . w_n| / sum_k |x_k w_nk| in float64"""
    x, ws = np.asarray(x, np.float64), np.asarray(wt, np.float64)[cols]
    return float((np.abs(x @ ws.T) / (np.abs(x) @ np.abs(ws).T)).max())


def ln_operands(kind, sk, bias, nrows, seed):
    """launches [(slabs (sk, 32, 1024) fp32, resid (nrows, 1024) fp32)] of a LayerNorm set; h = resid + sum of the slabs + bias.
      normal    resid unit normal, slabs normal / sqrt(sk)        mean1e3   h = 1e3 + a spread of 1 (a one-pass variance is wrong)
      const     h exactly constant (the first slab holds -bias: variance 0, rstd = eps^-1/2) in the first launch; the fp32 yardstick is
                exact there, so further launches hold constants with a spread of 1e-4 (variance far below eps) for the ratio
      mag1e4    h of magnitude 1e4                               slabs1e4  slabs of +-1e4 that cancel to order 1 (sk >= 2)
    slab rows nrows .. 31 hold the sentinel"""
    rng = np.random.default_rng(seed)
    zb = np.zeros(1024, np.float32) if bias is None else np.asarray(bias, np.float32)

    def done(slabs, resid):
        slabs = np.asarray(slabs, np.float32).reshape(sk, 32, 1024)
        slabs[:, nrows:] = FFN_FILL
        return slabs, np.asarray(resid, np.float32)[:nrows].copy()

    slabs = rng.normal(0.0, 1.0 / np.sqrt(max(sk, 1)), (sk, 32, 1024))
    resid = rng.normal(0.0, 1.0, (32, 1024))
    if kind == "normal":
        return [done(slabs, resid)]
    if kind == "mean1e3":
        return [done(0.1 * slabs, 1.0e3 + resid)]
    if kind == "mag1e4":
        return [done(slabs, 1.0e4 * resid)]
    if kind == "slabs1e4":
        if sk < 2:
            raise ValueError("no slabs to cancel")
        big = rng.uniform(0.5, 1.5, (sk // 2, 32, 1024)) * 1.0e4 * rng.choice([-1.0, 1.0], (sk // 2, 32, 1024))
        s = slabs.astype(np.float32)
        s[0::2] = big.astype(np.float32)
        s[1::2] = (slabs[1::2] - big).astype(np.float32)
        return [done(s, resid)]
    if kind == "const":
        s = np.zeros((sk, 32, 1024), np.float32)
        if sk:
            s[0] = -zb
        c = np.array([3.0, 1.1, -2.7, 10.3, 0.1, -7.3, 1.0e-3, 20.0], np.float32)[np.arange(32) % 8]
        out = [done(s.copy(), np.repeat(c[:, None], 1024, 1))]
        # next to a constant c the LayerNorm result moves by rstd = 316 for every unit of (x - mean), and (x - mean) comes in units of
        # ulp(c): a row's error is its mean's last bit, in the kernel and in the yardstick alike, so one row says nothing -- at least 16
        # rows go into the pool, each a constant of 0.1 .. 3 plus a spread of 1e-4 (hundreds of ulps; variance 1e-8, 0.1 % of eps)
        for _ in range(-(-16 // nrows)):
            cr = rng.uniform(0.1, 3.0, (32, 1)) * rng.choice([-1.0, 1.0], (32, 1))
            out.append(done(s.copy(), cr + 1.0e-4 * rng.normal(0.0, 1.0, (32, 1024))))
        return out
    raise ValueError(kind)


FFN_OPS = ("gemm:in_proj", "gemm:out_proj", "gemm:linear2", "gemm:predict", "qkv_bal", "linear1", "reduce_ln:0", "reduce_ln:4", "reduce_ln:8",
           "reduce_ln:16")
FFN_SB_OPS = ("sb_ln_gemm:in_proj", "sb_ln_gemm:predict", "sb_linear1")
_FFN_CASES = {}


def ffn_sets(op):
    if op.startswith(("gemm", "qkv_bal", "linear1")):
        return FFN_GEMM_SETS
    return tuple(k for k in FFN_LN_SETS if not (op == "reduce_ln:0" and k == "slabs1e4"))


def ffn_layer(op, nrows, nl=2):
    """the layer a case runs on: alternating with the row count, except where the op fixes it"""
    if op.startswith("sb_ln_gemm"):
        return nl - 1
    return nrows % nl


def ffn_reduce_params(w, layer, sk):
    """(bias, norm) of a reduce + LayerNorm launch as the engine pairs them (engine.hip ar_step_launches)"""
    if sk == 0:
        return None, w["norm"]
    if sk == 8:
        return w[layer]["l2_b"], (w[layer + 1]["n1"] if layer + 1 < w["nl"] else w["norm"])
    return w[layer]["out_b"], w[layer]["n2"]


def ffn_case(op, nrows, kind, w):
    """launches of one (op, row count, operand set): [dict(args = keyword arguments of Engine.dev_dec_op, ref, yard = {quantity: rows
    < nrows})] with the float64 reference and the torch-CPU fp32 yardstick on the fp32 operands.  Quantities: 'sum' (the slab sum of a
    GEMM, no bias), 'act' (linear1's ReLU output), 'xp' (the LayerNorm output)."""
    import zlib
    key = (op, nrows, kind)
    if key in _FFN_CASES:
        return _FFN_CASES[key]
    seed = zlib.crc32(repr(key).encode())
    name, _, arg = op.partition(":")
    layer = ffn_layer(op, nrows, w["nl"])
    out = []
    if name in ("gemm", "qkv_bal", "linear1"):
        wname = arg if name == "gemm" else "in_proj" if name == "qkv_bal" else "linear1"
        wt = ffn_weight(w, wname, layer)
        x = gemm_operands(kind, wt, wname, nrows, seed)
        args = dict(op=name, nrows=nrows, layer=layer, x=x)
        if name == "gemm":
            args["weight"] = arg
        bias, relu, q = (w[layer]["l1_b"], True, "act") if name == "linear1" else (None, False, "sum")
        out.append(dict(args=args, ref={q: linear_ref(x[:nrows], wt, bias, relu)}, yard={q: linear_fp32(x[:nrows], wt, bias, relu)}))
    else:
        sk = int(arg) if name == "reduce_ln" else 8 if name == "sb_ln_gemm" else 4
        # the small-batch consumers: REDUCE_LN 8 of the layer below in front of in_proj, of the last layer in front of predict; REDUCE_LN 4
        rl = layer - 1 if op == "sb_ln_gemm:in_proj" else layer
        bias, norm = ffn_reduce_params(w, rl, sk)
        for slabs, resid in ln_operands(kind, sk, bias, nrows, seed):
            args = dict(op=name, nrows=nrows, layer=layer, slabs=slabs if sk else None, resid=resid)
            sl = slabs[:, :nrows] if sk else None
            (_, xr), (_, xy) = reduce_ln_ref(sl, bias, resid, norm), reduce_ln_fp32(sl, bias, resid, norm)
            if name == "reduce_ln":
                args["sk"] = sk
                ref, yard = {"xp": xr}, {"xp": xy}
            elif name == "sb_ln_gemm":
                args["weight"] = arg
                wt = ffn_weight(w, arg, layer)
                ref, yard = {"sum": linear_ref(xr, wt)}, {"sum": linear_fp32(xy, wt)}
            else:
                ref = {"act": linear_ref(xr, w[layer]["linear1"], w[layer]["l1_b"], True)}
                yard = {"act": linear_fp32(xy, w[layer]["linear1"], w[layer]["l1_b"], True)}
            out.append(dict(args=args, ref=ref, yard=yard, bias=bias, norm=norm))
    if len(_FFN_CASES) >= 64:
        _FFN_CASES.pop(next(iter(_FFN_CASES)))
    _FFN_CASES[key] = out
    return out


def ffn_chain_ref(slabs, resid, w, layer):
    """norm2 -> linear1 -> ReLU -> linear2 -> + residual -> the next norm -> predict of `layer` (the last one: the final norm) from
    the out_proj slabs and the residual rows: (float64 logits, torch-CPU fp32 logits), (n, 1025)"""
    L = w[layer]
    bias8, norm8 = ffn_reduce_params(w, layer, 8)
    res = []
    for red, lin in ((reduce_ln_ref, linear_ref), (reduce_ln_fp32, linear_fp32)):
        h, x = red(slabs, L["out_b"], resid, L["n2"])
        y = lin(lin(x, L["linear1"], L["l1_b"], True), L["linear2"])
        _, x2 = red(y[None], bias8, h, norm8)
        res.append(lin(x2, w["pred"]))
    return res[0], res[1]


# ---- the full-sequence GEMMs and layernorm_kernel (tests/test_gpu_kernel_gemm.py) ---------------------------------------------------
H2_ACT_SHIFT = 5              # activations are split at 2^5 (vx_common.h)
H2_TILE = 256                 # rows of a plane tile, both operands
H2_LIMIT = 65504.0            # |X| at or above this (or non-finite) raises the range flag
H2_SENT = np.uint16(0xFBFF)   # VX_DEV_SENTINEL_H


def h2_split_ref(x, shift):
    """(head, tail) fp16 of X = x 2^shift: head = fp16(X), tail = fp16(X - head), both round-to-nearest-even with fp16 subnormals --
    h2_split of csrc/vx_common.h"""
    X = np.asarray(x, np.float32) * np.float32(2.0 ** shift)
    with np.errstate(over="ignore", invalid="ignore"):
        h = X.astype(np.float16)
        t = (X - h.astype(np.float32)).astype(np.float16)
    return h, t


def h2_value(x, shift):
    """(head + tail) 2^-shift in float64: the operand the f16x2 kernels see"""
    h, t = h2_split_ref(x, shift)
    return (h.astype(np.float64) + t.astype(np.float64)) * 2.0 ** -shift


def h2_range_bad(x, shift):
    """what h2_split calls bad: not |X| < 65504 (so NaN and +-inf too)"""
    with np.errstate(over="ignore", invalid="ignore"):
        X = np.asarray(x, np.float32) * np.float32(2.0 ** shift)
        return bool((~(np.abs(X) < np.float32(H2_LIMIT))).any())


def h2_tile_index(r, k, K, tile_rows=H2_TILE):
    """half-word index of element (r, k) inside one tile-major plane [rows / tile][K / 32][tile][32]"""
    r, k = np.asarray(r, np.int64), np.asarray(k, np.int64)
    return (((r // tile_rows) * (K // 32) + k // 32) * tile_rows + r % tile_rows) * 32 + k % 32


def h2_weight_shift_ref(absmax):
    """the loader's rule: max |w| 2^shift in [16384, 32768), shift clamped to 0 .. 24; 24 for a zero or non-finite maximum"""
    absmax = float(np.float32(absmax))
    if not (absmax > 0.0) or not np.isfinite(absmax):
        return 24
    _, ex = np.frexp(absmax)                       # absmax = m 2^ex, 0.5 <= m < 1
    return int(min(24, max(0, 15 - int(ex))))


def h2_gemm_model(a, w, shift):
    """float64 model of the f16x2 product: (head.head + head.tail + tail.head) 2^-(5 + shift); the tail.tail term is dropped"""
    ah, at = (p.astype(np.float64) for p in h2_split_ref(a, H2_ACT_SHIFT))
    wh, wt = (p.astype(np.float64) for p in h2_split_ref(w, shift))
    return (ah @ wh.T + ah @ wt.T + at @ wh.T) * 2.0 ** -(H2_ACT_SHIFT + shift)


def h2_model_bound(a, w, shift):
    """bound of |model - a W^T| per element: with d(x) = max(2^-22 |x|, 2^-25 2^-s) the split error of an operand at shift s,
    sum_k (d(a_k) |w_k| + |a_k| d(w_k)) + 2^-22 sum_k |a_k w_k|  (the last term: the dropped tail.tail products)"""
    a, w = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(w, np.float64))
    da = np.maximum(2.0 ** -22 * a, 2.0 ** -25 * 2.0 ** -H2_ACT_SHIFT)
    dw = np.maximum(2.0 ** -22 * w, 2.0 ** -25 * 2.0 ** -shift)
    return da @ w.T + a @ dw.T + 2.0 ** -22 * (a @ w.T)


def chain_bound(a, w):
    """K 2^-24 sum_k |a_k w_k| per output element: what K fp32 additions into one accumulator can lose, each at most 2^-24 of a
    partial sum that sum_k |a_k w_k| bounds"""
    a, w = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(w, np.float64))
    return a.shape[1] * 2.0 ** -24 * (a @ w.T)


def chain_fp32(a, w):
    """a W^T as ONE k-ordered fp32 chain per element (numpy's cumsum adds in order): the summation order of the GEMM kernels"""
    a, w = np.asarray(a, np.float32), np.asarray(w, np.float32)
    return np.stack([np.cumsum(a[:, None, :] * w[None, n0:n0 + 8, :], axis=-1, dtype=np.float32)[..., -1] for n0 in range(0, len(w), 8)], 1).reshape(len(a), -1)


def _act64(y, act):
    import torch
    if act == 1:
        return np.maximum(y, 0.0)
    if act == 2:
        return 0.5 * y * (1.0 + torch.erf(torch.from_numpy(y * np.sqrt(0.5))).numpy())
    if act == 3:
        return np.where(y > 0, y, np.expm1(np.minimum(y, 0.0)))
    return y


def gemm_ref(a, w, bias=None, act=0, colscale=None, resid=None, pre=None):
    """the GemmArgs contract in float64: resid + colscale act(a W^T + bias); act 0 none, 1 ReLU, 2 GELU (erf), 3 ELU.  pre: a sum to
    use instead of a W^T (the f16x2 model)"""
    y = np.asarray(a, np.float64) @ np.asarray(w, np.float64).T if pre is None else np.asarray(pre, np.float64)
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    y = _act64(y, act)
    if colscale is not None:
        y = y * np.asarray(colscale, np.float64)
    if resid is not None:
        y = np.asarray(resid, np.float64) + y
    return y


def gemm_fp32(a, w, bias=None, act=0, colscale=None, resid=None):
    """the yardstick: the same in torch-CPU fp32 (F.linear, F.relu / F.gelu / F.elu)"""
    import torch
    import torch.nn.functional as F
    T = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.float32))
    y = F.linear(T(a), T(w), T(bias))
    y = (lambda v: v, F.relu, F.gelu, F.elu)[act](y)
    if colscale is not None:
        y = y * T(colscale)
    if resid is not None:
        y = T(resid) + y
    return y.numpy()


def ln_ref(x, g=None, b=None, aw=None, ab=None):
    """float64 (LN(x) g + b) aw + ab with eps 1e-5; any pair may be None"""
    C = np.asarray(x).shape[-1]
    y = layer_norm_ref(x, np.ones(C) if g is None else g, np.zeros(C) if b is None else b)
    if aw is not None:
        y = np.asarray(aw, np.float64) * y + np.asarray(ab, np.float64)
    return y


def ln_fp32(x, g=None, b=None, aw=None, ab=None):
    """the yardstick: torch-CPU fp32 F.layer_norm, then weight * y + bias as AdaptiveLayerNorm does"""
    import torch
    import torch.nn.functional as F
    T = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.float32))
    x = T(x)
    y = F.layer_norm(x, (x.shape[-1],), T(g), T(b), 1e-5)
    if aw is not None:
        y = T(aw) * y + T(ab)
    return y.numpy()


GEMM_SETS = ("normal", "model", "wide", "cancel")


def gemm_cancel_rows(N, K):
    """the rows of W the 'cancel' set cancels on: every r-th, fewer than K / 2 of them"""
    return np.arange(0, N, max(1, -(-2 * N // K)))


def gemm_set(kind, M, N, K, seed, wmax=None):
    """(a (M, K), w (N, K)) fp32.  w: a normal of sigma 1 / sqrt(K), scaled to max |w| = wmax when one is given.  normal: a unit normal; model: a normal with per-channel gains {0.1, 1, 4}; wide:
    |a| = e^u, u uniform in [-12, 6), |w| = e^u', u' in [-12, 0), random signs, and the first elements of row 0 of a at the upper edge
    of the f16x2 range (2046.9: X = 65500.8); cancel: a unit normal projected onto the null space of the rows gemm_cancel_rows of w"""
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 1.0, (M, K))
    w = rng.normal(0.0, 1.0 / np.sqrt(K), (N, K))
    if kind == "model":
        a = a * rng.choice([0.1, 1.0, 4.0], K)
    elif kind == "wide":
        a = np.exp(rng.uniform(-12.0, 6.0, (M, K))) * rng.choice([-1.0, 1.0], (M, K))
        w = np.exp(rng.uniform(-12.0, 0.0, (N, K))) * rng.choice([-1.0, 1.0], (N, K))
        a[0, :4] = [2046.9, -2046.9, 2046.0, 1.0e-6]
    elif kind not in ("normal", "cancel"):
        raise ValueError(kind)
    if wmax is not None:
        w = w * (wmax / np.abs(w).max())
    w = w.astype(np.float32)
    if kind == "cancel":
        ws = w[gemm_cancel_rows(N, K)].astype(np.float64)
        a = a - np.linalg.solve(ws @ ws.T, ws @ a.T).T @ ws
    return a.astype(np.float32), w


LN_SETS = ("normal", "mean1e3", "const", "mag1e4", "offset")


def ln_set(kind, rows, C, seed):
    """x (rows, C) fp32 of a LayerNorm set: normal; mean1e3 = 1e3 + a spread of 1; const = row 0 exactly constant, the other rows a
    constant of 0.1 .. 3 plus a spread of 1e-4 (variance far below eps); mag1e4 = magnitude 1e4; offset = 3e4 + a spread of 10"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (rows, C))
    if kind == "mean1e3":
        x = 1.0e3 + x
    elif kind == "mag1e4":
        x = 1.0e4 * x
    elif kind == "offset":
        x = 3.0e4 + 10.0 * x
    elif kind == "const":
        cr = rng.uniform(0.1, 3.0, (rows, 1)) * rng.choice([-1.0, 1.0], (rows, 1))
        x = cr + 1.0e-4 * x
        x[0] = 10.25                 # few mantissa bits: every partial sum of the row is exact, so mean == x and x - mean == 0
    elif kind != "normal":
        raise ValueError(kind)
    return x.astype(np.float32)


def f16x2_choice(M, N, K):
    """which instantiation launch_gemm_f16x2 picks on its own (tn = 0), restated from csrc/gemm_f16x2.hip: the cost model between
    256 x 256 and 128 x 128 tiles, then the four-wave kernel for 256 x 256 unless K is a single tile, four LDS stages for at most 256
    tiles of 128 x 128.  (The fifth instantiation, 256 x 128, is only ever forced.)"""
    mt256, mt128 = (M + 255) // 256, (M + 127) // 128
    t128 = mt128 * ((N + 127) // 128)
    rem = t128 % 512
    c128 = (t128 // 512) * 2.3 + (0.0 if rem == 0 else 1.3 if rem <= 256 else 2.3)
    c256 = ((mt256 * (N // 256) + 255) // 256) * 4.0 if N % 256 == 0 else 1e30
    if c256 < c128:
        return "w4_256x256" if K >= 64 else "w8_256x256"
    return "128x128_s4" if t128 <= 256 else "128x128_s2"
