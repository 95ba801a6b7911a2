"""References of the text-alignment tests (test infrastructure): the definition of align_rows_kernel (csrc/align.hip) in float64
numpy and in torch-CPU fp32 (the yardstick), and the pass of vx_align from the CPU oracle's taps, in float64 or fp32."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

HEADS, DH, D = 16, 64, 1024


def make_tab(seqs, q_first=None):
    """table (nseq, 6) int32 = (seq_off, seq_len, S, q_first, n_rows, out_off) of packed sequences (S, Tp, T): text, BOS ++ prompt,
    T frames -- S + Tp + T rows, the reported rows are the last T (q_first = S + Tp) unless q_first[i] says a later start.
    Returns (tab, M, sum of the reported rows)."""
    tab, off, o = [], 0, 0
    for i, (S, Tp, T) in enumerate(seqs):
        n = S + Tp + T
        qf = S + Tp if q_first is None or q_first[i] is None else int(q_first[i])
        tab.append((off, n, S, qf, n - qf, o))
        off += n
        o += n - qf
    return np.array(tab, np.int32), off, o


def align_rows_ref(qkv, tab, w):
    """float64: list, per sequence, of the (n_rows, S) array sum_h w[h] softmax_j(q_r,h . k_j,h / 8)[s], j = 0 .. r, r = q_first + t.
    A head with w[h] == 0 is left out (not multiplied by zero)."""
    qkv = np.asarray(qkv, np.float64)
    w = np.asarray(w, np.float64)
    out = []
    for off, n, S, qf, T, _ in np.asarray(tab):
        res = np.zeros((T, S))
        for h in np.flatnonzero(w):
            q = qkv[off + qf: off + qf + T, h * DH:(h + 1) * DH]
            k = qkv[off: off + n, D + h * DH: D + (h + 1) * DH]
            s = q @ k.T / 8.0
            s = np.where(np.arange(n)[None, :] <= (qf + np.arange(T))[:, None], s, -np.inf)
            e = np.exp(s - s.max(-1, keepdims=True))
            res += w[h] * (e / e.sum(-1, keepdims=True))[:, :S]
        out.append(res)
    return out


def align_rows_fp32_yardstick(qkv, tab, w):
    """the same definition in torch-CPU fp32: (q * 0.125) k^T, masked_fill, F.softmax, heads added in index order"""
    t = torch.from_numpy(np.ascontiguousarray(qkv, np.float32))
    w = np.asarray(w, np.float32)
    out = []
    for off, n, S, qf, T, _ in np.asarray(tab):
        res = torch.zeros(T, S)
        hidden = torch.arange(n)[None, :] > (qf + torch.arange(T))[:, None]
        for h in np.flatnonzero(w):
            q = t[off + qf: off + qf + T, h * DH:(h + 1) * DH] * 0.125
            k = t[off: off + n, D + h * DH: D + (h + 1) * DH]
            p = F.softmax((q @ k.T).masked_fill(hidden, float("-inf")), dim=-1)
            res = res + float(w[h]) * p[:, :S]
        out.append(res.numpy())
    return out


def uniform_weights(nl):
    return np.full((nl, HEADS), 1.0 / (HEADS * nl))


def align_ref(o, row, codes0, head_weights=None):
    """the pass of vx_align from the oracle `o` (tests/_score_refs.oracle64: float64; a plain VallexOracle: fp32, the yardstick):
    the input of AR layer i is the tap ar_prefill_in (i = 0) or ar_layer_out[i - 1]; q and k are F.linear(_ln(x, norm1), in_proj);
    the mask of ar_prefill; softmax; the text columns of rows S + Tp .. S + Tp + T - 1, summed over layers and heads with
    head_weights (None: 1 / (16 num_layers) each).  (T, S) in the oracle's precision."""
    ids = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int64)))
    text, p0, c0 = ids(row["text"]), ids(row["prompt"][:, 0]), ids(codes0).reshape(-1)
    taps = {}
    with torch.no_grad():
        o.ar_prefill(text, torch.cat([p0, c0]), row["enroll"], row["prompt_language"], row["text_language"], taps)
        S, Tp, T = len(text), len(p0), len(c0)
        L = S + 1 + Tp + T
        hw = uniform_weights(o.nl) if head_weights is None else np.asarray(head_weights, np.float64)
        mask = torch.zeros(L, L, dtype=torch.bool)
        mask[:S, S:] = True
        mask[S:, S:] = torch.triu(torch.ones(L - S, L - S, dtype=torch.bool), diagonal=1)
        dt = taps["ar_prefill_in"].dtype
        res = torch.zeros(T, S, dtype=dt)
        for i in range(o.nl):
            if not hw[i].any():
                continue
            x = taps["ar_prefill_in"] if i == 0 else taps["ar_layer_out"][i - 1]
            p = f"ar_decoder.layers.{i}."
            qkv = F.linear(o._ln(x, p + "norm1"), o.w[p + "self_attn.in_proj_weight"], o.w[p + "self_attn.in_proj_bias"])
            q, k, _ = qkv.chunk(3, dim=-1)
            q = q.view(L, HEADS, DH).transpose(0, 1)
            k = k.view(L, HEADS, DH).transpose(0, 1)
            att = F.softmax(((q @ k.transpose(-2, -1)) * 0.125).masked_fill(mask, float("-inf")), dim=-1)
            rows = att[:, S + Tp: S + Tp + T, :S]
            for h in np.flatnonzero(hw[i]):
                res = res + torch.tensor(float(hw[i, h]), dtype=dt) * rows[h]
    return res.numpy()


def align_ref64(o, row, codes0, head_weights=None):
    """align_ref on a float64 oracle (tests/_score_refs.oracle64)"""
    assert o.pe.dtype == torch.float64
    return align_ref(o, row, codes0, head_weights)


def path_of_segments(seg, T):
    """the column (0-based, relative to enroll) of every frame from the (n, 2) first / last frames of monotonic_segments"""
    path = np.full(T, -1, np.int64)
    for j, (a, b) in enumerate(np.asarray(seg)):
        path[a: b + 1] = j
    return path


def all_monotone_paths(T, n):
    """every path of T frames from column 0 to column n - 1 in steps of 0 or 1"""
    for ups in itertools.combinations(range(1, T), n - 1):
        step = np.zeros(T, np.int64)
        step[list(ups)] = 1
        yield np.cumsum(step)


def best_monotone_path(attn, enroll):
    """exhaustive search: (best score, best path); among equal scores the path whose columns are smaller compared from the LAST frame
    backwards (the rule of monotonic_segments)"""
    a = np.log(np.maximum(np.asarray(attn, np.float64)[:, enroll:], 1e-30))
    T, n = a.shape
    best = None
    for p in all_monotone_paths(T, n):
        sc = float(a[np.arange(T), p].sum())
        key = (-sc, tuple(p[::-1]))
        if best is None or key < best[0]:
            best = (key, sc, p)
    return best[1], best[2]
