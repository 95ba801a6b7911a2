"""References of the teacher-forced scoring tests (test infrastructure): the CPU oracle driven with GIVEN codes, in fp32 or float64,
and the float64 (log-probability, rank) of a target in a logit row with the error bound of the fp32 kernel that computes it."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import synth
from oracle.vallex_oracle import VallexOracle


def oracle64(sd, nl):
    """a VallexOracle whose weights and position table are float64: its methods run unchanged, in float64"""
    o = VallexOracle(sd, nl)
    o.w = {k: v.double() for k, v in o.w.items()}
    o.pe = o.pe.double()
    return o


def _ids(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int64)))


def ar_logits_tf(o, row, codes0):
    """AR logits of the T + 1 rows that predict frame 0 .. T-1 and the stop decision, from ONE full-sequence pass over
    text, BOS ++ prompt codebook 0 ++ codes0 under the prefill's prefix-LM mask: (T + 1, 1025)"""
    text, p0, c0 = _ids(row["text"]), _ids(row["prompt"][:, 0]), _ids(codes0).reshape(-1)
    taps = {}
    o.ar_prefill(text, torch.cat([p0, c0]), row["enroll"], row["prompt_language"], row["text_language"], taps)
    S, Tp, T = len(text), len(p0), len(c0)
    return o.ar_logits(taps["ar_prefill_out"][S + Tp: S + Tp + T + 1])


def ar_logits_stepwise(o, row, codes0):
    """the same rows from the cached chain: ar_prefill, then T x (ar_logits, ar_step)"""
    text, p0 = _ids(row["text"]), _ids(row["prompt"][:, 0])
    h, kv, _ = o.ar_prefill(text, p0, row["enroll"], row["prompt_language"], row["text_language"])
    Tp, out = len(p0), []
    for t, tok in enumerate(np.asarray(codes0).reshape(-1)):
        out.append(o.ar_logits(h))
        h, kv = o.ar_step(int(tok), Tp + 1 + t, kv)
    out.append(o.ar_logits(h))
    return torch.stack(out)


def nar_logits_tf(o, row, codes):
    """the loop of VallexOracle.nar_generate with the GIVEN codes (T, 8) accumulated behind every stage instead of the arg-max:
    list of 7 logit arrays (T, 1024); stage i predicts codes[:, i + 1] given codes[:, : i + 1]"""
    text, prompts, cd = _ids(row["text"]), _ids(row["prompt"]), _ids(codes).reshape(-1, 8)
    Tp, T = prompts.shape[0], cd.shape[0]
    emb = [o.w[f"nar_audio_embeddings.{j}.word_embeddings.weight"] for j in range(synth.NUM_QUANTIZERS)]
    y_emb = emb[0][torch.cat([prompts[:, 0], cd[:, 0]])].clone()
    x = o._text_embed("nar", text, row["enroll"], row["prompt_language"], row["text_language"])
    S = x.shape[0]
    for j in range(1, synth.NUM_QUANTIZERS):
        y_emb[:Tp] += emb[j][prompts[:, j]]
    alpha = o.w["nar_audio_position.alpha"]
    out = []
    for i in range(synth.NUM_QUANTIZERS - 1):
        xy = torch.cat([x, y_emb + alpha * o._pe(Tp + T)[: Tp + T]], 0)
        dec = o._nar_stack(xy, o.w[f"nar_stage_embeddings.{i}.word_embeddings.weight"])
        out.append(F.linear(dec[S + Tp:], o.w[f"nar_predict_layers.{i}.weight"]))
        if i < synth.NUM_QUANTIZERS - 2:
            y_emb[Tp:] += emb[i + 1][cd[:, i + 1]]
    return out


def score_ref(logits, targets):
    """float64 log-softmax value and rank (number of STRICTLY larger logits) of targets[r] in logits[r]; n_near(tol) counts, per row,
    the OTHER columns within tol of the target's logit (the columns whose order against the target an error of tol / 2 per logit
    can change).  Returns (logp (R,) float64, rank (R,) int64, n_near)."""
    l = np.asarray(logits, np.float64)
    t = np.asarray(targets, np.int64).reshape(-1)
    assert l.ndim == 2 and t.shape == (l.shape[0],)
    m = l.max(axis=1, keepdims=True)
    lt = l[np.arange(len(t)), t]
    logp = (lt - m[:, 0]) - np.log(np.exp(l - m).sum(axis=1))
    rank = (l > lt[:, None]).sum(axis=1)

    def n_near(tol):
        return (np.abs(l - lt[:, None]) <= tol).sum(axis=1) - 1

    return logp, rank, n_near


def lse_bound(logits, targets):
    """bound on |logp of the fp32 kernel - float64| per row: 4e-5 + 2^-22 |l_t - max l|.  Every exp argument carries one rounding,
    <= 2^-24 x, and x e^-x <= 0.368: over <= 1025 terms with s >= 1 at most 2.3e-5 in log s; 2 ulp of expf, <= 23 roundings of the
    tree sum and 2 ulp of logf at <= 6.94 together < 5e-6; the two roundings of the final difference give the relative term."""
    l = np.asarray(logits, np.float64)
    t = np.asarray(targets, np.int64).reshape(-1)
    return 4e-5 + 2.0 ** -22 * np.abs(l[np.arange(len(t)), t] - l.max(axis=1))
