"""GPU: per-request logit filters (top_p, repetition penalty, min_frames) of the serving session through the C ABI
(vx_serve_submit_filtered) and ServeSession.

Contract: a request returns the same result whatever else is in the session; with the neutral filters it returns what a batch-1
vx_infer call returns (the live-reference goldens); with filters it follows the float64 reference of tests/_filter_refs.py applied
to the oracle's logits (first-codebook ids equal along trajectories whose every decision is at least 1e-4 of probability mass away
from flipping -- twenty times the engine-to-reference logit distance DESIGN.md section 2 measures, 5e-6).
Caps: force_eos_at <= 24.  Sessions of 4, 8 and 32 decode rows: the three decode chains."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import synth
from oracle.make_golden import all_cases, case_inputs
from oracle.vallex_oracle import VallexOracle
from tests import _filter_refs as FR
from tests import _kernel_refs as R
from tests._util import case_model, get_model, golden

pytestmark = pytest.mark.gpu

NL, SEED = 2, 12
SIZES = pytest.mark.parametrize("max_batch", [4, 8, 32], ids=["sb_chain", "split_fused", "rows32"])


def _model(max_batch, eos_gain=2.5, max_new=64):
    return get_model(NL, SEED, eos_gain, max_new=max_new, max_prompt=128, max_text=64, max_batch=max_batch)


def _rows(n, seed, text_lo=2, text_hi=19):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        tp = int(rng.choice([0, 1, 2, int(rng.integers(3, 91))]))
        sp = 0 if tp == 0 else int(rng.integers(1, 13))
        a, t = synth.synth_prompt(tp, sp, seed=int(rng.integers(1, 1 << 30)))
        txt = np.concatenate([t[0], synth.synth_text(int(rng.integers(text_lo, text_hi)), int(rng.integers(1, 1 << 30)))])
        rows.append(dict(text=txt, prompt=a[0], enroll=sp, prompt_language=("en", "zh", "ja")[int(rng.integers(0, 3))],
                         text_language=("en", "zh", "ja")[int(rng.integers(0, 3))]))
    return rows


def _run_all(sess, m, rows, reqs):
    got = {}
    ids = sess.submit(m.make_batch(rows), reqs)
    assert sess.run(0, lambda rid, c: got.__setitem__(rid, c)) == (0, 0)
    return [got[i] for i in ids]


# ---- 1. neutral filters equal the goldens ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nl2_topk10", "nl2_full_multinomial"])
def test_neutral_filters_equal_the_golden(name):
    c = all_cases()[name]
    a, t, text, pl, langs = case_inputs(c)
    row = dict(text=text[0], prompt=a[0], enroll=t.shape[-1], prompt_language=pl, text_language=langs)
    q = dict(top_k=c["top_k"], temperature=c.get("temperature", 1.0), force_eos_at=-1 if c["force_eos_at"] is None else c["force_eos_at"],
             uniforms=synth.uniforms(4096, 1, c["useed"])[:, 0], top_p=1.0, repetition_penalty=1.0, repetition_window=0, min_frames=0)
    m = case_model(c, max_new=64, max_prompt=400, max_text=256, max_batch=4)
    calls = []
    with m.engine.serve(top_k=1, temperature=1.3, force_eos_at=2) as sess:
        sess.lib = _Spy(m.engine.lib, "vx_serve_submit_filtered", calls)
        out = _run_all(sess, m, [row], [q])[0]
    assert calls == ["vx_serve_submit_filtered"]                         # the request went through the new entry
    gold = golden(name)["codes"][0]
    assert out.shape == gold.shape, (out.shape, gold.shape)
    assert (out == gold).all(), f"{name}: {int((out != gold).sum())} ids differ from the live-reference golden"


class _Spy:
    """the library handle with one entry recorded"""

    def __init__(self, lib, name, calls):
        self._lib, self._name, self._calls = lib, name, calls

    def __getattr__(self, k):
        f = getattr(self._lib, k)
        if k != self._name:
            return f

        def rec(*a):
            self._calls.append(k)
            return f(*a)
        return rec


# ---- 2. session invariance ------------------------------------------------------------------------------------------------------
def _random_requests(n, nd, seed):
    rng = np.random.default_rng(seed)
    reqs = []
    for i in range(n):
        b = min(int(rng.choice([1, 2, 3])), nd)
        q = dict(best_of=b, top_k=int(rng.choice([-100, 10, 50])), temperature=float(rng.choice([0.7, 1.0, 1.5])),
                 force_eos_at=int(rng.choice([6, 15, 24])), length_penalty=(1.0, 0.7)[i % 2],
                 top_p=(None, 0.5, 0.8, 0.95)[int(rng.integers(0, 4))], repetition_penalty=(None, 1.3, 0.8, 1.1)[int(rng.integers(0, 4))],
                 repetition_window=(None, 0, 1, 4)[int(rng.integers(0, 4))], min_frames=(None, 0, 3, 30)[int(rng.integers(0, 4))])
        if i % 2:
            q["uniforms"] = synth.uniforms(64, b, seed + 100 + i)
        else:
            q["seed"] = 7_000_000_000 + 131 * i + seed
        reqs.append(q)
    reqs[0].update(top_p=0.8, repetition_penalty=1.3, min_frames=3)      # every filter at once, at least once
    reqs[1].update(top_p=None, repetition_penalty=None, repetition_window=None, min_frames=None)      # and a neutral request
    return reqs


@SIZES
def test_a_request_returns_the_same_alone_and_in_a_crowd(max_batch):
    m = _model(max_batch)
    nd = min(max_batch, 32)
    n = 12
    rows = _rows(n, 12_100 + max_batch)
    reqs = _random_requests(n, nd, 12_200 + max_batch)
    alone = []
    for r, q in zip(rows, reqs):
        with m.engine.serve(top_k=3, temperature=1.1, force_eos_at=12) as sess:
            alone.append(_run_all(sess, m, [r], [q])[0])
    # the crowd, in three waves between short runs
    with m.engine.serve(top_k=3, temperature=1.1, force_eos_at=12) as sess:
        got, ids = {}, []
        for k in range(3):
            ids += sess.submit(m.make_batch(rows[4 * k:4 * k + 4]), reqs[4 * k:4 * k + 4])
            sess.run(3, lambda rid, c: got.__setitem__(rid, c))
        assert sess.run(0, lambda rid, c: got.__setitem__(rid, c)) == (0, 0)
    for i, rid in enumerate(ids):
        np.testing.assert_array_equal(got[rid], alone[i], err_msg=f"request {i} ({reqs[i]}): crowd != alone")
    # the crowd again, admitted into rows a cancelled request (filters of its own, long history) has just freed
    long_row = dict(rows[0], text=np.concatenate([rows[0]["text"][:rows[0]["enroll"]], synth.synth_text(20, 12_300)]))
    with m.engine.serve(top_k=3, temperature=1.1, force_eos_at=12) as sess:
        got = {}
        victim = sess.submit(m.make_batch([long_row]), [dict(best_of=nd if nd <= 4 else 3, seed=5, top_k=-100, force_eos_at=24, top_p=0.6,
                                                             repetition_penalty=1.7, min_frames=24)])[0]
        assert sess.run(5, lambda rid, c: got.__setitem__(rid, c))[0] == 1
        assert sess.cancel(victim) == "decoding"
        ids = sess.submit(m.make_batch(rows), reqs)
        assert sess.run(0, lambda rid, c: got.__setitem__(rid, c)) == (0, 0)
    assert sorted(got) == ids
    for i, rid in enumerate(ids):
        np.testing.assert_array_equal(got[rid], alone[i], err_msg=f"request {i} ({reqs[i]}): after a cancel != alone")
    lens = [a.shape[0] for a in alone]
    assert len(set(lens)) > 2, lens
    assert all(a.shape[0] >= min(q["min_frames"] or 0, q["force_eos_at"], 16 * len(r["text"])) for a, q, r in zip(alone, reqs, rows))
    print(f"max_batch {max_batch}: lengths {lens}")


# ---- 3. oracle trajectory -------------------------------------------------------------------------------------------------------
TRAINED = dict(num_layers=2, seed=5, eos_gain=1.85, trained=True)
MARGIN = 1e-4


def _oracle_requests():
    """6 requests of at most 24 frames with injected draws; the draw seeds were chosen on the CPU so that every trajectory of the
    oracle keeps MARGIN (test_oracle_trajectories asserts it before it looks at the GPU)"""
    rows = _rows(6, 12_400, text_lo=3)
    flt = [dict(top_k=-100, temperature=1.0, top_p=0.9),
           dict(top_k=50, temperature=1.0, top_p=0.8, repetition_penalty=1.3, repetition_window=8),
           dict(top_k=-100, temperature=0.8, top_p=0.95, min_frames=10),
           dict(top_k=10, temperature=1.2, repetition_penalty=1.2, repetition_window=0, min_frames=4),
           dict(top_k=-100, temperature=1.0, top_p=0.6, repetition_penalty=0.8, repetition_window=3, min_frames=24),
           dict(top_k=20, temperature=1.5, top_p=0.85, repetition_penalty=1.5, repetition_window=16, min_frames=2)]
    return rows, [dict(f, force_eos_at=(24, 20, 16, 24, 24, 12)[i], uniforms=synth.uniforms(32, 1, ORACLE_USEEDS[i])[:, 0])
                  for i, f in enumerate(flt)]


ORACLE_USEEDS = (12_500, 12_510, 12_520, 12_530, 12_540, 12_550)


def oracle_trajectory(orc, row, q):
    """the test's own decode loop on the oracle's pieces with the float64 filtered sampler and the request's draws: (first-codebook
    ids, smallest decision margin: the distance of u from the nearest inner CDF edge and the nucleus margin, per step)"""
    text = torch.from_numpy(np.asarray(row["text"]).astype(np.int64))
    codes0 = torch.from_numpy(np.asarray(row["prompt"])[:, 0].astype(np.int64))
    h, kv, S = orc.ar_prefill(text, codes0, int(row["enroll"]), row["prompt_language"], row["text_language"])
    Tp = len(codes0)
    gen, margin = [], np.inf
    tp, rp = q.get("top_p", 1.0), q.get("repetition_penalty", 1.0)
    win, mf = q.get("repetition_window", 0), q.get("min_frames", 0)
    while True:
        n = len(gen)
        lg = orc.ar_logits(h).detach().numpy().astype(np.float32).reshape(-1)
        v, kept, p, cdf = FR.filtered_sampler_ref(lg, gen, q["top_k"], q["temperature"], tp, rp, win, mf, n)
        u = float(q["uniforms"][n])
        tok = R.sample_token(p, cdf, u)
        edges = cdf[np.flatnonzero(kept)][:-1]
        if len(edges):
            margin = min(margin, float(np.abs(edges - u).min()))
        if tp < 1.0:
            margin = min(margin, FR.nucleus_margin(lg, gen, q["top_k"], q["temperature"], tp, rp, win, mf, n))
        if n >= q["force_eos_at"]:
            tok = R.EOS
        if tok == R.EOS or (1 + n) > 16 * S:
            return gen, margin
        gen.append(tok)
        h, kv = orc.ar_step(tok, Tp + 1 + n, kv)


@pytest.fixture(scope="module")
def oracle_runs():
    from oracle.make_golden import case_state_dict
    orc = VallexOracle(case_state_dict(TRAINED), TRAINED["num_layers"])
    rows, reqs = _oracle_requests()
    with torch.no_grad():
        return rows, reqs, [oracle_trajectory(orc, r, q) for r, q in zip(rows, reqs)]


def test_oracle_trajectories(oracle_runs):
    rows, reqs, want = oracle_runs
    for i, (gen, margin) in enumerate(want):                             # the inputs first, on the CPU
        assert margin >= MARGIN, (i, margin)
        assert len(gen) <= 24
        assert len(gen) >= min(reqs[i].get("min_frames", 0), reqs[i]["force_eos_at"], 16 * len(rows[i]["text"])), (i, len(gen))
    assert sum(len(g) for g, _ in want) >= 60
    for max_batch in (4, 8, 32):
        m = case_model(TRAINED, max_new=64, max_prompt=128, max_text=64, max_batch=max_batch)
        with m.engine.serve(top_k=1, temperature=1.0, force_eos_at=3) as sess:
            outs = _run_all(sess, m, rows, reqs)
        for i, (out, (gen, _)) in enumerate(zip(outs, want)):
            assert out.shape[0] == len(gen) and (out[:, 0] == np.array(gen, np.int64)).all(), (max_batch, i, out[:, 0].tolist(), gen)
    print(f"oracle trajectories: lengths {[len(g) for g, _ in want]}, margins {[f'{mg:.1e}' for _, mg in want]}")


# ---- 4. distribution ------------------------------------------------------------------------------------------------------------
def _chi2_pvalue(obs, p, n):
    """chi-square goodness of fit of counts obs against probabilities p, bins merged (smallest first) to an expected count >= 5"""
    from scipy.stats import chi2
    order = np.argsort(p)
    e_bins, o_bins, e_acc, o_acc = [], [], 0.0, 0
    for i in order:
        e_acc += p[i] * n
        o_acc += obs[i]
        if e_acc >= 5:
            e_bins.append(e_acc)
            o_bins.append(o_acc)
            e_acc, o_acc = 0.0, 0
    if e_acc > 0 or o_acc:
        e_bins[-1] += e_acc
        o_bins[-1] += o_acc
    e, o = np.array(e_bins), np.array(o_bins, np.float64)
    stat = float(((o - e) ** 2 / e).sum())
    return float(chi2.sf(stat, len(e) - 1)), len(e), stat


@pytest.mark.parametrize("top_k,top_p,temperature", [(-100, 0.85, 1.0), (50, 0.9, 1.5)])
def test_first_token_distribution_under_top_p(top_k, top_p, temperature):
    """3000 seeded requests sample the first token of one fixed row: its histogram against the float64 filtered distribution of the
    prefill logits (vx_ar_logits); no count on a token outside the float64 nucleus.  The row is the first of eight candidates whose
    prefill logits keep the nucleus margin of the kernel tests (2^-12)."""
    m = _model(32, eos_gain=1.0, max_new=8)
    for row in _rows(8, 12_600):
        m.engine.ar_prefill(m.make_batch([row]))
        lg = m.engine.ar_logits()[0].astype(np.float32)
        if FR.nucleus_margin(lg, [], top_k, temperature, top_p) >= FR.MARGIN_MIN:
            break
    else:
        raise AssertionError("no candidate row keeps the nucleus margin")
    _, kept, p, _ = FR.filtered_sampler_ref(lg, [], top_k, temperature, top_p, 1.0, 0, 0, 0)
    n = 3000
    counts = np.zeros(1025, np.int64)
    with m.engine.serve(top_k=1, temperature=1.0, force_eos_at=-1) as sess:
        got = {}
        for w in range(0, n, 500):
            k = min(500, n - w)
            sess.submit(m.make_batch([row] * k), [dict(seed=2_000_003 * (w + i) + 29, top_k=top_k, temperature=temperature, top_p=top_p,
                                                       force_eos_at=1) for i in range(k)])
            assert sess.run(0, lambda rid, c: got.__setitem__(rid, c)) == (0, 0)
    assert len(got) == n
    for c in got.values():
        assert c.shape[0] <= 1
        counts[int(c[0, 0]) if c.shape[0] else 1024] += 1
    assert counts[~kept].sum() == 0, "a token outside the float64 nucleus was drawn"
    pv, bins, stat = _chi2_pvalue(counts, p, n)
    print(f"top_k {top_k} top_p {top_p} T {temperature}: nucleus {int(kept.sum())}, chi2 {stat:.1f} over {bins} bins, p = {pv:.4f}")
    assert bins >= 3, bins
    assert pv > 1e-4, (pv, stat, bins)


# ---- 5. argument checks ---------------------------------------------------------------------------------------------------------
def test_filtered_refusals_enqueue_nothing():
    from vallex_amd._capi import VX_EINVAL, _ptr, vx_request, vx_request_filters
    m = _model(4)
    row = _rows(1, 12_700)[0]
    b = m.make_batch([row, row])
    with m.engine.serve(top_k=10, force_eos_at=6) as sess:
        def raw(vals, size=C.sizeof(vx_request_filters), null=False):
            arr = (vx_request * 2)()
            flt = (vx_request_filters * 2)()
            for i in range(2):
                arr[i].struct_size = C.sizeof(vx_request)
                arr[i].best_of = 1
                arr[i].length_penalty = 1.0
                arr[i].seed = 40 + i
                flt[i].struct_size = size
                flt[i].top_p, flt[i].repetition_penalty, flt[i].repetition_window, flt[i].min_frames = vals[i]
            out = np.full(2, -7, np.int64)
            rc = m.engine.lib.vx_serve_submit_filtered(sess.h, C.byref(b.c), arr, None, None if null else flt, _ptr(out, C.c_int64))
            return rc, m.engine.lib.vx_last_error(m.engine.ctx).decode(), out

        ok = (0.9, 1.2, 4, 2)
        nan, inf = float("nan"), float("inf")
        for bad, word in (((0.0, 1.2, 4, 2), "top_p"), ((-0.1, 1.2, 4, 2), "top_p"), ((1.5, 1.2, 4, 2), "top_p"), ((nan, 1.2, 4, 2), "top_p"),
                          ((inf, 1.2, 4, 2), "top_p"), ((0.9, 0.0, 4, 2), "repetition_penalty"), ((0.9, -1.0, 4, 2), "repetition_penalty"),
                          ((0.9, nan, 4, 2), "repetition_penalty"), ((0.9, inf, 4, 2), "repetition_penalty"),
                          ((0.9, 1.2, -1, 2), "repetition_window"), ((0.9, 1.2, 4, -1), "min_frames")):
            rc, msg, out = raw([ok, bad])
            assert rc == VX_EINVAL and word in msg, (bad, msg)
            assert list(out) == [-7, -7]
        rc, msg, _ = raw([ok, ok], size=16)
        assert rc == VX_EINVAL and "struct_size" in msg, msg
        for kw, word in ((dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"), (dict(repetition_penalty=0.0), "repetition_penalty"),
                         (dict(repetition_window=-1), "repetition_window"), (dict(min_frames=-2), "min_frames")):
            with pytest.raises(ValueError, match=word):
                sess.submit(b, [dict(seed=1), dict(seed=2, **kw)])
        assert sess.run(0, None) == (0, 0) and m.engine.last_stats()["ar_steps"] == 0       # nothing was enqueued
        # the session is still usable: flt NULL is vx_serve_submit_ex, and a valid record is taken
        want = _run_all(sess, m, [row, row], [dict(seed=40), dict(seed=41)])
        rc, msg, out = raw([ok, ok], null=True)
        assert rc == 0, msg
        got = {}
        assert sess.run(0, lambda rid, c: got.__setitem__(rid, c)) == (0, 0)
        for i in range(2):
            np.testing.assert_array_equal(got[int(out[i])], want[i])
        rc, msg, out = raw([ok, (1.0, 1.0, 0, 0)])
        assert rc == 0 and list(out) == [int(out[0]), int(out[0]) + 1], msg
        got = {}
        assert sess.run(0, lambda rid, c: got.__setitem__(rid, c)) == (0, 0)
        np.testing.assert_array_equal(got[int(out[1])], want[1])           # the neutral record: today's result
        assert got[int(out[0])].shape[0] >= 2                               # min_frames 2 (force_eos_at 6)
