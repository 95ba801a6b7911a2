"""GPU: vx_score (teacher-forced log-probabilities and ranks of given codes) against the float64 oracle, and its exact properties.

Tolerances.  tests/test_gpu_parity.py holds the engine's teacher-forced AR logits to the live reference within 3e-4 and its NAR
logits within 5e-3 on these same 2-layer models; a log-softmax moves by at most twice the largest logit error, so
|logp - logp64| <= 2 tol, and a rank can differ from the float64 rank by at most the number of OTHER columns within 2 tol of the
target's logit, counted per element (n_near).  Everything else here is exact: bit-identical logits score bit-identically."""
import numpy as np
import pytest
import torch

from oracle import synth
from oracle.make_golden import CASES, RANGE_CASES, all_cases
from oracle.vallex_oracle import VallexOracle
from tests._score_refs import ar_logits_tf, nar_logits_tf, oracle64, score_ref
from tests._util import case_model, case_row, get_model, golden

pytestmark = pytest.mark.gpu

TOL_AR, TOL_NAR = 3e-4, 5e-3
MARGIN = 6e-4                                  # float64 top-2 margin above which an arg-max survives a logit error of TOL_AR
NAMES = ["nl2_greedy_eos", "nl2_topk10", "nl2_force40_mixlang"]
EOS = synth.EOS_ID
_REF = {}
_GEN = {}


def perturbed(codes):
    """a copy with 30 % of all entries redrawn"""
    rng = np.random.default_rng(7)
    mask = rng.random(codes.shape) < 0.3
    return np.where(mask, rng.integers(0, 1024, codes.shape), codes).astype(np.int64)


def ref64(key, sd, nl, row, codes):
    """float64 teacher-forced logits of (row, codes): AR (T + 1, 1025) and the 7 NAR stages (T, 1024), computed once per key"""
    if key not in _REF:
        o = oracle64(sd, nl)
        with torch.no_grad():
            _REF[key] = (ar_logits_tf(o, row, codes[:, 0]).numpy(), [l.numpy() for l in nar_logits_tf(o, row, codes)])
    return _REF[key]


def check_row(res, ar64, nar64, codes, parts=3):
    """one row of Engine.score against float64; returns (max |dlogp| AR, NAR, max |drank| AR, NAR)"""
    logp, rank, el, er = res
    T = len(codes)
    assert logp.shape == rank.shape == (T, 8)
    out = [0.0, 0.0, 0, 0]
    if parts & 1:
        lp64, rk64, near = score_ref(ar64, np.concatenate([codes[:, 0], [EOS]]))
        dl = np.abs(np.concatenate([logp[:, 0], [el]]).astype(np.float64) - lp64)
        dr = np.abs(np.concatenate([rank[:, 0], [er]]).astype(np.int64) - rk64)
        assert (dl <= 2 * TOL_AR).all(), ("AR logp", int(dl.argmax()), float(dl.max()))
        assert (dr <= near(2 * TOL_AR)).all(), ("AR rank", int(dr.argmax()), int(dr.max()))
        out[0], out[2] = float(dl.max()), int(dr.max())
    if parts & 2:
        for q in range(1, 8):
            lp64, rk64, near = score_ref(nar64[q - 1], codes[:, q])
            dl = np.abs(logp[:, q].astype(np.float64) - lp64)
            dr = np.abs(rank[:, q].astype(np.int64) - rk64)
            assert (dl <= 2 * TOL_NAR).all(), ("NAR logp", q, int(dl.argmax()), float(dl.max()))
            assert (dr <= near(2 * TOL_NAR)).all(), ("NAR rank", q, int(dr.argmax()), int(dr.max()))
            out[1], out[3] = max(out[1], float(dl.max())), max(out[3], int(dr.max()))
    return out


def _case_refs(name):
    c, row, _ = case_row(name)
    sd = synth.vallex_state_dict(c["num_layers"], c["seed"], c["eos_gain"])
    own = golden(name)["codes"][0].astype(np.int64)
    sets = [("own", own), ("perturbed", perturbed(own))]
    return c, row, [(tag, cd) + ref64((name, tag), sd, c["num_layers"], row, cd) for tag, cd in sets]


# ---- 1. reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["default", "bf16x3", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_score_matches_float64_oracle(name, arith):
    c, row, sets = _case_refs(name)
    m = case_model(c, arith=arith)
    res = m.score_batch([row] * len(sets), [cd for _, cd, _, _ in sets])
    for r, (tag, cd, ar64, nar64) in zip(res, sets):
        worst = check_row((r["logp"], r["rank"], r["eos_logp"], r["eos_rank"]), ar64, nar64, cd)
        print(f"score vs float64 [{name} {arith} {tag}]: max |dlogp| AR {worst[0]:.3e} NAR {worst[1]:.3e}, "
              f"max |drank| AR {worst[2]} NAR {worst[3]}")
    assert m.engine.last_fallbacks()["prefill"] == 0 and m.engine.last_fallbacks()["nar"] == 0
    st = m.engine.last_stats()
    assert st["ar_steps"] == 0 and st["frames"] == sum(len(cd) for _, cd, _, _ in sets) and st["ar_ms"] > 0 and st["nar_ms"] > 0


# ---- 6. range guard ---------------------------------------------------------------------------------------------------
def test_out_of_range_operands_rerun_the_scoring_passes_in_fp32():
    """RANGE_CASES weights are the same fp32 function as their base case with FFN activations beyond fp16: both passes raise the flag,
    are re-run on the fp32 kernels and meet the bounds of the reference test; the in-range base model reports no re-run (test above)"""
    base, _kind = RANGE_CASES["nl2_range_ffn"]
    c, row, sets = _case_refs(base)
    m = case_model(all_cases()["nl2_range_ffn"])
    assert m.engine.arith_mode() == ("f16x2", "f16x2")
    res = m.score_batch([row] * len(sets), [cd for _, cd, _, _ in sets])
    fb = m.engine.last_fallbacks()
    assert fb["prefill"] == 1 and fb["nar"] == 1, fb
    for r, (tag, cd, ar64, nar64) in zip(res, sets):
        check_row((r["logp"], r["rank"], r["eos_logp"], r["eos_rank"]), ar64, nar64, cd)


# ---- ragged rows and what the engine generated for them ---------------------------------------------------------------
def _ragged():
    """the first three row shapes of test_ragged_batch_rows_equal_their_batch1_runs, their greedy codes and the parts=3 scores"""
    if not _GEN:
        base = CASES["nl2_greedy_eos"]
        m = get_model(base["num_layers"], base["seed"], base["eos_gain"])
        rows = []
        for i, (tp, sp, nt, lang) in enumerate([(20, 6, 9, "en"), (57, 11, 5, "zh"), (3, 2, 14, "ja")]):
            a, t = synth.synth_prompt(tp, sp, seed=50 + i)
            txt = np.concatenate([t[0], synth.synth_text(nt, 50 + i)])
            rows.append(dict(text=txt, prompt=a[0], enroll=sp, prompt_language=lang, text_language=lang))
        outs = m.inference_batch(rows, top_k=1, force_eos_at=25)
        assert all(len(o) >= 8 for o in outs)
        res = m.engine.score(m.make_batch(rows), outs)
        _GEN.update(m=m, rows=rows, outs=outs, res=res, sd=synth.vallex_state_dict(base["num_layers"], base["seed"], base["eos_gain"]))
    return _GEN


# ---- 2. scoring what the engine generated, exact ----------------------------------------------------------------------
def test_generated_codes_score_rank_zero():
    g = _ragged()
    for i, (row, codes, (logp, rank, el, er)) in enumerate(zip(g["rows"], g["outs"], g["res"])):
        ar64, _ = ref64(("ragged", i), g["sd"], 2, row, codes)
        top2 = np.sort(ar64[: len(codes)], axis=1)[:, -2:]
        sure = (top2[:, 1] - top2[:, 0]) > MARGIN
        assert (~sure).sum() <= 0.05 * len(codes), ("fixture: too many near-tied frames", i, int((~sure).sum()))
        # the NAR stages score the logits the arg-max was taken from, bit for bit
        assert (rank[:, 1:] == 0).all(), (i, np.argwhere(rank[:, 1:] != 0)[:4])
        assert (rank[sure, 0] == 0).all(), (i, np.flatnonzero(rank[:, 0] != 0))
        assert np.isfinite(logp).all() and (logp <= 0).all() and np.isfinite(el)


# ---- 3. teacher forcing, exact ------------------------------------------------------------------------------------------
def test_a_codebook_only_influences_what_comes_behind_it():
    g = _ragged()
    m, rows = g["m"], g["rows"]
    batch = m.make_batch(rows)
    base = g["res"]
    again = m.engine.score(batch, g["outs"])
    for (a, b, c, d), (a2, b2, c2, d2) in zip(base, again):                  # two calls, one result: what "bit-identical" stands on
        assert a.tobytes() == a2.tobytes() and b.tobytes() == b2.tobytes() and (c, d) == (c2, d2)
    rng = np.random.default_rng(11)
    t0s = [len(o) // 2 for o in g["outs"]]

    def redrawn(k):
        outs = [o.copy() for o in g["outs"]]
        for o, t0 in zip(outs, t0s):
            o[t0:, k] = (o[t0:, k] + rng.integers(1, 1024, len(o) - t0)) % 1024      # every entry changes
        return outs

    for k in (7, 3, 1):
        got = m.engine.score(batch, redrawn(k))
        for (lp, rk, el, er), (lp0, rk0, el0, er0), t0 in zip(got, base, t0s):
            assert lp[:, :k].tobytes() == lp0[:, :k].tobytes() and rk[:, :k].tobytes() == rk0[:, :k].tobytes(), k
            assert lp[:t0, k].tobytes() == lp0[:t0, k].tobytes() and rk[:t0, k].tobytes() == rk0[:t0, k].tobytes(), k
            assert (el, er) == (el0, er0)
            if k < 7:
                assert (lp[:, k + 1] != lp0[:, k + 1]).any(), k
    got = m.engine.score(batch, redrawn(0))
    for (lp, rk, el, er), (lp0, rk0, el0, er0), t0 in zip(got, base, t0s):
        assert lp[:t0, 0].tobytes() == lp0[:t0, 0].tobytes() and rk[:t0, 0].tobytes() == rk0[:t0, 0].tobytes()
        assert lp[t0, 0] != lp0[t0, 0]


# ---- 4. best_of criterion -------------------------------------------------------------------------------------------------
def test_sum_of_scores_is_the_best_of_criterion():
    """nl2_bestof3 inputs and uniforms.  (a) Unfiltered sampling (top_k = -100): sum_t logp[t, 0] + eos_logp of every beam equals the
    sum(logp) the oracle's sampler accumulated (models/vallex.py:572) within (T + 1) x 6e-4; a beam the cap ended took its last term
    at the token it drew, not at EOS, and that one term is exchanged before comparing.  (b) The case's own run (top_k = 10): selecting
    on sum / len^penalty of the scores picks the beam the live reference returned."""
    name = "nl2_bestof3"
    c, row, us = case_row(name)
    sd = synth.vallex_state_dict(c["num_layers"], c["seed"], c["eos_gain"])
    o = VallexOracle(sd, c["num_layers"])
    text, p0 = torch.from_numpy(row["text"].astype(np.int64)), torch.from_numpy(row["prompt"][:, 0].astype(np.int64))
    beams = {}
    with torch.no_grad():
        for tk in (-100, c["top_k"]):
            for j in range(3):
                taps = {}
                gen, slp = o.ar_generate(text, p0, row["enroll"], row["prompt_language"], row["text_language"], top_k=tk,
                                         uniforms=us[:, j], force_eos_at=c["force_eos_at"], taps=taps, return_logp=True)
                if tk < 0 and len(gen) == c["force_eos_at"]:          # forced: exchange the last term (drawn token -> EOS)
                    last = taps["ar_logits"][-1].double().reshape(1, -1)
                    drawn, lp_drawn = o.sample(taps["ar_logits"][-1], tk, 1.0, float(us[len(gen), j]))
                    slp = slp - lp_drawn + float(torch.log_softmax(last, -1)[0, EOS])
                beams[tk, j] = (np.array(gen, np.int64), slp)
    m = case_model(c)
    keys = sorted(beams)
    codes = [np.zeros((len(beams[k][0]), 8), np.int64) for k in keys]
    for cd, k in zip(codes, keys):
        cd[:, 0] = beams[k][0]
    res = m.score_batch([row] * len(keys), codes, parts="ar")
    total = {k: float(r["logp"][:, 0].astype(np.float64).sum() + r["eos_logp"]) for k, r in zip(keys, res)}
    for j in range(3):
        T = len(beams[-100, j][0])
        print(f"beam {j}: T {T}, vx_score sum {total[-100, j]:.5f}, oracle sum_logp {beams[-100, j][1]:.5f}")
        assert abs(total[-100, j] - beams[-100, j][1]) <= (T + 1) * 6e-4
    Tp = len(p0)
    crit = [total[c["top_k"], j] / (1 + Tp + len(beams[c["top_k"], j][0])) ** c.get("length_penalty", 1.0) for j in range(3)]
    pick = int(np.argmax(crit))
    np.testing.assert_array_equal(beams[c["top_k"], pick][0], golden(name)["codes"][0, :, 0])


# ---- 5. parts, batching, edges ----------------------------------------------------------------------------------------------
def _into(eng, batch, codes_list, parts, lens=None, **kw):
    n = len(codes_list)
    lens = np.array([len(c) for c in codes_list], np.int32) if lens is None else np.asarray(lens, np.int32)
    stride = max(len(c) for c in codes_list)
    codes = np.zeros((n, stride, 8), np.int64)
    for i, c in enumerate(codes_list):
        codes[i, : len(c)] = c
    logp, rank = np.full((n, stride, 8), np.nan, np.float32), np.full((n, stride, 8), -7, np.int32)
    elp, erk = np.full(n, np.nan, np.float32), np.full(n, -7, np.int32)
    eng.score_into(batch, codes, lens, parts, logp, rank, elp, erk, **kw)
    return logp, rank, elp, erk


def test_parts_write_exactly_their_columns():
    g = _ragged()
    eng, batch, outs = g["m"].engine, g["m"].make_batch(g["rows"]), g["outs"]
    lens = [len(o) for o in outs]
    full = _into(eng, batch, outs, 3)
    ar, nar = _into(eng, batch, outs, 1), _into(eng, batch, outs, 2)
    for i, T in enumerate(lens):
        for got in (full, ar, nar):                                      # frames behind T_b are never written
            assert np.isnan(got[0][i, T:]).all() and (got[1][i, T:] == -7).all()
        assert np.isfinite(full[0][i, :T]).all() and (full[1][i, :T] >= 0).all()
        assert ar[0][i, :T, 0].tobytes() == full[0][i, :T, 0].tobytes() and ar[1][i, :T, 0].tobytes() == full[1][i, :T, 0].tobytes()
        assert np.isnan(ar[0][i, :, 1:]).all() and (ar[1][i, :, 1:] == -7).all()
        assert nar[0][i, :T, 1:].tobytes() == full[0][i, :T, 1:].tobytes() and nar[1][i, :T, 1:].tobytes() == full[1][i, :T, 1:].tobytes()
        assert np.isnan(nar[0][i, :, 0]).all() and (nar[1][i, :, 0] == -7).all()
    assert ar[2].tobytes() == full[2].tobytes() and ar[3].tobytes() == full[3].tobytes()
    assert np.isnan(nar[2]).all() and (nar[3] == -7).all()
    # VX_SCORE_NAR alone needs neither EOS array
    n = len(outs)
    lp, rk = np.full(full[0].shape, np.nan, np.float32), np.full(full[1].shape, -7, np.int32)
    codes = np.zeros(full[0].shape, np.int64)
    for i, c in enumerate(outs):
        codes[i, : len(c)] = c
    eng.score_into(batch, codes, np.array(lens, np.int32), 2, lp, rk, None, None)
    assert lp.tobytes() == nar[0].tobytes() and n == 3


def test_a_row_alone_equals_the_row_in_the_batch_and_an_empty_row_scores_eos_only():
    g = _ragged()
    m, rows, outs = g["m"], g["rows"], g["outs"]
    for i in (0, 2):
        lp, rk, el, er = m.engine.score(m.make_batch([rows[i]]), [outs[i]])[0]
        lp0, rk0, el0, er0 = g["res"][i]
        assert np.abs(lp[:, 0] - lp0[:, 0]).max() <= 2 * TOL_AR and abs(el - el0) <= 2 * TOL_AR
        assert np.abs(lp[:, 1:] - lp0[:, 1:]).max() <= 2 * TOL_NAR
    # T_b = 0 for the middle row: only its EOS pair is written; the other rows are what they were
    batch = m.make_batch(rows)
    logp, rank, elp, erk = _into(m.engine, batch, outs, 3, lens=[len(outs[0]), 0, len(outs[2])])
    assert np.isnan(logp[1]).all() and (rank[1] == -7).all() and np.isfinite(elp[1]) and elp[1] <= 0 and erk[1] >= 0
    ar64, _ = ref64(("ragged-empty", 1), g["sd"], 2, rows[1], outs[1][:0])
    lp64, rk64, near = score_ref(ar64, [EOS])
    assert abs(elp[1] - lp64[0]) <= 2 * TOL_AR and abs(erk[1] - rk64[0]) <= near(2 * TOL_AR)[0]
    for i in (0, 2):
        T = len(outs[i])
        assert np.abs(logp[i, :T, 0] - g["res"][i][0][:, 0]).max() <= 2 * TOL_AR
        assert np.abs(logp[i, :T, 1:] - g["res"][i][0][:, 1:]).max() <= 2 * TOL_NAR


def test_refused_calls_leave_the_outputs_untouched():
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_EINVAL, VX_ESTATE, Batch, Engine
    g = _ragged()
    m, rows, outs = g["m"], g["rows"], g["outs"]
    eng, batch = m.engine, m.make_batch(rows)
    lens = [len(o) for o in outs]

    def refused(code, field, e=eng, b=batch, codes=outs, parts=3, **kw):
        lp = rk = None
        try:
            _into(e, b, codes, parts, **kw)
        except VallexHipError as err:
            assert err.code == code, err
            assert field in str(err), (field, str(err))
            return
        raise AssertionError(f"accepted: {field} {kw}")

    # _into pre-fills with NaN / -7 and raises before returning: check untouched outputs through score_into directly once
    codes = np.zeros((3, max(lens), 8), np.int64)
    lp, rk = np.full(codes.shape, np.nan, np.float32), np.full(codes.shape, -7, np.int32)
    el, er = np.full(3, np.nan, np.float32), np.full(3, -7, np.int32)
    for bad in (dict(parts=0), dict(parts=4), dict(parts=3, lens=[1, -1, 1]), dict(parts=3, lens=[1, eng.max_new + 1, 1]),
                dict(parts=3, codes_stride=max(lens) - 1), dict(parts=3, out_stride=max(lens) - 1)):
        kw = dict(bad)
        with pytest.raises(VallexHipError) as e:
            eng.score_into(batch, codes, np.array(kw.pop("lens", lens), np.int32), kw.pop("parts"), lp, rk, el, er, **kw)
        assert e.value.code == VX_EINVAL, e.value
        assert np.isnan(lp).all() and (rk == -7).all() and np.isnan(el).all() and (er == -7).all(), bad
    refused(VX_EINVAL, "parts", parts=0)
    refused(VX_EINVAL, "parts", parts=4)
    refused(VX_EINVAL, "lens", lens=[lens[0], -1, lens[2]])
    refused(VX_EINVAL, "codes_stride", codes_stride=max(lens) - 1)
    refused(VX_EINVAL, "out_stride", out_stride=max(lens) - 1)
    hi, neg = [o.copy() for o in outs], [o.copy() for o in outs]
    hi[1][2, 0] = 1024
    neg[2][1, 3] = -1
    refused(VX_EINVAL, "codes", codes=hi, parts=1)
    refused(VX_EINVAL, "codes", codes=hi, parts=2)                        # the NAR stages embed codebook 0 too
    refused(VX_EINVAL, "codes", codes=neg, parts=2)
    _into(eng, batch, neg, 1)                                            # the AR part does not read codebook 3: accepted
    wide = Batch([r["text"].astype(np.int32) for r in rows], [np.zeros(len(r["text"]), np.int32) for r in rows],
                 [r["prompt"].astype(np.int32) for r in rows])
    wide.text_ids[0, 0] = 5000
    refused(VX_EINVAL, "text id", b=wide)                                # what check_batch refuses
    raw = Engine(0, 2, 2, 16, 16, 16, with_vocos=False)                  # no weights: not finalized
    try:
        refused(VX_ESTATE, "finalized", e=raw)
    finally:
        raw.close()


def test_score_is_refused_inside_a_session_and_changes_nothing():
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_EINVAL
    g = _ragged()
    m, rows, outs = g["m"], g["rows"], g["outs"]
    eng, batch = m.engine, m.make_batch(rows)
    got = {}
    with eng.serve(top_k=1, force_eos_at=25) as sess:
        ids = sess.submit(batch, [dict() for _ in rows])
        sess.run(3, lambda rid, c: got.__setitem__(rid, c))
        with pytest.raises(VallexHipError) as e:
            eng.score(batch, outs)
        assert e.value.code == VX_EINVAL and "session" in str(e.value)
        sess.run(0, lambda rid, c: got.__setitem__(rid, c))
    for rid, o in zip(ids, outs):
        np.testing.assert_array_equal(got[rid], o)
    # and generation after scoring is what it was: the golden ids
    name = "nl2_greedy_eos"
    c, row, us = case_row(name)
    m.score_batch([row], [golden(name)["codes"][0]])
    out = m.inference_batch([row], top_k=c["top_k"], force_eos_at=c["force_eos_at"])[0]
    np.testing.assert_array_equal(out, golden(name)["codes"][0])
