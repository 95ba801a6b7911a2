"""GPU: vx_align (text attention of given codes, per frame, from one teacher-forced AR pass) against the float64 oracle, and its
exact properties.

Tolerance of the float64 comparison.  The yardstick of a case is the fp32 oracle's own deviation from the float64 oracle
(tests/_align_refs.align_ref on both), rms and max over the case's (T, S) array, computed here on the CPU.  The `f32` arithmetic must
stay within 4 x both (the rule of tests/test_gpu_kernel_attention.py: the same arithmetic, another summation order).  For `default`
(f16x2) and `bf16x3` the factor is the power of two at or above twice the worst ratio measured on the MI355X (docs/log_r19.md).
Measured, worst of rms and max ratio over the three cases, both code sets and both weight sets: default 1.80 (nl2_force40_mixlang,
perturbed, table, max), bf16x3 1.42, f32 1.63.  Factors: default 4 (>= 2 x 1.80), bf16x3 4 (>= 2 x 1.42), f32 4 (the rule).  The q and
k the kernel reads are the fp32 output of the in_proj in every mode and the softmax is fp32: the arithmetic mode only enters through
the residual stream below the tapped layer."""
import numpy as np
import pytest

from oracle import synth
from oracle.make_golden import CASES, RANGE_CASES, all_cases
from oracle.vallex_oracle import VallexOracle
from tests import _align_refs as A
from tests._score_refs import oracle64
from tests._util import case_model, case_row, get_model, golden

pytestmark = pytest.mark.gpu

NAMES = ["nl2_greedy_eos", "nl2_topk10", "nl2_force40_mixlang"]
FACTOR = {"f32": 4.0, "default": 4.0, "bf16x3": 4.0}
SENT = np.float32(-7.5)
_REF = {}
_GEN = {}
_ORC = {}


def perturbed(codes):
    """a copy with 30 % of all entries redrawn (as tests/test_gpu_score.py)"""
    rng = np.random.default_rng(7)
    mask = rng.random(codes.shape) < 0.3
    return np.where(mask, rng.integers(0, 1024, codes.shape), codes).astype(np.int64)


def table(nl, seed=31):
    """a seeded random weight table with a few zero heads"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 0.2, (nl, 16)) * (rng.random((nl, 16)) < 0.8)).astype(np.float32)


def ref(key, sd, nl, row, codes, hw):
    """(float64 (T, S), yardstick rms, yardstick max) of (row, codes, weights), computed once per key"""
    if key not in _REF:
        wk = (id(sd), nl)
        if wk not in _ORC:
            _ORC.clear()
            _ORC[wk] = (oracle64(sd, nl), VallexOracle(sd, nl), sd)
        o64, o32, _ = _ORC[wk]
        want = A.align_ref64(o64, row, codes[:, 0], hw)
        err = A.align_ref(o32, row, codes[:, 0], hw).astype(np.float64) - want
        _REF[key] = (want, float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max()))
    return _REF[key]


_SD = {}


def _case_refs(name):
    c, row, _ = case_row(name)
    k = (c["num_layers"], c["seed"], c["eos_gain"])
    if k not in _SD:
        _SD[k] = synth.vallex_state_dict(*k)
    own = golden(name)["codes"][0].astype(np.int64)
    return c, row, _SD[k], [("own", own), ("perturbed", perturbed(own))]


def ratios(got, want, y_rms, y_max):
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    err = got.astype(np.float64) - want
    return float(np.sqrt(np.mean(err ** 2))) / y_rms, float(np.abs(err).max()) / y_max


def check_case(m, name, arith):
    """both code sets of a case, uniform weights and the random table, against float64; returns the worst ratio"""
    c, row, sd, sets = _case_refs(name)
    nl = c["num_layers"]
    worst, frames = 0.0, 0
    for wtag, hw in (("uniform", None), ("table", table(nl))):
        res = m.align_batch([row] * len(sets), [cd for _, cd in sets], head_weights=hw)
        frames = sum(len(cd) for _, cd in sets)
        for r, (tag, cd) in zip(res, sets):
            want, y_rms, y_max = ref((name, tag, wtag), sd, nl, row, cd, hw)
            r_rms, r_max = ratios(r["attn"], want, y_rms, y_max)
            print(f"[align] {name} {arith} {tag} w {wtag}: yardstick rms {y_rms:.3e} max {y_max:.3e}; engine {r_rms:.2f} x rms, {r_max:.2f} x max")
            worst = max(worst, r_rms, r_max)
    return worst, frames


# ---- 1. reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["default", "bf16x3", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_align_matches_float64_oracle(name, arith):
    c = CASES[name]
    m = case_model(c, arith=arith)
    worst, frames = check_case(m, name, arith)
    fb = m.engine.last_fallbacks()
    assert fb["prefill"] == 0 and fb["nar"] == 0, fb
    st = m.engine.last_stats()
    assert st["ar_steps"] == 0 and st["frames"] == frames and st["nar_ms"] == 0 and st["ar_ms"] > 0, st
    assert worst <= FACTOR[arith], f"{name} {arith}: {worst:.2f} x the fp32 oracle's own error, allowed {FACTOR[arith]}"


# ---- ragged rows ----------------------------------------------------------------------------------------------------------------
def _rows():
    rows = []
    for i, (tp, sp, nt, lang) in enumerate([(20, 6, 9, "en"), (57, 11, 5, "zh"), (3, 2, 14, "ja")]):      # tests/test_gpu_score.py _ragged
        a, t = synth.synth_prompt(tp, sp, seed=50 + i)
        txt = np.concatenate([t[0], synth.synth_text(nt, 50 + i)])
        rows.append(dict(text=txt, prompt=a[0], enroll=sp, prompt_language=lang, text_language=lang))
    return rows


def _ragged():
    """the three row shapes of tests/test_gpu_score.py's _ragged, their greedy codes, and the alignment of the three-row call"""
    base = CASES["nl2_greedy_eos"]
    m = get_model(base["num_layers"], base["seed"], base["eos_gain"])      # not kept: the model cache may have dropped its engine
    if not _GEN:
        rows = _rows()
        outs = m.inference_batch(rows, top_k=1, force_eos_at=25)
        assert all(len(o) >= 8 for o in outs)
        res = m.engine.align(m.make_batch(rows), outs)
        _GEN.update(rows=rows, outs=outs, res=res)
    return dict(_GEN, m=m)


def _into(eng, batch, codes_list, lens=None, hw=None, **kw):
    n = len(codes_list)
    lens = np.array([len(c) for c in codes_list], np.int32) if lens is None else np.asarray(lens, np.int32)
    stride = max(len(c) for c in codes_list)
    codes = np.zeros((n, stride, 8), np.int64)
    for i, c in enumerate(codes_list):
        codes[i, : len(c)] = c
    attn = np.full((n, stride + 2, int(batch.text_lens.max()) + 3), SENT, np.float32)
    eng.align_into(batch, codes, lens, attn, hw, **kw)
    return attn


# ---- 2. properties --------------------------------------------------------------------------------------------------------------
def test_rows_are_probabilities_and_a_row_alone_equals_the_row_in_the_batch():
    g = _ragged()
    m, rows, outs = g["m"], g["rows"], g["outs"]
    for i, (row, o, a) in enumerate(zip(rows, outs, g["res"])):
        assert a.shape == (len(o), len(row["text"])) and a.dtype == np.float32
        assert (a >= 0).all() and (a.sum(1) <= 1 + 1e-5).all() and (a.sum(1) > 0).all()
        alone = m.engine.align(m.make_batch([row]), [o])[0]
        assert np.abs(alone - a).max() <= 1e-6, (i, float(np.abs(alone - a).max()))
    hw = table(2)
    for a in m.engine.align(m.make_batch(rows), outs, hw):
        assert (a >= 0).all() and (a.sum(1) <= float(hw.sum()) * (1 + 1e-5)).all()


def test_only_the_reported_elements_are_written():
    g = _ragged()
    m, rows, outs = g["m"], g["rows"], g["outs"]
    batch = m.make_batch(rows)
    full = _into(m.engine, batch, outs)
    for i, (row, o) in enumerate(zip(rows, outs)):
        T, S = len(o), len(row["text"])
        np.testing.assert_array_equal(full[i, :T, :S], g["res"][i])
        assert (full[i, T:] == SENT).all() and (full[i, :, S:] == SENT).all()
    # T_b = 0 for the middle row: it writes nothing, the others are what they were
    part = _into(m.engine, batch, outs, lens=[len(outs[0]), 0, len(outs[2])])
    assert (part[1] == SENT).all()
    for i in (0, 2):
        T, S = len(outs[i]), len(rows[i]["text"])
        assert np.abs(part[i, :T, :S] - g["res"][i]).max() <= 1e-6 and (part[i, T:] == SENT).all() and (part[i, :, S:] == SENT).all()
    assert m.engine.last_stats()["frames"] == len(outs[0]) + len(outs[2])
    none = _into(m.engine, batch, outs, lens=[0, 0, 0])
    assert (none == SENT).all() and m.engine.last_stats()["frames"] == 0


def test_forty_rows_in_two_groups_equal_the_rows_alone():
    g = _ragged()
    base = CASES["nl2_greedy_eos"]
    m = get_model(base["num_layers"], base["seed"], base["eos_gain"], max_new=160, max_prompt=96, max_text=32, max_batch=40)
    alone = [m.engine.align(m.make_batch([r]), [o])[0] for r, o in zip(g["rows"], g["outs"])]
    pick = [(7 * i) % 3 for i in range(40)]
    res = m.engine.align(m.make_batch([g["rows"][j] for j in pick]), [g["outs"][j] for j in pick])
    assert m.engine.last_stats()["frames"] == sum(len(g["outs"][j]) for j in pick)
    for i, j in enumerate(pick):
        assert res[i].shape == alone[j].shape and np.abs(res[i] - alone[j]).max() <= 1e-6, (i, j)


# ---- 3. layers ------------------------------------------------------------------------------------------------------------------
def test_layers_add_up():
    name = "nl2_topk10"
    c, row, sd, sets = _case_refs(name)
    tag, cd = sets[0]
    m = case_model(c)
    hw = table(2, seed=41)
    h0, h1 = hw.copy(), hw.copy()
    h0[1] = 0
    h1[0] = 0
    a0, a1, a01 = (m.align_batch([row], [cd], head_weights=h)[0]["attn"] for h in (h0, h1, hw))
    want0, y_rms0, y_max0 = ref((name, tag, "layer0"), sd, 2, row, cd, h0)
    r = ratios(a0, want0, y_rms0, y_max0)
    print(f"[align] layer 0 only: {r[0]:.2f} x rms, {r[1]:.2f} x max")
    assert max(r) <= FACTOR["default"]
    _, _, y_max = ref((name, tag, "both41"), sd, 2, row, cd, hw)
    d = float(np.abs(a0.astype(np.float64) - (a01.astype(np.float64) - a1.astype(np.float64))).max())
    print(f"[align] layer 0 vs both - layer 1: max {d:.3e}, fp32 bound {4 * y_max:.3e}")
    assert d <= 4 * y_max
    assert (a01 >= a0).all() and (a01 >= a1).all() and (a1 > 0).any()


# ---- 4. nothing is disturbed --------------------------------------------------------------------------------------------------------
def test_align_disturbs_neither_generation_nor_scoring_nor_the_decode_state():
    g = _ragged()
    m, rows, outs = g["m"], g["rows"], g["outs"]
    batch = m.make_batch(rows)
    sc0 = m.engine.score(batch, outs)
    m.engine.align(batch, outs)
    again = m.inference_batch(rows, top_k=1, force_eos_at=25)
    for a, b in zip(again, outs):
        np.testing.assert_array_equal(a, b)
    m.engine.align(batch, outs, table(2))
    for (a, b, c_, d), (a2, b2, c2, d2) in zip(sc0, m.engine.score(batch, outs)):
        assert a.tobytes() == a2.tobytes() and b.tobytes() == b2.tobytes() and (c_, d) == (c2, d2)
    # the KV arena and the decode state: prefill, two steps with an align in between, against the same without
    toks = [np.array([o[t, 0] for o in outs], np.int32) for t in range(2)]
    eng = m.engine
    eng.ar_prefill(batch)
    eng.ar_step(toks[0])
    eng.ar_step(toks[1])
    want = eng.ar_logits()
    eng.ar_prefill(batch)
    eng.ar_step(toks[0])
    eng.align(batch, outs)
    eng.ar_step(toks[1])
    eng.align(batch, outs, table(2))
    np.testing.assert_array_equal(eng.ar_logits().view(np.uint32), want.view(np.uint32))


# ---- 5. range guard -----------------------------------------------------------------------------------------------------------------
def test_out_of_range_operands_rerun_the_pass_in_fp32_from_a_zeroed_sum():
    base, _kind = RANGE_CASES["nl2_range_ffn"]
    m = case_model(all_cases()["nl2_range_ffn"])
    assert m.engine.arith_mode() == ("f16x2", "f16x2")
    c, row, sd, sets = _case_refs(base)
    first = m.align_batch([row] * len(sets), [cd for _, cd in sets])
    fb = m.engine.last_fallbacks()
    assert fb["prefill"] == 1 and fb["nar"] == 0, fb
    for r, (tag, cd) in zip(first, sets):
        want, y_rms, y_max = ref((base, tag, "uniform"), sd, c["num_layers"], row, cd, None)
        rr = ratios(r["attn"], want, y_rms, y_max)
        print(f"[align] nl2_range_ffn {tag}: {rr[0]:.2f} x rms, {rr[1]:.2f} x max")
        assert max(rr) <= FACTOR["default"]
    second = m.align_batch([row] * len(sets), [cd for _, cd in sets])
    assert m.engine.last_fallbacks()["prefill"] == 1
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a["attn"].view(np.uint32), b["attn"].view(np.uint32))


# ---- 6. refusals, the Python layer ------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_output_untouched():
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_EINVAL, VX_ESTATE, Batch, Engine
    g = _ragged()
    m, rows, outs = g["m"], g["rows"], g["outs"]
    eng, batch = m.engine, m.make_batch(rows)
    lens = [len(o) for o in outs]
    smax = int(batch.text_lens.max())

    def refused(code, field, e=eng, b=batch, codes=outs, **kw):
        try:
            _into(e, b, codes, **kw)
        except VallexHipError as err:
            assert err.code == code, err
            assert field in str(err), (field, str(err))
            return
        raise AssertionError(f"accepted: {field} {kw}")

    codes = np.zeros((3, max(lens), 8), np.int64)
    attn = np.full((3, max(lens), smax), SENT, np.float32)
    for bad in (dict(lens=[1, -1, 1]), dict(lens=[1, eng.max_new + 1, 1]), dict(codes_stride=max(lens) - 1),
                dict(out_stride=max(lens) - 1), dict(text_out_stride=smax - 1), dict(hw=np.zeros((2, 16), np.float32))):
        kw = dict(bad)
        with pytest.raises(VallexHipError) as e:
            eng.align_into(batch, codes, np.array(kw.pop("lens", lens), np.int32), attn, kw.pop("hw", None), **kw)
        assert e.value.code == VX_EINVAL, e.value
        assert (attn == SENT).all(), bad
    refused(VX_EINVAL, "lens", lens=[lens[0], -1, lens[2]])
    refused(VX_EINVAL, "lens", lens=[lens[0], eng.max_new + 1, lens[2]])
    refused(VX_EINVAL, "codes_stride", codes_stride=max(lens) - 1)
    refused(VX_EINVAL, "out_stride", out_stride=max(lens) - 1)
    refused(VX_EINVAL, "text_out_stride", text_out_stride=smax - 1)
    hi, neg, deep = [o.copy() for o in outs], [o.copy() for o in outs], [o.copy() for o in outs]
    hi[1][2, 0] = 1024
    neg[2][1, 0] = -1
    deep[2][1, 3] = -1
    refused(VX_EINVAL, "codes", codes=hi)
    refused(VX_EINVAL, "codes", codes=neg)
    _into(eng, batch, deep)                                              # only codebook 0 is read: accepted
    for v in (np.nan, np.inf, -0.5):
        hw = table(2)
        hw[1, 4] = v
        refused(VX_EINVAL, "head_weights[1][4]", hw=hw)
    refused(VX_EINVAL, "all zero", hw=np.zeros((2, 16), np.float32))
    wide = Batch([r["text"].astype(np.int32) for r in rows], [np.zeros(len(r["text"]), np.int32) for r in rows],
                 [r["prompt"].astype(np.int32) for r in rows])
    wide.text_ids[0, 0] = 5000
    refused(VX_EINVAL, "text id", b=wide)                                # what check_batch refuses
    raw = Engine(0, 2, 2, 16, 16, 16, with_vocos=False)                  # no weights: not finalized
    try:
        refused(VX_ESTATE, "finalized", e=raw)
    finally:
        raw.close()
    with eng.serve(top_k=1, force_eos_at=25):
        refused(VX_EINVAL, "session")
    np.testing.assert_array_equal(eng.align(batch, outs)[1], g["res"][1])     # closing the session allows


def test_the_python_layer_returns_attention_mass_and_segments():
    from vallex_amd.utils.alignment import monotonic_segments
    g = _ragged()
    m, rows, outs = g["m"], g["rows"], g["outs"]
    res = m.align_batch(rows, outs)
    for r, a, row, o in zip(res, g["res"], rows, outs):
        np.testing.assert_array_equal(r["attn"], a)
        np.testing.assert_array_equal(r["text_mass"], a.sum(1))
        n = len(row["text"]) - row["enroll"]
        assert len(o) >= n
        np.testing.assert_array_equal(r["segments"], monotonic_segments(a, row["enroll"]))
        assert r["segments"].shape == (n, 2) and r["segments"][0, 0] == 0 and r["segments"][-1, 1] == len(o) - 1
    short = m.align_batch([rows[2]], [outs[2][:5]])[0]                     # 5 frames for 14 tokens: no path
    assert short["segments"] is None and short["attn"].shape == (5, len(rows[2]["text"]))
    # VALLE.align: the signature of VALLE.score
    row, o = rows[0], outs[0]
    one = m.align(row["text"][None], np.array([len(row["text"])]), row["prompt"][None], row["enroll"], o[None],
                  prompt_language=row["prompt_language"], text_language=row["text_language"], head_weights=table(2))
    want = m.align_batch([row], [o], head_weights=table(2))[0]
    np.testing.assert_array_equal(one["attn"], want["attn"])
    np.testing.assert_array_equal(one["segments"], want["segments"])
