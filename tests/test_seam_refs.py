"""CPU: the references of tests/_seam_refs.py are pinned to what the project already trusts -- the embedding code of
oracle/vallex_oracle.py, the draw formula of include/vallex_hip.h and tests/test_gpu_continuous.py, torch.argmax -- and the assertion
helper rejects plausible wrong kernels on the very inputs tests/test_gpu_kernel_seam.py launches.  Also asserted here: the condition on
the embedding inputs under which a fused multiply-add or a re-associated sum cannot pass (alpha is not a power of two)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle.vallex_oracle import LANG_ID, VallexOracle
from tests import _seam_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, i32 = np.float32, np.int32


def _mutant_rejected(ref, kw, mutant, name):
    want, got = ref(**kw), ref(**kw, mutant=mutant)
    R.check(ref(**kw), want, name)                                         # the helper accepts the reference itself ...
    assert R.rejects(got, want), f"{name}: the wrong kernel '{mutant}' passes"      # ... and not the wrong kernel


# ---- pins ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def orc():
    rng = np.random.default_rng(31)
    sd = {}
    for which in ("ar", "nar"):
        sd[f"{which}_text_embedding.word_embeddings.weight"] = rng.standard_normal((40, 1024)).astype(f32)
        sd[f"{which}_language_embedding.word_embeddings.weight"] = rng.standard_normal((3, 1024)).astype(f32)
        sd[f"{which}_text_position.alpha"] = np.array([R.ALPHA if which == "ar" else 2.5], f32)
    for j in range(8):
        sd[f"nar_audio_embeddings.{j}.word_embeddings.weight"] = rng.standard_normal((32, 1024)).astype(f32)
    sd["nar_audio_position.alpha"] = np.array([1.37], f32)
    return VallexOracle(sd, 2), sd


@pytest.mark.parametrize("which,langs", [("ar", ("zh", ["en", "ja", "ja", "zh", "en", "en", "ja"])), ("nar", ("en", "ja")), ("ar", (None, None))])
def test_embed_rows_ref_is_the_oracles_text_embedding(orc, which, langs):
    o, sd = orc
    text = np.array([5, 39, 0, 5, 17, 17, 2, 8, 30, 1, 5], np.int64)
    enroll = 4
    want = o._text_embed(which, torch.from_numpy(text), enroll, *langs).numpy()
    idB = None if langs[0] is None else o.text_language_ids(len(text), enroll, *langs)
    got = R.embed_rows_ref(sd[f"{which}_text_embedding.word_embeddings.weight"], text.astype(i32),
                           None if idB is None else sd[f"{which}_language_embedding.word_embeddings.weight"], idB,
                           sd[f"{which}_text_position.alpha"][0], o._pe(len(text)).numpy(), np.arange(len(text), dtype=i32), None, len(text))
    R.check(got, want, f"embed_rows vs _text_embed({which})")
    if idB is not None:                                                    # idB = -1 is the oracle's "no language embedding" row by row
        none = o._text_embed(which, torch.from_numpy(text), enroll, None, None).numpy()
        got = R.embed_rows_ref(sd[f"{which}_text_embedding.word_embeddings.weight"], text.astype(i32),
                               sd[f"{which}_language_embedding.word_embeddings.weight"], np.full(len(text), -1, i32),
                               sd[f"{which}_text_position.alpha"][0], o._pe(len(text)).numpy(), np.arange(len(text), dtype=i32), None, len(text))
        R.check(got, none, "embed_rows with idB = -1")


def test_nar_embedding_refs_are_the_oracles_nar_generate_statements(orc):
    """the statements of VallexOracle.nar_generate (oracle/vallex_oracle.py, models/vallex.py:605-607, 659-667, 682-683) on the same ids:
    y_emb = emb_0[y]; y_emb[:Tp] += emb_j[prompts[:, j]]; y_pos = y_emb + alpha * pe; y_emb[Tp:] += emb_{i+1}[samples]"""
    o, sd = orc
    rng = np.random.default_rng(32)
    Tp, T, S = 5, 4, 3
    prompts, codes0, samples = rng.integers(0, 32, (Tp, 8)), rng.integers(0, 32, T), rng.integers(0, 32, T)
    emb = [o.w[f"nar_audio_embeddings.{j}.word_embeddings.weight"] for j in range(8)]
    y = torch.cat([torch.from_numpy(prompts[:, 0]), torch.from_numpy(codes0)])
    y_emb = emb[0][y].clone()
    for j in range(1, 8):
        y_emb[:Tp] += emb[j][torch.from_numpy(prompts[:, j])]
    alpha = o.w["nar_audio_position.alpha"]
    y_pos = y_emb + alpha * o._pe(Tp + T)[: Tp + T]
    codes = np.zeros((Tp + T, 8), i32)
    codes[:Tp] = prompts
    codes[Tp:, 0] = codes0
    tabs = np.stack([e.numpy() for e in emb])
    mine = R.nar_yemb_init_ref(tabs, codes, np.array([8] * Tp + [1] * T, i32))
    R.check(mine, y_emb.numpy(), "nar_yemb_init")
    dst = (S + np.arange(Tp + T)).astype(i32)
    out = R.add_pe_scatter_ref(mine, sd["nar_audio_position.alpha"][0], o._pe(Tp + T).numpy(), np.arange(Tp + T, dtype=i32), dst, S + Tp + T)
    R.check(out[S:], y_pos.numpy(), "add_pe_scatter")
    assert (R.bits(out[:S]) == R.bits(R.SENT_F)).all()
    y_emb[Tp:] += emb[1][torch.from_numpy(samples)]
    R.check(R.embed_accum_ref(mine, tabs[1], samples.astype(i32), (Tp + np.arange(T)).astype(i32)), y_emb.numpy(), "embed_accum")


def test_draw_is_the_documented_counter_formula():
    from tests.test_gpu_continuous import _counter_uniforms
    hdr = open(os.path.join(ROOT, "include", "vallex_hip.h")).read()
    assert "u = (splitmix64(splitmix64(splitmix64(seed) + r) + step) >> 40) x 2^-24" in hdr
    assert "u_t = (splitmix64(splitmix64(splitmix64(s) + j) + t) >> 40) x 2^-24" in hdr
    for seed in R.SEEDS:
        for key in (0, 31):
            want = _counter_uniforms(seed, key, 5)
            got = np.array([R.draw(seed, key, t) for t in range(5)], f32)
            R.check(got, want, f"draw seed {seed:#x} key {key}")
            assert (0 <= got).all() and (got < 1).all()
    assert R.mix64(0) == 0xE220A8397B1DCDAF                                 # splitmix64's first output for the seed 0 (Vigna's reference code)


def test_argmax_ref_is_torch_argmax_on_the_tie_inputs_and_skips_nan_where_torch_does_not():
    for N in (1024, 1025):
        x = R.argmax_special(N)
        mine = R.argmax_rows_ref(x, N)
        theirs = torch.argmax(torch.from_numpy(x[:, :N]), dim=-1).numpy()
        assert (mine[:13] == theirs[:13]).all(), (mine, theirs)            # every row without a NaN next to a number -- all-NaN included
        assert list(mine[:13]) == [0, 63, 64, 1023, N - 1, 5, 69, 3, 70, 70, 0, 66, 0]
        # NaN mixed with finite values: torch.argmax treats NaN as the maximum (the first NaN wins), the kernel's `>` never selects one.
        # Such a pass raised the f16x2 range flag and is re-run in fp32: its ids are thrown away, they only have to be table indices.
        assert list(theirs[13:]) == [0, 0] and list(mine[13:]) == [100, 3]


# ---- the condition on the inputs -------------------------------------------------------------------------------------------------
def test_alpha_is_no_power_of_two_and_the_embedding_inputs_separate_fused_from_unfused():
    assert np.frexp(f32(R.ALPHA))[0] != 0.5
    for ref, cases in ((R.embed_rows_ref, R.embed_rows_cases()), (R.add_pe_scatter_ref, R.add_pe_scatter_cases())):
        for c in cases:
            want, fused = ref(**c["kw"]), ref(**c["kw"], mutant="fma")
            written = (R.bits(want) != R.bits(R.SENT_F)).all(1)
            diff = R.bits(want) != R.bits(fused)
            assert not diff[~written].any()
            frac = diff[written].mean()
            assert frac >= 0.10 and diff[written].any(1).all(), (c["name"], frac)
            print(f"{ref.__name__} {c['name']}: a fused multiply-add differs on {100 * frac:.1f} % of the elements")
    for c in R.embed_rows_cases():
        kw = c["kw"]
        if kw["tabB"] is None:
            continue
        want, re_assoc = R.embed_rows_ref(**kw), R.embed_rows_ref(**kw, mutant="reassoc")
        diff = R.bits(want) != R.bits(re_assoc)
        for r in range(len(kw["idA"])):
            o = r if kw["dst"] is None else kw["dst"][r]
            if kw["idB"][r] >= 0:
                assert diff[o].mean() >= 0.10, (c["name"], r, diff[o].mean())
            else:
                assert not diff[o].any()


# ---- wrong kernels the helper must reject ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", ["fma", "reassoc", "idb_row0"])
def test_wrong_embed_rows_is_rejected(mutant):
    for c in R.embed_rows_cases():
        if c["kw"]["tabB"] is not None or mutant == "fma":
            _mutant_rejected(R.embed_rows_ref, c["kw"], mutant, f"embed_rows {c['name']}")


def test_wrong_nar_and_scatter_embeddings_are_rejected():
    _mutant_rejected(R.nar_yemb_init_ref, R.nar_yemb_init_cases()[0]["kw"], "one_more", "nar_yemb_init")
    _mutant_rejected(R.add_pe_scatter_ref, R.add_pe_scatter_cases()[0]["kw"], "fma", "add_pe_scatter")
    kw = R.embed_accum_cases()[0]["kw"]
    got = R.embed_accum_ref(**kw)
    got[0, 5] = np.nextafter(got[0, 5], f32(9))                             # a row nobody named moved by one ulp
    assert R.rejects(got, R.embed_accum_ref(**kw))
    got = R.embed_accum_ref(**kw)
    got[-1, 0] = 0                                                         # a word behind the end
    assert R.rejects(got, R.embed_accum_ref(**kw))
    a, b = np.array([0.0, 1.0], f32), np.array([-0.0, 1.0], f32)
    assert R.rejects(a, b) and not R.rejects(a, a.copy())                 # bit-identical means the sign of zero, too


@pytest.mark.parametrize("mutant,rows", [("last", (5, 6, 7, 11)), ("lane_first", (7,)), ("negzero", (8,))])
def test_wrong_argmax_is_rejected(mutant, rows):
    for N in (1024, 1025):
        x = R.argmax_special(N)
        want, got = R.argmax_rows_ref(x, N, R.EXTRA), R.argmax_rows_ref(x, N, R.EXTRA, mutant=mutant)
        assert set(np.flatnonzero(want != got)) >= set(rows), (mutant, np.flatnonzero(want != got))
        assert R.rejects(got, want)
    hit = [c["name"] for c in R.argmax_cases() if R.rejects(R.argmax_rows_ref(**c["kw"], mutant=mutant), R.argmax_rows_ref(**c["kw"]))]
    assert len(hit) >= 2, hit                                              # ... and in the launches of the GPU test, at both N


@pytest.mark.parametrize("mutant", ["swap_ht", "q_for_k"])
def test_wrong_kv_scatter_is_rejected(mutant):
    _mutant_rejected(R.kv_scatter_ref, R.kv_scatter_cases()[0]["kw"], mutant, "kv_scatter")


@pytest.mark.parametrize("mutant", ["len-1", "len+1", "dh_from_dh"])
def test_wrong_beam_fanout_is_rejected(mutant):
    cases = R.beam_fanout_cases()
    for c in cases[:3] if mutant != "dh_from_dh" else (cases[0], cases[3]):
        kw = dict(c["kw"])
        if mutant == "len+1" and (kw["pairs"][:, 2] == kw["Tmax"]).any():
            continue
        _mutant_rejected(R.beam_fanout_ref, kw, mutant, f"beam_fanout {c['name']}")
    lens = sorted(int(n) for c in cases for n in c["kw"]["pairs"][:, 2])
    assert lens == [0, 1, 15, 16, 47, 48, 63, 64, 65, 129]


def test_wrong_state_kernels_are_rejected():
    for c in R.admit_rows_cases():
        _mutant_rejected(R.admit_rows_ref, c["kw"], "meta_of_row", f"admit_rows {c['name']}")
    c = R.admit_mask_cases()[2]["kw"]
    st0 = R.admit_mask_ref(0, c["admitted"], c["state"])
    kw = dict(phase=1, admitted=c["admitted"], state=R.admit_mask_sampled(st0, c["admitted"]), extra=R.EXTRA)
    _mutant_rejected(R.admit_mask_ref, kw, "forget_saved", "admit_mask phase 1")
    st1 = R.admit_mask_ref(**kw)
    assert st0["active"][3] == 1 and st0["saved"][3] == 0 and st1["active"][3] == 0      # the predecessor of row 3 does not revive
    hit = 0
    for c in R.serve_cancel_cases():
        hit += R.rejects(R.serve_cancel_ref(**c["kw"], mutant="no_recount"), R.serve_cancel_ref(**c["kw"]))
    assert hit == len(R.serve_cancel_cases())                              # the incoming n_active is never the right count
    st = R.make_state(1)
    blk = R.pack_state(st, R.EXTRA)
    R.check(R.unpack_state(blk, st["gen"].shape[1], R.EXTRA), R._copy_state(st, R.EXTRA), "pack / unpack")
    blk[R.DEV_SEAM_STATE["slot_meta"] + 4 * 9 + 3] += 1                    # one word of a neighbour's slot record
    assert R.rejects(R.unpack_state(blk, st["gen"].shape[1], R.EXTRA), R._copy_state(st, R.EXTRA))


@pytest.mark.parametrize("mutant", ["key_is_row", "shift39"])
def test_wrong_uniforms_are_rejected(mutant):
    for c in R.admit_uniforms_cases()[:4]:
        _mutant_rejected(R.admit_uniforms_ref, c["kw"], mutant, f"admit_uniforms {c['name']}")
    for c in R.serve_uniforms_cases():
        _mutant_rejected(R.serve_uniforms_ref, c["kw"], mutant, f"serve_uniforms {c['name']}")


def test_uniforms_inputs_cover_what_the_issue_names():
    cases = R.admit_uniforms_cases()
    assert {c["kw"]["seed"] for c in cases[:4]} == {0, 1, 2 ** 32, 2 ** 63 + 12345} and {c["kw"]["steps"] for c in cases[:4]} == {1, 255, 256, 257}
    keys = {int(r) for c in cases for r in c["kw"]["pairs"][:, 1]}
    assert {0, 31} <= keys
    tabs = np.concatenate([c["kw"]["tab"] for c in R.serve_uniforms_cases()])
    assert {0, 1, 255, 256, 257} <= set(tabs[:, 3]) and {0, 31} <= set(tabs[:, 1]) and (tabs[:, 4:6] < 0).any() and (tabs[:, 2] >= 0).any()


def test_gemv_bound_counts_the_kernels_own_roundings():
    assert [R.gemv_roundings(K) for K in (4, 256, 260, 1024)] == [12, 12, 13, 15]
    assert {c["kw"]["W"].shape for c in R.gemv_cases()} == set(R.GEMV_SHAPES)
    for c in R.gemv_cases():
        kw = c["kw"]
        ref, bound = R.gemv_ref(**kw)
        # the kernel's own order in fp32 passes; a row shifted by one, or a forgotten bias, does not
        W, e = kw["W"], kw["e"]
        N, K = W.shape
        acc = np.zeros((N, 64), f32)
        for c0 in range(0, K, 256):
            for lane in range(min(64, (K - c0) // 4)):
                w, x = W[:, c0 + 4 * lane:c0 + 4 * lane + 4], e[c0 + 4 * lane:c0 + 4 * lane + 4]
                p = (w * x).astype(f32)
                acc[:, lane] += ((p[:, 0] + p[:, 1]).astype(f32) + p[:, 2]).astype(f32) + p[:, 3]
        o = 32
        while o:
            acc = (acc + acc[:, np.arange(64) ^ o]).astype(f32)
            o >>= 1
        y = acc[:, 0] if kw["bias"] is None else (acc[:, 0] + kw["bias"]).astype(f32)
        got = np.concatenate([y, np.full(R.EXTRA, R.SENT_F, f32)])
        assert R.check_bound(got, ref, bound, c["name"]) <= 1.0
        if N > 1:
            with pytest.raises(AssertionError):
                R.check_bound(np.concatenate([np.roll(y, 1), got[N:]]), ref, bound, c["name"])
        if kw["bias"] is not None:
            with pytest.raises(AssertionError):
                R.check_bound(np.concatenate([acc[:, 0], got[N:]]), ref, bound, c["name"])
