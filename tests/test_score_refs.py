"""CPU: the references of the teacher-forced scoring tests (tests/_score_refs.py) against what the suite already pins -- the cached
AR chain of the oracle, the goldens of the live reference, the oracle's own sum(logp) -- and the C prototypes of vx_score /
vx_dev_score_rows against the ctypes binding.  Tolerances: fp32 reassociation of one full-sequence pass against the cached steps
(measured 1.4e-6, bound 5e-6), fp32 against float64 (measured 1.5e-6 AR, 5.8e-5 NAR at |logit| <= 97; bounds 1e-5, 5e-4)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import synth
from oracle.vallex_oracle import VallexOracle
from tests._score_refs import ar_logits_stepwise, ar_logits_tf, lse_bound, nar_logits_tf, oracle64, score_ref
from tests._util import case_row, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nl2_greedy_eos", "nl2_topk10"]
_CACHE = {}


def _refs(name):
    """fp32 and float64 teacher-forced logits of a golden's own codes, computed once per case"""
    if name not in _CACHE:
        c, row, _ = case_row(name)
        sd = synth.vallex_state_dict(c["num_layers"], c["seed"], c["eos_gain"])
        codes = golden(name)["codes"][0]
        o32, o64 = VallexOracle(sd, c["num_layers"]), oracle64(sd, c["num_layers"])
        with torch.no_grad():
            _CACHE[name] = dict(row=row, codes=codes, o32=o32, ar32=ar_logits_tf(o32, row, codes[:, 0]).numpy(),
                                ar64=ar_logits_tf(o64, row, codes[:, 0]).numpy(),
                                nar32=[l.numpy() for l in nar_logits_tf(o32, row, codes)],
                                nar64=[l.numpy() for l in nar_logits_tf(o64, row, codes)])
    return _CACHE[name]


@pytest.mark.parametrize("name", NAMES)
def test_ar_full_sequence_pass_equals_cached_chain_and_golden(name):
    r = _refs(name)
    with torch.no_grad():
        step = ar_logits_stepwise(r["o32"], r["row"], r["codes"][:, 0]).numpy()
    assert r["ar32"].shape == step.shape == (len(r["codes"]) + 1, 1025)
    d = float(np.abs(r["ar32"] - step).max())
    print(name, "full-sequence pass vs cached chain", d)
    assert d <= 5e-6
    g = golden(name)["ar_logits"]
    n = min(len(g), len(step))
    dg = float(np.abs(r["ar32"][:n] - g[:n]).max())
    print(name, "full-sequence pass vs live reference", dg)
    assert n > 0 and dg <= 5e-6


@pytest.mark.parametrize("name", NAMES)
def test_nar_teacher_forced_reproduces_golden(name):
    r = _refs(name)
    for st in range(7):
        np.testing.assert_array_equal(r["nar32"][st].argmax(axis=1), r["codes"][:, st + 1])
    d = float(np.abs(r["nar32"][0][:16] - golden(name)["nar_logits0"]).max())
    print(name, "nar_logits0 vs live reference", d)
    assert d <= 5e-4


@pytest.mark.parametrize("name", NAMES)
def test_fp32_and_float64_oracles_agree(name):
    r = _refs(name)
    assert r["ar64"].dtype == np.float64 and r["nar64"][0].dtype == np.float64
    da = float(np.abs(r["ar32"] - r["ar64"]).max())
    dn = max(float(np.abs(a - b).max()) for a, b in zip(r["nar32"], r["nar64"]))
    print(name, "fp32 vs float64: AR", da, "NAR", dn, "max |NAR logit|", max(float(np.abs(b).max()) for b in r["nar64"]))
    assert da <= 1e-5 and dn <= 5e-4


@pytest.mark.parametrize("name,force", [("nl2_greedy_eos", None), ("nl2_topk10", 24)])
def test_score_ref_sums_to_the_samplers_sum_logp(name, force):
    """sum_t logp[t] + eos_logp == the sum(logp) the oracle's sampler accumulates (models/vallex.py:572) for an unfiltered sampled run
    that ends in a SAMPLED EOS (force == None), or -- forced EOS at the end -- up to the term of the forced step, which the sampler
    takes at the token it drew there and the score at EOS: that step's own logp is exchanged before comparing"""
    c, row, _ = case_row(name)
    sd = synth.vallex_state_dict(c["num_layers"], c["seed"], c["eos_gain"])
    o = VallexOracle(sd, c["num_layers"])
    us = synth.uniforms(4096, 1, 77)[:, 0]
    text, p0 = torch.from_numpy(row["text"].astype(np.int64)), torch.from_numpy(row["prompt"][:, 0].astype(np.int64))
    with torch.no_grad():
        taps = {}
        gen, slp = o.ar_generate(text, p0, row["enroll"], row["prompt_language"], row["text_language"], top_k=-100, uniforms=us,
                                 force_eos_at=force, taps=taps, return_logp=True)
        lg = ar_logits_tf(o, row, np.array(gen, np.int64)).numpy()
    assert len(gen) >= 4 and len(gen) < 16 * len(row["text"])
    logp, _, _ = score_ref(lg, np.array(gen + [synth.EOS_ID]))
    total = float(logp.sum())
    if force is not None:
        assert len(gen) == force
        last = taps["ar_logits"][-1].double().reshape(1, -1)
        drawn, _ = o.sample(taps["ar_logits"][-1], -100, 1.0, float(us[force]))
        total += float(torch.log_softmax(last, -1)[0, drawn]) - float(logp[-1])
    print(name, "sum of score_ref", total, "sampler", slp)
    assert abs(total - slp) <= 1e-4


def test_lse_bound_and_score_ref_on_a_known_row():
    l = np.zeros((2, 1025))
    l[1, 7] = 30.0
    logp, rank, n_near = score_ref(l, [3, 8])
    np.testing.assert_allclose(logp, [-np.log(1025.0), -30.0 - np.log1p(1024 * np.exp(-30.0))], rtol=1e-12)
    assert rank.tolist() == [0, 1] and n_near(1e-3).tolist() == [1024, 1023]
    np.testing.assert_allclose(lse_bound(l, [3, 8]), [4e-5, 4e-5 + 30 * 2.0 ** -22])


def test_score_prototypes_match_binding():
    """the header prototypes of vx_score / vx_dev_score_rows and the ctypes argtypes agree in count and kind; VX_SCORE_* too"""
    import ctypes as C

    import __graft_entry__ as g
    g.build()
    import vallex_amd
    from vallex_amd import _capi
    lib = vallex_amd.load_library()
    P = C.POINTER
    kinds = {"vx_ctx*": C.c_void_p, "const vx_batch*": P(_capi.vx_batch), "int32_t": C.c_int32, "const int32_t*": P(C.c_int32),
             "int32_t*": P(C.c_int32), "float*": P(C.c_float), "const float*": P(C.c_float), "const int64_t*": P(C.c_int64)}
    want = {("vallex_hip.h", "vx_score"): 11, ("vallex_hip_dev.h", "vx_dev_score_rows"): 9}
    for (header, name), nargs in want.items():
        hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        proto = re.search(r"\bint %s\((.*?)\);" % name, hdr, re.S).group(1)
        args = [" ".join(a.split()).rsplit(" ", 1)[0] for a in proto.split(",")]
        fn = getattr(lib, name)
        assert len(args) == nargs and fn.restype is C.c_int
        assert list(fn.argtypes) == [kinds[a] for a in args], (name, args)
        if name == "vx_score":
            assert int(re.search(r"#define VX_SCORE_AR (\d+)", hdr).group(1)) == _capi.SCORE_AR == 1
            assert int(re.search(r"#define VX_SCORE_NAR (\d+)", hdr).group(1)) == _capi.SCORE_NAR == 2
    assert "vx_score" in _capi.SYMBOLS and "vx_dev_score_rows" in _capi.DEV_SYMBOLS
