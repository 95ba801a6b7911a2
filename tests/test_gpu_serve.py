"""GPU: the serving session (vx_serve_*, Engine.serve, VALLE.serve, AudioServer).

Requests join a running decode batch as soon as enough decode rows are free, each with its own best_of, selection, seed or injected
draws.  Contract: a request returns exactly what a batch-1 vx_infer call on it returns, whatever else is in the session."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from oracle import synth
from oracle.make_golden import RANGE_CASES, UI_CASES, all_cases
from oracle.vallex_oracle import VallexOracle
from tests._util import case_model, case_row, get_model, golden

pytestmark = pytest.mark.gpu

NL, SEED, EOS_GAIN, CAP = 2, 12, 2.5, 36


def _model(max_batch, vocos=False):
    return get_model(NL, SEED, EOS_GAIN, vocos=vocos, max_new=64, max_prompt=128, max_text=64, max_batch=max_batch)


def _rows(n, seed):
    """ragged rows: prompts 0 .. 90 frames, text 1 .. 18 ids, three languages (the test_gpu_fuzz recipe)"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        tp = int(rng.choice([0, 1, 2, int(rng.integers(3, 91))]))
        sp = 0 if tp == 0 else int(rng.integers(1, 13))
        a, t = synth.synth_prompt(tp, sp, seed=int(rng.integers(1, 1 << 30)))
        txt = np.concatenate([t[0], synth.synth_text(int(rng.integers(1, 19)), int(rng.integers(1, 1 << 30)))])
        rows.append(dict(text=txt, prompt=a[0], enroll=sp, prompt_language=("en", "zh", "ja")[int(rng.integers(0, 3))],
                         text_language=("en", "zh", "ja")[int(rng.integers(0, 3))]))
    return rows


def _short(n, seed, lang="en"):
    """short fillers: 2 text ids, no enrolled text -> the reference's cap of 16 x 2 = 32 frames"""
    out = []
    for i in range(n):
        a, _ = synth.synth_prompt(12, 1, seed=seed + i)
        out.append(dict(text=synth.synth_text(2, seed + 100 + i), prompt=a[0], enroll=0, prompt_language=lang,
                        text_language=("en", "zh", "ja")[i % 3]))
    return out


def _serve(sess, m, waves, max_steps=3):
    """submit every wave (rows, request dicts) between vx_serve_run calls of max_steps steps, then run to the end; returns
    ({request id: codes}, [ids per wave], AR steps of the session); m.serve_fallbacks: prefill phases re-run in fp32"""
    got, ids, steps = {}, [], 0
    m.serve_fallbacks = 0

    def done(rid, codes):
        assert rid not in got
        got[rid] = codes

    for rows, reqs in waves:
        ids.append(sess.submit(m.make_batch(rows), reqs))
        live, waiting = sess.run(max_steps, done)
        steps += m.engine.last_stats()["ar_steps"]
        m.serve_fallbacks += m.engine.last_fallbacks()["prefill"]
        assert live + waiting <= sum(len(w) for w in ids)
    live, waiting = sess.run(0, done)
    steps += m.engine.last_stats()["ar_steps"]
    m.serve_fallbacks += m.engine.last_fallbacks()["prefill"]
    assert (live, waiting) == (0, 0)
    return got, ids, steps


def _alone(m, row, req, top_k, force_eos_at):
    """the batch-1 vx_infer call the contract compares against, and its AR steps"""
    out = m.inference_batch([row], top_k=top_k, force_eos_at=force_eos_at, best_of=req.get("best_of", 1),
                            uniforms=req.get("uniforms"), seed=req.get("seed", 0), length_penalty=req.get("length_penalty", 1.0),
                            return_worst=req.get("return_worst", False))[0]
    return out, m.engine.last_stats()["ar_steps"]


def _oracle_req(orc, row, req, top_k, force_eos_at):
    u = np.asarray(req["uniforms"], np.float32)
    u = u.reshape(-1) if req.get("best_of", 1) == 1 else u
    return orc.inference(row["text"][None], np.array([len(row["text"])]), row["prompt"][None], row["enroll"], top_k=top_k,
                         prompt_language=row["prompt_language"], text_language=row["text_language"], uniforms=u,
                         force_eos_at=force_eos_at, best_of=req.get("best_of", 1), length_penalty=req.get("length_penalty", 1.0),
                         return_worst=req.get("return_worst", False))[0]


@pytest.mark.parametrize("max_batch", [4, 8, 32], ids=["sb_chain", "split_fused", "rows32"])
@pytest.mark.parametrize("draws", ["uniforms", "seed"])
def test_waves_of_mixed_requests_equal_batch1_calls(max_batch, draws):
    """three waves of requests with best_of in {1, 3, 5} (clipped to the decode rows), submitted between short vx_serve_run calls,
    some while every decode row is busy: each request equals its batch-1 vx_infer call; injected draws also equal the oracle"""
    m = _model(max_batch)
    nd = min(max_batch, 32)
    n = 9 if max_batch < 32 else 15
    rows = _rows(n, 8100 + max_batch)
    reqs = []
    for i in range(n):
        b = min((1, 3, 5)[i % 3], nd)
        q = dict(best_of=b, length_penalty=(1.0, 0.7)[i % 2], return_worst=i % 4 == 3)
        if draws == "uniforms":
            q["uniforms"] = synth.uniforms(256, b, 8200 + i)
        else:
            q["seed"] = 9_000_000_000 + 17 * i
        reqs.append(q)
    w = n // 3
    waves = [(rows[k * w:(k + 1) * w], reqs[k * w:(k + 1) * w]) for k in range(3)]
    with m.engine.serve(top_k=10, force_eos_at=CAP) as sess:
        got, ids, steps = _serve(sess, m, waves)
    flat = [i for wv in ids for i in wv]
    assert flat == sorted(flat) and len(set(flat)) == n and sorted(got) == flat
    orc = VallexOracle(synth.vallex_state_dict(NL, SEED, EOS_GAIN), NL) if draws == "uniforms" else None
    alone_steps = 0
    lens = []
    for i, rid in enumerate(flat):
        ref, st = _alone(m, rows[i], reqs[i], 10, CAP)
        alone_steps += st
        lens.append(ref.shape[0])
        np.testing.assert_array_equal(got[rid], ref, err_msg=f"request {i} (best_of {reqs[i]['best_of']}): session != batch-1 vx_infer")
        if orc is not None:
            np.testing.assert_array_equal(got[rid], _oracle_req(orc, rows[i], reqs[i], 10, CAP), err_msg=f"request {i} vs the oracle")
    assert len(set(lens)) > 1, lens
    assert steps < alone_steps, (steps, alone_steps)
    print(f"max_batch {max_batch} [{draws}]: lengths {lens}; AR steps session {steps} vs batch-1 calls {alone_steps}")


def _ui_row(c):
    from oracle.make_golden import case_inputs
    a, t, text, pl, langs = case_inputs(c)
    return dict(text=text[0], prompt=a[0], enroll=t.shape[-1], prompt_language=pl, text_language=langs)


def _golden_req(c, us):
    return dict(best_of=c.get("best_of", 1), uniforms=us, length_penalty=c.get("length_penalty", 1.0),
                return_worst=c.get("return_worst", False))


def _assert_golden(name, out, gold):
    assert out.shape == gold.shape, (name, out.shape, gold.shape)
    np.testing.assert_array_equal(out, gold, err_msg=name)


@pytest.mark.parametrize("arith", ["default", "f32"])
def test_live_reference_ui_goldens_admitted_mid_session(arith):
    """the reference UI's request (best_of=5, top_k=-100) and its return_worst twin wait behind six short fillers of five beams
    each (30 of 32 decode rows busy) and enter by admission; ids bit-exact against the live-reference goldens"""
    c = UI_CASES["nl12_ui_bestof5_ja"]
    m = case_model(c, arith=arith, max_new=128, max_prompt=700, max_text=256, max_batch=32)
    fill = _short(6, 91_000, "ja")
    fill_reqs = [dict(best_of=5, uniforms=synth.uniforms(256, 5, 91_500 + i)) for i in range(6)]
    names = ["nl12_ui_bestof5_ja", "nl12_ui_bestof5_ja_worst"]
    gold_rows = [_ui_row(UI_CASES[nm]) for nm in names]
    gold_reqs = [_golden_req(UI_CASES[nm], synth.uniforms(4096, 5, UI_CASES[nm]["useed"])) for nm in names]
    with m.engine.serve(top_k=c["top_k"], temperature=c.get("temperature", 1.0), force_eos_at=c["force_eos_at"]) as sess:
        got, ids, _ = _serve(sess, m, [(fill, fill_reqs), (gold_rows, gold_reqs)], max_steps=2)
    for nm, rid in zip(names, ids[1]):
        _assert_golden(f"{nm} [{arith}] admitted mid-session", got[rid], golden(nm)["codes"][0])


def test_nl2_best_of_goldens_admitted_mid_session():
    c, row, us = case_row("nl2_bestof3")
    cw, roww, usw = case_row("nl2_bestof3_worst")
    m = case_model(c, max_batch=8)
    fill = _short(4, 92_000)
    fill_reqs = [dict(best_of=2 if i % 2 else 1, uniforms=synth.uniforms(128, 2 if i % 2 else 1, 92_500 + i)) for i in range(4)]
    with m.engine.serve(top_k=c["top_k"], force_eos_at=c["force_eos_at"]) as sess:
        got, ids, _ = _serve(sess, m, [(fill, fill_reqs), ([row, roww], [_golden_req(c, us), _golden_req(cw, usw)])], max_steps=2)
    _assert_golden("nl2_bestof3 admitted mid-session", got[ids[1][0]], golden("nl2_bestof3")["codes"][0])
    _assert_golden("nl2_bestof3_worst admitted mid-session", got[ids[1][1]], golden("nl2_bestof3_worst")["codes"][0])


def test_request_is_independent_of_its_co_tenants():
    """the same request with the same seed, alone in a session and submitted into a busy one, returns the same codes"""
    m = _model(8)
    row = _rows(1, 8300)[0]
    req = dict(best_of=3, seed=424242)
    with m.engine.serve(top_k=10, force_eos_at=CAP) as sess:
        alone, ids, _ = _serve(sess, m, [([row], [req])])
        a = alone[ids[0][0]]
    busy_rows = _rows(7, 8301)
    busy_reqs = [dict(best_of=(1, 3)[i % 2], seed=i) for i in range(7)]
    with m.engine.serve(top_k=10, force_eos_at=CAP) as sess:
        got, ids, _ = _serve(sess, m, [(busy_rows[:4], busy_reqs[:4]), ([row] + busy_rows[4:], [req] + busy_reqs[4:])], max_steps=5)
    np.testing.assert_array_equal(got[ids[1][0]], a)
    np.testing.assert_array_equal(a, _alone(m, row, req, 10, CAP)[0])


def test_range_fallback_on_a_beam_admission():
    """out-of-range FFN channels (the same fp32 function as nl2_topk10): the admission rounds leave the fp16 range and are re-run on
    the fp32 kernels.  The golden row (best_of 1, its draws) equals the base golden, the same row with best_of=3 equals the batch-1
    call, and the fillers equal the oracle"""
    name = "nl2_range_ffn"
    base, _ = RANGE_CASES[name]
    c = all_cases()[name]
    _, row, gus = case_row(base)
    m = case_model(c, max_batch=8)
    fill = _short(4, 93_000)
    fill_reqs = [dict(uniforms=synth.uniforms(128, 1, 93_500 + i)) for i in range(4)]
    us3 = np.concatenate([gus[:, None], synth.uniforms(4096, 2, 93_900)], axis=1)
    reqs = [dict(uniforms=gus), dict(best_of=3, uniforms=us3)]
    with m.engine.serve(top_k=c["top_k"], force_eos_at=c["force_eos_at"]) as sess:
        got, ids, _ = _serve(sess, m, [(fill, fill_reqs), ([row, row], reqs)], max_steps=2)
    assert m.serve_fallbacks >= 2, m.serve_fallbacks        # the first admission round and (at least) the golden rows' round
    _assert_golden(f"{name} admitted mid-session", got[ids[1][0]], golden(base)["codes"][0])
    np.testing.assert_array_equal(got[ids[1][1]], _alone(m, row, reqs[1], c["top_k"], c["force_eos_at"])[0])
    orc = VallexOracle(synth.vallex_state_dict(c["num_layers"], c["seed"], c["eos_gain"]), c["num_layers"])
    for i in range(4):
        np.testing.assert_array_equal(got[ids[0][i]], _oracle_req(orc, fill[i], fill_reqs[i], c["top_k"], c["force_eos_at"]),
                                      err_msg=f"filler {i}")


def test_context_exclusivity_and_side_paths():
    from vallex_amd._capi import VX_EINVAL, VallexHipError, vx_request, _ptr
    m = _model(4, vocos=True)
    eng = m.engine
    rows = _rows(5, 8400)
    reqs = [dict(best_of=(1, 3)[i % 2], seed=100 + i) for i in range(5)]
    refs = [_alone(m, r, q, 10, CAP)[0] for r, q in zip(rows, reqs)]
    codes = [np.random.default_rng(5).integers(0, 1024, size=(40, 8)).astype(np.int64)]
    wav_before = eng.vocos_decode(codes)[0].copy()
    sess = eng.serve(top_k=10, force_eos_at=CAP)
    try:
        with pytest.raises(VallexHipError) as ei:
            m.inference_batch(rows[:1], top_k=10, seed=1, force_eos_at=CAP)
        assert ei.value.code == VX_EINVAL and "serving session" in str(ei.value)
        with pytest.raises(VallexHipError):
            eng.nar(m.make_batch(rows[:1]), [np.zeros(4, np.int32)])
        got = {}
        ids = sess.submit(m.make_batch(rows), reqs)
        sess.run(3, lambda rid, c: got.__setitem__(rid, c))
        # the vocoder between two runs leaves the decoding requests alone
        np.testing.assert_array_equal(eng.vocos_decode(codes)[0], wav_before)

        # refusals at submit: nothing of the call is enqueued, the session goes on
        def raw(row, **kw):
            r = vx_request()
            r.struct_size = C.sizeof(vx_request)
            r.best_of = kw.get("best_of", 1)
            r.length_penalty = 1.0
            keep = kw.get("uniforms")
            if keep is not None:
                r.uniforms = _ptr(keep, C.c_float)
                r.uniforms_steps = keep.shape[0]
            b = m.make_batch([row])
            out = np.zeros(1, np.int64)
            rc = eng.lib.vx_serve_submit(sess.h, C.byref(b.c), C.byref(r), _ptr(out, C.c_int64))
            return rc, eng.lib.vx_last_error(eng.ctx).decode()

        rc, msg = raw(rows[0], best_of=5)
        assert rc == VX_EINVAL and "best_of" in msg, msg
        big = dict(rows[0], prompt=np.zeros((129, 8), np.int32))
        rc, msg = raw(big)
        assert rc == VX_EINVAL and "prompt" in msg, msg
        rc, msg = raw(rows[0], uniforms=np.full((5, 1), 0.5, np.float32))
        assert rc == VX_EINVAL and "uniforms" in msg, msg
        sess.run(0, lambda rid, c: got.__setitem__(rid, c))
        assert sorted(got) == ids
        for i, rid in enumerate(ids):
            np.testing.assert_array_equal(got[rid], refs[i], err_msg=f"request {i}")
    finally:
        sess.close()
    # usable for vx_infer again
    np.testing.assert_array_equal(m.inference_batch(rows[:1], top_k=10, seed=100, force_eos_at=CAP)[0], refs[0])


def test_python_server_threads_callbacks_and_drain():
    m = _model(8)
    rows = _rows(10, 8500)
    reqs = [dict(best_of=(1, 3, 5)[i % 3], seed=7_000 + i) for i in range(10)]
    refs = [_alone(m, r, q, 10, CAP)[0] for r, q in zip(rows, reqs)]
    # an exception in a done callback reaches the caller of run(), the other requests are still delivered
    with m.engine.serve(top_k=10, force_eos_at=CAP) as sess:
        ids = sess.submit(m.make_batch(rows[:3]), reqs[:3])

        class Boom(RuntimeError):
            pass

        seen = []

        def bad(rid, codes):
            seen.append(rid)
            if rid == ids[1]:
                raise Boom("request 1")

        with pytest.raises(Boom):
            sess.run(0, bad)
    # two submitting threads while the worker runs; every future resolves to the batch-1 result
    futs = [None] * 10
    with m.serve(top_k=10, force_eos_at=CAP, max_steps=4) as srv:
        def client(k):
            for i in range(k, 10, 2):
                futs[i] = srv.submit(rows[i], **reqs[i])

        th = [threading.Thread(target=client, args=(k,)) for k in (0, 1)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    # close() drained: every future is done without waiting
    assert all(f.done() for f in futs)
    for i, f in enumerate(futs):
        np.testing.assert_array_equal(f.result(), refs[i], err_msg=f"request {i}")
    with pytest.raises(ValueError, match="best_of"):
        m.serve(best_of=5)
    with m.serve(top_k=10) as srv:
        with pytest.raises(ValueError, match="best_of"):
            srv.submit(rows[0], best_of=0)


def test_audio_server_equals_vocos_of_the_same_codes():
    from vallex_amd.utils import generation as G
    G.preload_models(state_dict=synth.vallex_state_dict(2, 11), vocos_state_dict=synth.vocos_state_dict(2), num_layers=2, max_new=320,
                     max_prompt=400, max_text=256, max_batch=8)
    pdir = os.path.join(os.path.dirname(__file__), "golden", "presets")
    texts = [synth.synth_text(12, 61), synth.synth_text(7, 62), synth.synth_text(15, 63)]
    prompts = [os.path.join(pdir, "paimon.npz"), None, os.path.join(pdir, "cafe.npz")]
    langs = ["en", "zh", "ja"]
    kw = [dict(best_of=3, seed=11), dict(best_of=1, seed=12), dict(best_of=5, seed=13)]
    want = [G.generate_audio_batch([t], prompts=[p], language=[lg], force_eos_at=20, **k)[0] for t, p, lg, k in zip(texts, prompts, langs, kw)]
    with G.AudioServer(force_eos_at=20) as srv:
        futs = [srv.submit(t, prompt=p, language=lg, **k) for t, p, lg, k in zip(texts, prompts, langs, kw)]
        wavs = [f.result() for f in futs]
    for i in range(3):
        assert wavs[i].dtype == np.float32 and len(wavs[i]) % 320 == 0
        np.testing.assert_array_equal(wavs[i], want[i], err_msg=f"utterance {i}")
