"""GPU: per-request sampling (vx_serve_submit_ex) and cancellation (vx_serve_cancel) in the serving session.

Contract: a request submitted with (top_k, temperature, force_eos_at) returns exactly what a batch-1 vx_infer call with those
vx_sampling values and the request's best_of / selection / seed or draws returns, whatever else is in the session; cancelling a
request never changes what another one returns."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

from oracle import synth
from oracle.make_golden import all_cases, case_inputs
from tests._util import case_model, get_model, golden

pytestmark = pytest.mark.gpu

NL, SEED = 2, 12


def _model(max_batch, eos_gain=2.5, max_new=64):
    return get_model(NL, SEED, eos_gain, max_new=max_new, max_prompt=128, max_text=64, max_batch=max_batch)


def _until(cond, timeout=60.0):
    t0 = time.perf_counter()
    while not cond():
        assert time.perf_counter() - t0 < timeout, "timed out"
        time.sleep(0.0005)


def _record_cancels(monkeypatch):
    """every ServeSession.cancel call the Server's worker makes: [(request id, state)]"""
    from vallex_amd._capi import ServeSession
    calls, orig = [], ServeSession.cancel

    def rec(self, rid):
        st = orig(self, rid)
        calls.append((rid, st))
        return st

    monkeypatch.setattr(ServeSession, "cancel", rec)
    return calls


def _rows(n, seed):
    """ragged rows: prompts 0 .. 90 frames, text 1 .. 18 ids, three languages"""
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


def _truncated(m):
    cut = C.c_int32()
    m.engine._chk(m.engine.lib.vx_last_truncated(m.engine.ctx, C.byref(cut)))
    return cut.value


def _serve(sess, m, waves, max_steps=3):
    """submit every wave (rows, request dicts) between vx_serve_run calls of max_steps steps, then run to the end; returns
    ({request id: codes}, [ids per wave], AR steps, truncated rows reported by the runs)"""
    got, ids, steps, cut = {}, [], 0, 0

    def done(rid, codes):
        assert rid not in got
        got[rid] = codes

    for rows, reqs in waves:
        ids.append(sess.submit(m.make_batch(rows), reqs))
        sess.run(max_steps, done)
        steps += m.engine.last_stats()["ar_steps"]
        cut += _truncated(m)
    assert sess.run(0, done) == (0, 0)
    steps += m.engine.last_stats()["ar_steps"]
    cut += _truncated(m)
    return got, ids, steps, cut


def _alone(m, row, q):
    """the batch-1 vx_infer call the contract compares against (the request's own sampling; unset: the defaults of the sessions
    below, top_k -100, temperature 1, no forced EOS), and its truncation count"""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # arena cuts are compared explicitly
        out = m.inference_batch([row], top_k=q.get("top_k", -100), temperature=q.get("temperature", 1.0),
                                force_eos_at=q.get("force_eos_at", -1),
                                best_of=q.get("best_of", 1), uniforms=q.get("uniforms"), seed=q.get("seed", 0),
                                length_penalty=q.get("length_penalty", 1.0), return_worst=q.get("return_worst", False))[0]
    return out, _truncated(m)


# ---- 1. live-reference goldens with different sampling in one session ----------------------------------------------------

def _case_req(name):
    c = all_cases()[name]
    a, t, text, pl, langs = case_inputs(c)
    row = dict(text=text[0], prompt=a[0], enroll=t.shape[-1], prompt_language=pl, text_language=langs)
    q = dict(top_k=c["top_k"], temperature=c.get("temperature", 1.0),
             force_eos_at=-1 if c["force_eos_at"] is None else c["force_eos_at"])
    if c["useed"] is not None:
        q["uniforms"] = synth.uniforms(4096, 1, c["useed"])[:, 0]
    return c, row, q


def _goldens_in_one_session(names, m, defaults, max_steps=3):
    reqs = [_case_req(n) for n in names]
    half = (len(names) + 1) // 2
    waves = [([r for _, r, _ in reqs[:half]], [q for _, _, q in reqs[:half]]),
             ([r for _, r, _ in reqs[half:]], [q for _, _, q in reqs[half:]])]
    with m.engine.serve(**defaults) as sess:
        got, ids, _, _ = _serve(sess, m, waves, max_steps=max_steps)
    flat = [i for w in ids for i in w]
    for n, rid in zip(names, flat):
        gold = golden(n)["codes"][0]
        out = got[rid]
        assert out.shape == gold.shape, (n, out.shape, gold.shape)
        d = np.argwhere(out != gold)
        assert not len(d), f"{n}: {len(d)} ids differ from the live-reference golden, first at {tuple(d[0])}"


@pytest.mark.parametrize("arith", ["default", "f32"])
def test_full_length_goldens_with_their_own_sampling(arith):
    """the six 600-frame live-reference rows (greedy and top-k 10, three languages) in ONE session opened with other defaults"""
    names = ["nl12_full_en_greedy", "nl12_full_zh_greedy", "nl12_full_ja_greedy", "nl12_full_en_topk10", "nl12_full_zh_topk10",
             "nl12_full_ja_topk10"]
    m = case_model(all_cases()[names[0]], arith=arith, max_new=608, max_prompt=400, max_text=256, max_batch=8)
    _goldens_in_one_session(names, m, dict(top_k=50, temperature=0.7, force_eos_at=3))


def test_nl2_goldens_with_their_own_sampling():
    # multinomial at T 0.8 forced at 32, and top-k 10 at T 1 forced at 40 on a 1125-frame prompt (seed 4)
    names = ["nl2_full_multinomial", "nl2_max_prompt"]
    m = case_model(all_cases()[names[0]], max_new=64, max_prompt=1160, max_text=256, max_batch=4)
    _goldens_in_one_session(names, m, dict(top_k=1, temperature=1.3, force_eos_at=-1), max_steps=2)
    # top-k 10 forced at 48 and greedy forced at 5 (seed 3)
    names = ["nl2_topk10", "nl2_minimal"]
    m = case_model(all_cases()[names[0]], max_new=64, max_prompt=400, max_text=256, max_batch=4)
    _goldens_in_one_session(names, m, dict(top_k=-100, temperature=0.6, force_eos_at=2), max_steps=2)


# ---- 2. random mixed load ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_batch", [4, 8, 32], ids=["sb_chain", "split_fused", "rows32"])
def test_random_mixed_sampling_equals_batch1_calls(max_batch):
    """24 ragged requests in four waves, each with its own top_k, temperature, force_eos_at, best_of and seed or draws: every
    request equals its batch-1 vx_infer call, and the session reports the arena cuts the batch-1 calls report"""
    m = _model(max_batch)
    nd = min(max_batch, 32)
    n = 24
    rows = _rows(n, 9100 + max_batch)
    rng = np.random.default_rng(9200 + max_batch)
    reqs = []
    for i in range(n):
        b = min(int(rng.choice([1, 3, 5])), nd)
        q = dict(best_of=b, top_k=int(rng.choice([-100, 1, 2, 10, 50])), temperature=float(rng.choice([0.6, 1.0, 1.7])),
                 force_eos_at=int(rng.choice([-1, 0, 7, 30])), length_penalty=(1.0, 0.7)[i % 2], return_worst=i % 5 == 4)
        if i % 2:
            q["uniforms"] = synth.uniforms(128, b, 9300 + i)
        else:
            q["seed"] = 5_000_000_000 + 31 * i
        reqs.append(q)
    waves = [(rows[k * 6:(k + 1) * 6], reqs[k * 6:(k + 1) * 6]) for k in range(4)]
    with m.engine.serve(top_k=3, temperature=1.1, force_eos_at=12) as sess:
        got, ids, steps, cut = _serve(sess, m, waves)
    flat = [i for w in ids for i in w]
    assert sorted(got) == flat
    cut_alone, lens = 0, []
    for i, rid in enumerate(flat):
        ref, c1 = _alone(m, rows[i], reqs[i])
        cut_alone += c1
        lens.append(ref.shape[0])
        np.testing.assert_array_equal(got[rid], ref, err_msg=f"request {i} ({reqs[i]}): session != batch-1 vx_infer")
        if reqs[i]["force_eos_at"] >= 0:
            assert ref.shape[0] <= reqs[i]["force_eos_at"]
    assert cut == cut_alone, (cut, cut_alone)
    assert len(set(lens)) > 3, lens
    print(f"max_batch {max_batch}: lengths {lens}, AR steps {steps}, arena cuts {cut}")


# ---- 3. defaults ------------------------------------------------------------------------------------------------------------

def test_submit_ex_with_the_sessions_values_equals_submit():
    from vallex_amd._capi import _ptr, vx_request
    m = _model(8)
    rows = _rows(7, 9400)
    reqs = [dict(best_of=(1, 3)[i % 2], seed=77 + i) if i % 3 else dict(best_of=1, uniforms=synth.uniforms(128, 1, 9500 + i))
            for i in range(7)]
    opts = dict(top_k=10, temperature=0.8, force_eos_at=20)
    outs = []
    for mode in ("submit", "submit_ex", "submit_ex_null"):
        with m.engine.serve(**opts) as sess:
            got = {}
            if mode == "submit":
                ids = sess.submit(m.make_batch(rows), reqs)
            elif mode == "submit_ex":
                ids = sess.submit(m.make_batch(rows), [dict(q, **opts) for q in reqs])
            else:                                       # smp = NULL: the session's values
                b = m.make_batch(rows)
                arr = (vx_request * len(rows))()
                keep = []
                for i, q in enumerate(reqs):
                    arr[i].struct_size = C.sizeof(vx_request)
                    arr[i].best_of = q["best_of"]
                    arr[i].length_penalty = 1.0
                    arr[i].seed = q.get("seed", 0)
                    if "uniforms" in q:
                        u = np.ascontiguousarray(q["uniforms"], np.float32)
                        keep.append(u)
                        arr[i].uniforms = _ptr(u, C.c_float)
                        arr[i].uniforms_steps = u.shape[0]
                out = np.zeros(len(rows), np.int64)
                m.engine._chk(m.engine.lib.vx_serve_submit_ex(sess.h, C.byref(b.c), arr, None, _ptr(out, C.c_int64)))
                ids = [int(x) for x in out]
            assert sess.run(0, lambda rid, c: got.__setitem__(rid, c)) == (0, 0)
            outs.append([got[i] for i in ids])
    for i in range(len(rows)):
        np.testing.assert_array_equal(outs[1][i], outs[0][i], err_msg=f"request {i}: submit_ex(session values) != submit")
        np.testing.assert_array_equal(outs[2][i], outs[0][i], err_msg=f"request {i}: submit_ex(NULL) != submit")


def test_submit_ex_refusals_enqueue_nothing():
    from vallex_amd._capi import VX_EINVAL, _ptr, vx_request, vx_request_sampling
    m = _model(4)
    row = _rows(1, 9600)[0]
    b = m.make_batch([row, row])
    with m.engine.serve(top_k=10, force_eos_at=30) as sess:
        def raw(smp_vals, uniforms=None, size=C.sizeof(vx_request_sampling)):
            arr = (vx_request * 2)()
            smp = (vx_request_sampling * 2)()
            for i in range(2):
                arr[i].struct_size = C.sizeof(vx_request)
                arr[i].best_of = 1
                arr[i].length_penalty = 1.0
                if uniforms is not None:
                    arr[i].uniforms = _ptr(uniforms, C.c_float)
                    arr[i].uniforms_steps = uniforms.shape[0]
                smp[i].struct_size = size
                smp[i].top_k, smp[i].temperature, smp[i].force_eos_at = smp_vals[i]
            out = np.full(2, -7, np.int64)
            rc = m.engine.lib.vx_serve_submit_ex(sess.h, C.byref(b.c), arr, smp, _ptr(out, C.c_int64))
            return rc, m.engine.lib.vx_last_error(m.engine.ctx).decode(), out

        ok = (10, 1.0, 5)
        for bad, word in (((10, 0.0, 5), "temperature"), ((10, float("nan"), 5), "temperature"), ((10, float("inf"), 5), "temperature"),
                          ((10, 1.0, -2), "force_eos_at")):
            rc, msg, out = raw([ok, bad])
            assert rc == VX_EINVAL and word in msg, msg
            assert list(out) == [-7, -7]
        rc, msg, _ = raw([ok, ok], size=12)
        assert rc == VX_EINVAL and "struct_size" in msg, msg
        # draws for the request's own cap: force_eos_at 5 needs 6, force_eos_at -1 needs min(16 S, max_new) + 1
        u6 = np.full((6, 1), 0.5, np.float32)
        rc, msg, _ = raw([ok, (10, 1.0, -1)], uniforms=u6)
        assert rc == VX_EINVAL and "uniforms" in msg, msg
        rc, msg, out = raw([ok, ok], uniforms=u6)
        assert rc == 0 and list(out) == [0, 1], msg
        got = {}
        assert sess.run(0, lambda rid, c: got.__setitem__(rid, c)) == (0, 0)
        assert sorted(got) == [0, 1] and all(c.shape[0] <= 5 for c in got.values())


# ---- 4. distribution of the counter-RNG path ---------------------------------------------------------------------------------

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


@pytest.mark.parametrize("top_k,temperature", [(10, 0.7), (50, 1.5)])
def test_first_token_distribution_of_the_counter_rng(top_k, temperature):
    """3000 requests with distinct seeds sample the first token of one fixed row: its histogram against the float64 top-k filtered
    softmax of the prefill logits (vx_ar_logits), chi-square with bins merged to >= 5 expected"""
    m = _model(32, eos_gain=1.0, max_new=8)
    row = _rows(1, 9700)[0]
    m.engine.ar_prefill(m.make_batch([row]))
    lg = m.engine.ar_logits()[0].astype(np.float64) / temperature
    kth = np.sort(lg)[::-1][top_k - 1]
    z = np.where(lg >= kth, lg, -np.inf)
    p = np.exp(z - z.max())
    p /= p.sum()
    n = 3000
    counts = np.zeros(1025, np.int64)
    with m.engine.serve(top_k=1, temperature=1.0, force_eos_at=-1) as sess:
        got = {}
        for w in range(0, n, 500):
            k = min(500, n - w)
            sess.submit(m.make_batch([row] * k), [dict(seed=1_000_003 * (w + i) + 17, top_k=top_k, temperature=temperature,
                                                       force_eos_at=1) for i in range(k)])
            assert sess.run(0, lambda rid, c: got.__setitem__(rid, c)) == (0, 0)
    assert len(got) == n
    for c in got.values():
        assert c.shape[0] <= 1
        counts[int(c[0, 0]) if c.shape[0] else 1024] += 1
    assert counts[p == 0].sum() == 0, "a token outside the top-k filter was drawn"
    pv, bins, stat = _chi2_pvalue(counts, p, n)
    print(f"top_k {top_k} T {temperature}: chi2 {stat:.1f} over {bins} bins, p = {pv:.4f}; max p {p.max():.3f}")
    assert bins >= 3, bins
    assert pv > 1e-4, (pv, stat, bins)


# ---- 5. cancellation -------------------------------------------------------------------------------------------------------

def _lengths(m, row, cols, top_k, temperature):
    """frames of a best_of=1 request with each injected draw column: the length of the beam that draws that column"""
    with m.engine.serve(top_k=top_k, temperature=temperature) as sess:
        got = {}
        ids = sess.submit(m.make_batch([row] * len(cols)), [dict(uniforms=u) for u in cols])
        assert sess.run(0, lambda rid, c: got.__setitem__(rid, c)) == (0, 0)
    return [got[i].shape[0] for i in ids]


def _cancel_schedule(m, x, y, cancel_at, cancel):
    """X (best_of 3) is admitted, Y (best_of 2) is submitted behind it; after cancel_at decode steps X is cancelled (or not, the
    control); returns (cancel state, {id: codes}, total AR steps, ids)"""
    got, steps = {}, 0

    def done(rid, c):
        got[rid] = c

    with m.engine.serve(top_k=-100) as sess:
        ix = sess.submit(m.make_batch([x[0]]), [x[1]])[0]
        iy = sess.submit(m.make_batch([y[0]]), [y[1]])[0]
        live, waiting = sess.run(cancel_at, done)
        steps += m.engine.last_stats()["ar_steps"]
        state = sess.cancel(ix) if cancel else None
        assert sess.run(0, done) == (0, 0)
        steps += m.engine.last_stats()["ar_steps"]
        if cancel:
            assert sess.cancel(ix) is None and sess.cancel(iy) is None and sess.cancel(10 ** 9) is None
    return state, got, steps, (ix, iy), (live, waiting)


def test_cancel_waiting_and_decoding_requests():
    m = _model(4)
    rows = _rows(6, 9800)
    # draw columns of one row by the length of the beam that draws them (top_k -100, T 1): the five longest and the shortest
    cols = [synth.uniforms(128, 1, 9900 + i) for i in range(48)]
    x_row = max(rows, key=lambda r: len(r["text"]))
    lens = _lengths(m, x_row, cols, -100, 1.0)
    by_len = sorted(range(len(cols)), key=lambda i: -lens[i])
    longs, short = by_len[:5], by_len[-1]
    assert lens[longs[4]] >= 8 and lens[short] + 6 <= lens[longs[4]], lens
    y = (rows[0], dict(best_of=2, seed=4242, top_k=10, temperature=1.0, force_eos_at=4))
    y_ref, _ = _alone(m, y[0], y[1])

    # a decoding best_of=3 request (no beam stopped yet) with a best_of=2 request waiting behind it
    ux = np.concatenate([cols[i] for i in longs[:3]], axis=1)
    x = (x_row, dict(best_of=3, uniforms=ux, top_k=-100, temperature=1.0, force_eos_at=-1))
    st, got, steps, (ix, iy), lw = _cancel_schedule(m, x, y, 3, True)
    assert lw == (1, 1) and st == "decoding", (lw, st)
    assert sorted(got) == [iy]
    np.testing.assert_array_equal(got[iy], y_ref)
    st0, got0, steps0, _, _ = _cancel_schedule(m, x, y, 3, False)
    assert sorted(got0) == [ix, iy] and got0[ix].shape[0] >= 8
    np.testing.assert_array_equal(got0[iy], y_ref)
    np.testing.assert_array_equal(got0[ix], _alone(m, x[0], x[1])[0])
    assert steps < steps0, (steps, steps0)

    # the same when one of its beams has already stopped (and been harvested by the run's last poll)
    s = lens[short]
    ux = np.concatenate([cols[short]] + [cols[i] for i in longs[3:5]], axis=1)
    x = (x_row, dict(best_of=3, uniforms=ux, top_k=-100, temperature=1.0, force_eos_at=-1))
    st, got, steps, (ix, iy), _ = _cancel_schedule(m, x, y, s + 1, True)
    assert st == "decoding"
    assert sorted(got) == [iy]
    np.testing.assert_array_equal(got[iy], y_ref)
    _, got0, steps0, _, _ = _cancel_schedule(m, x, y, s + 1, False)
    np.testing.assert_array_equal(got0[iy], y_ref)
    assert steps < steps0, (steps, steps0)

    # a waiting request: removed, never delivered; the rows of a cancelled request serve the next admission exactly
    later = [dict(best_of=(1, 3)[i % 2], seed=600 + i, top_k=(1, 10, -100)[i % 3], temperature=(0.6, 1.7)[i % 2],
                  force_eos_at=(7, -1, 30)[i % 3]) for i in range(4)]
    later_refs = [_alone(m, rows[2 + i], later[i])[0] for i in range(4)]
    with m.engine.serve(top_k=-100) as sess:
        got = {}
        i_long = sess.submit(m.make_batch([x_row]), [dict(best_of=4, uniforms=np.concatenate([cols[i] for i in longs[:4]], axis=1))])[0]
        i_wait = sess.submit(m.make_batch([rows[1]]), [dict(seed=5, top_k=2)])[0]
        assert sess.run(2, lambda rid, c: got.__setitem__(rid, c)) == (1, 1)
        assert sess.cancel(i_wait) == "waiting"
        assert sess.cancel(i_wait) is None
        assert sess.cancel(i_long) == "decoding"
        ids = sess.submit(m.make_batch(rows[2:6]), later)
        assert sess.run(0, lambda rid, c: got.__setitem__(rid, c)) == (0, 0)
        assert sorted(got) == ids
        for i, rid in enumerate(ids):
            np.testing.assert_array_equal(got[rid], later_refs[i], err_msg=f"request {i} after the cancel")
        assert sess.cancel(ids[0]) is None                   # delivered
        # everything cancelled: nothing left to run
        a, b = sess.submit(m.make_batch([x_row, rows[0]]), [dict(best_of=3, uniforms=np.concatenate([cols[i] for i in longs[:3]], axis=1)),
                                                            dict(best_of=2, seed=2)])
        sess.run(1, lambda rid, c: got.__setitem__(rid, c))
        assert sess.cancel(a) == "decoding" and sess.cancel(b) in ("waiting", "decoding")
        n_before = len(got)
        assert sess.run(0, lambda rid, c: got.__setitem__(rid, c)) == (0, 0)
        assert m.engine.last_stats()["ar_steps"] == 0 and len(got) == n_before


def test_cancel_from_on_done_is_refused():
    from vallex_amd._capi import VX_EINVAL, VallexHipError
    m = _model(8)
    rows = _rows(4, 9850)
    reqs = [dict(seed=i, top_k=(1, 10)[i % 2], temperature=(1.0, 0.6)[i % 2], force_eos_at=(3, 6, 9, 12)[i]) for i in range(4)]
    refs = [_alone(m, r, q)[0] for r, q in zip(rows, reqs)]
    errors, got = [], {}
    with m.engine.serve(top_k=-100) as sess:
        ids = sess.submit(m.make_batch(rows), reqs)

        def done(rid, c):
            got[rid] = c
            try:
                sess.cancel(ids[-1])
            except VallexHipError as e:
                errors.append(e)

        assert sess.run(0, done) == (0, 0)
    assert len(errors) == 4 and all(e.code == VX_EINVAL for e in errors)
    assert sorted(got) == ids
    for i, rid in enumerate(ids):
        np.testing.assert_array_equal(got[rid], refs[i])


def test_server_futures_cancel_until_delivered(monkeypatch):
    # eos_gain 0: no beam emits EOS, the long request (60 text ids) decodes for 16 x 60 = 960 steps unless it is cancelled
    m = _model(4, eos_gain=0.0, max_new=1024)
    rows = _rows(4, 9870)
    long_row = dict(rows[3], text=np.concatenate([rows[3]["text"][:rows[3]["enroll"]], synth.synth_text(60 - rows[3]["enroll"], 9871)]))
    others = rows[:3]
    oreq = [dict(seed=10 + i, top_k=(1, 10, -100)[i], temperature=(1.0, 0.6, 1.7)[i], force_eos_at=(4, 8, 12)[i]) for i in range(3)]
    refs = [_alone(m, r, q)[0] for r, q in zip(others, oreq)]
    calls = _record_cancels(monkeypatch)
    with m.serve(top_k=-100, max_steps=1) as srv:
        f_long = srv.submit(long_row, best_of=3, seed=1, temperature=1.5)
        _until(lambda: any(f is f_long for f in list(srv._futs.values())))      # handed to the session: decoding from its next run
        rid_long = next(r for r, f in list(srv._futs.items()) if f is f_long)
        futs = [srv.submit(r, **q) for r, q in zip(others, oreq)]
        assert f_long.cancel()
        f_after = srv.submit(others[0], **oreq[0])
        res = [f.result(timeout=120) for f in futs]
        assert f_after.result(timeout=120) is not None
    assert f_long.cancelled()
    # the worker cancelled it in the session while it was decoding (its decode rows went to the next admission)
    assert calls == [(rid_long, "decoding")], calls
    for i in range(3):
        np.testing.assert_array_equal(res[i], refs[i], err_msg=f"request {i}")
    np.testing.assert_array_equal(f_after.result(), refs[0])
    # a Future delivered already cannot be cancelled
    assert not futs[0].cancel()


def test_audio_server_per_request_sampling_and_cancel(monkeypatch):
    from vallex_amd.utils import generation as G
    G.preload_models(state_dict=synth.vallex_state_dict(2, 11), vocos_state_dict=synth.vocos_state_dict(2), num_layers=2, max_new=320,
                     max_prompt=400, max_text=256, max_batch=8)
    pdir = os.path.join(os.path.dirname(__file__), "golden", "presets")
    texts = [synth.synth_text(12, 71), synth.synth_text(7, 72), synth.synth_text(15, 73)]
    prompts = [os.path.join(pdir, "paimon.npz"), None, os.path.join(pdir, "cafe.npz")]
    langs = ["en", "zh", "ja"]
    kw = [dict(best_of=3, seed=21, top_k=10, temperature=0.7), dict(best_of=1, seed=22, top_k=1), dict(best_of=2, seed=23)]
    want = []
    for t, p, lg, k in zip(texts, prompts, langs, kw):
        row = G._utterance_row(t, p, lg, "no-accent", None)
        k = dict(dict(top_k=-100, temperature=1.0), **k)     # AudioServer.submit's defaults: generate_audio's
        codes = G.model.inference_batch([row], force_eos_at=20, **k)[0]
        want.append(G.model.engine.vocos_decode([codes], 2)[0].copy())
    # the defaults equal generate_audio_batch
    np.testing.assert_array_equal(want[2], G.generate_audio_batch([texts[2]], prompts=[prompts[2]], language=[langs[2]], force_eos_at=20,
                                                                  **kw[2])[0])
    with G.AudioServer(force_eos_at=20, max_steps=1) as srv:
        futs = [srv.submit(t, prompt=p, language=lg, **k) for t, p, lg, k in zip(texts, prompts, langs, kw)]
        wavs = [f.result(timeout=120) for f in futs]
    for i in range(3):
        np.testing.assert_array_equal(wavs[i], want[i], err_msg=f"utterance {i}")
    # cancelling a DECODING request: no forced EOS, a 60-id text (cap min(16 x 60, max_new 320) frames) with five beams
    long_text = synth.synth_text(60, 74)
    row = G._utterance_row(texts[1], prompts[1], langs[1], "no-accent", None)
    other = G.model.engine.vocos_decode([G.model.inference_batch([row], top_k=-100, temperature=1.0, seed=31)[0]], 2)[0].copy()
    calls = _record_cancels(monkeypatch)
    with G.AudioServer(max_steps=1) as srv:
        f_long = srv.submit(long_text, prompt=prompts[0], language="en", best_of=5, seed=99)
        _until(lambda: any(f is f_long for f in list(srv._server._futs.values())))       # handed to the session
        rid_long = next(r for r, f in list(srv._server._futs.items()) if f is f_long)
        f_other = srv.submit(texts[1], prompt=prompts[1], language=langs[1], seed=31)
        assert f_long.cancel()
        w = f_other.result(timeout=120)
    assert f_long.cancelled()
    assert calls == [(rid_long, "decoding")], calls
    np.testing.assert_array_equal(w, other)


def test_threads_submit_and_cancel_concurrently():
    """two client threads submit while a third cancels every other Future: the remaining Futures equal their batch-1 results"""
    m = _model(8)
    rows = _rows(12, 9890)
    reqs = [dict(best_of=(1, 3)[i % 2], seed=3_000 + i, top_k=(10, -100)[i % 2], force_eos_at=(30, 9)[i % 2]) for i in range(12)]
    refs = [_alone(m, r, q)[0] for r, q in zip(rows, reqs)]
    futs = [None] * 12
    with m.serve(max_steps=2) as srv:
        def client(k):
            for i in range(k, 12, 2):
                futs[i] = srv.submit(rows[i], **reqs[i])

        th = [threading.Thread(target=client, args=(k,)) for k in (0, 1)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        flags = [futs[i].cancel() for i in range(0, 12, 3)]
    for i, f in enumerate(futs):
        assert f.done()
        if f.cancelled():
            assert i % 3 == 0
            continue
        np.testing.assert_array_equal(f.result(), refs[i], err_msg=f"request {i}")
    # cancel() returned True exactly for the Futures that end cancelled: no result reached any of them
    assert flags == [futs[i].cancelled() for i in range(0, 12, 3)], flags
