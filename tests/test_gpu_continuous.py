"""GPU: the continuous schedule (vx_infer_continuous, VALLE.inference_batch(continuous=True)).

A finished row's decode row is refilled with the next waiting caller row at the next host poll: every admitted row runs its own
prefill into the freed KV slot and its first sample while the other rows of the decode batch keep decoding.  Every row must still be
exactly what the oracle returns for that row alone, and what vx_infer returns for it in the same call."""
import numpy as np
import pytest

from oracle import synth
from oracle.make_golden import RANGE_CASES, TRAINED_CASES, all_cases
from oracle.vallex_oracle import VallexOracle
from tests._util import case_model, get_model, golden, inputs_row

pytestmark = pytest.mark.gpu

NL, SEED, EOS_GAIN, CAP = 2, 12, 2.5, 36
_ORC = {}


def _oracle():
    if "fuzz" not in _ORC:
        _ORC["fuzz"] = VallexOracle(synth.vallex_state_dict(NL, SEED, EOS_GAIN), NL)
    return _ORC["fuzz"]


def _fuzz_rows(n, seed):
    """the test_gpu_fuzz recipe: prompts 0 .. 90 frames, text 1 .. 18 ids, three languages; one uniforms column per row"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for _ in range(n):
        tp = int(rng.choice([0, 1, 2, int(rng.integers(3, 91))]))
        sp = 0 if tp == 0 else int(rng.integers(1, 13))
        nt = int(rng.integers(1, 19))
        a, t = synth.synth_prompt(tp, sp, seed=int(rng.integers(1, 1 << 30)))
        txt = np.concatenate([t[0], synth.synth_text(nt, int(rng.integers(1, 1 << 30)))])
        lang = ("en", "zh", "ja")[int(rng.integers(0, 3))]
        rows.append(dict(text=txt, prompt=a[0], enroll=sp, prompt_language=lang, text_language=("en", "zh", "ja")[int(rng.integers(0, 3))]))
        cols.append(synth.uniforms(4096, 1, int(rng.integers(1, 1 << 30)))[:, 0])
    return rows, cols


def _oracle_row(r, u, top_k=10, force_eos_at=CAP, orc=None):
    orc = orc or _oracle()
    return orc.inference(r["text"][None], np.array([len(r["text"])]), r["prompt"][None], r["enroll"], top_k=top_k,
                         prompt_language=r["prompt_language"], text_language=r["text_language"], uniforms=u,
                         force_eos_at=force_eos_at)[0]


def _model(max_batch):
    return get_model(NL, SEED, EOS_GAIN, max_new=64, max_prompt=128, max_text=64, max_batch=max_batch)


@pytest.mark.parametrize("max_batch", [4, 8, 32], ids=["sb_chain", "split_fused", "rows32"])
def test_ragged_rows_equal_the_oracle_and_vx_infer(max_batch):
    """2.5 x max_batch + 3 ragged rows on each decode chain: <= 4 rows (small-batch chain, slot == row), 8 rows (out_proj fused into
    the context-split dec_attn), 32 rows (one split, balanced slot order -- admitted rows take the freed rows' slots)"""
    n = int(2.5 * max_batch) + 3
    m = _model(max_batch)
    rows, cols = _fuzz_rows(n, 7143 + max_batch)
    U = np.stack(cols, axis=1)
    outs_c = m.inference_batch(rows, top_k=10, uniforms=U, force_eos_at=CAP, continuous=True)
    st_c = m.engine.last_stats()
    # vx_infer takes at most max_batch rows per call and decodes them as one micro-batch: the same rows in calls of max_batch rows
    # are exactly its schedule of this batch (row r depends on its own inputs and uniforms column only)
    outs_v, st_v = [], dict(ar_steps=0, frames=0)
    for r0 in range(0, n, max_batch):
        outs_v += m.inference_batch(rows[r0:r0 + max_batch], top_k=10, uniforms=U[:, r0:r0 + max_batch], force_eos_at=CAP)
        st = m.engine.last_stats()
        st_v["ar_steps"] += st["ar_steps"]; st_v["frames"] += st["frames"]
    lens = [o.shape[0] for o in outs_c]
    assert len(set(lens)) > 1, lens
    for i, (r, u) in enumerate(zip(rows, cols)):
        np.testing.assert_array_equal(outs_c[i], outs_v[i], err_msg=f"row {i} of {n}: continuous != vx_infer")
        ref = _oracle_row(r, u)
        assert outs_c[i].shape == ref.shape, (i, outs_c[i].shape, ref.shape)
        np.testing.assert_array_equal(outs_c[i], ref, err_msg=f"row {i} of {n}")
    assert st_c["frames"] == st_v["frames"] == sum(lens)
    assert st_c["ar_steps"] < st_v["ar_steps"], (st_c, st_v)
    print(f"max_batch {max_batch}, {n} rows: lengths {lens}; AR steps continuous {st_c['ar_steps']} vs micro-batched {st_v['ar_steps']}")


def test_callback_once_per_row_and_exceptions_reach_the_caller():
    m = _model(4)
    rows, cols = _fuzz_rows(11, 7200)
    U = np.stack(cols, axis=1)
    seen = []
    outs = m.inference_batch(rows, top_k=10, uniforms=U, force_eos_at=CAP, continuous=True, on_row=lambda r, c: seen.append((r, c)))
    assert sorted(r for r, _ in seen) == list(range(len(rows)))
    for r, c in seen:
        assert c.dtype == np.int64 and c.shape == outs[r].shape
        np.testing.assert_array_equal(c, outs[r])

    class Boom(RuntimeError):
        pass

    def bad(r, c):
        if r == 5:
            raise Boom("row 5")

    with pytest.raises(Boom):
        m.inference_batch(rows, top_k=10, uniforms=U, force_eos_at=CAP, continuous=True, on_row=bad)
    again = m.inference_batch(rows, top_k=10, uniforms=U, force_eos_at=CAP, continuous=True)
    for a, b in zip(again, outs):
        np.testing.assert_array_equal(a, b)


def _counter_uniforms(seed, r, steps):
    """include/vallex_hip.h: u = (splitmix64(splitmix64(splitmix64(seed) + r) + step) >> 40) x 2^-24"""
    M = (1 << 64) - 1

    def sm(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    base = sm((sm(seed) + r) & M)
    return np.array([np.float32(sm((base + t) & M) >> 40) * np.float32(1.0 / 16777216.0) for t in range(steps)], np.float32)


def test_counter_rng_is_keyed_on_the_caller_row():
    mb, seed = 4, 987654321
    m = _model(mb)
    rows, _ = _fuzz_rows(2 * mb + 5, 7300)
    outs = m.inference_batch(rows, top_k=10, seed=seed, force_eos_at=CAP, continuous=True)
    again = m.inference_batch(rows, top_k=10, seed=seed, force_eos_at=CAP, continuous=True)
    for a, b in zip(outs, again):
        np.testing.assert_array_equal(a, b)
    ref_v = m.inference_batch(rows[:mb], top_k=10, seed=seed, force_eos_at=CAP)
    for i in range(mb):
        np.testing.assert_array_equal(outs[i], ref_v[i], err_msg=f"row {i}: continuous != vx_infer with the same seed")
    r = mb + 3
    ref = _oracle_row(rows[r], _counter_uniforms(seed, r, 4096))
    np.testing.assert_array_equal(outs[r], ref, err_msg=f"row {r} against the oracle fed the documented counter draws")


def _fillers(n, seed):
    """short rows: S = 2 text ids -> the reference's cap of 16 x 2 = 32 frames"""
    out = []
    for i in range(n):
        a, t = synth.synth_prompt(12, 1, seed=seed + i)
        out.append(dict(text=np.concatenate([t[0], synth.synth_text(1, seed + 100 + i)]), prompt=a[0], enroll=1,
                        prompt_language="en", text_language=("en", "zh", "ja")[i % 3]))
    return out


def _assert_golden(name, out, g):
    gold = g["codes"][0]
    assert out.shape == gold.shape, (name, out.shape, gold.shape)
    d = np.argwhere(out != gold)
    if len(d):
        t, q = (int(v) for v in d[0])
        marg = float(g["ar_margin"][t]) if q == 0 else float(g["nar_margin"][q - 1])
        raise AssertionError(f"{name}: first differing id at frame {t}, codebook {q}: got {out[t, q]}, reference {gold[t, q]}; "
                             f"reference decision margin there {marg:.3e}; {int((out != gold).sum())} ids differ")


@pytest.mark.parametrize("arith", ["default", "f32"])
@pytest.mark.parametrize("name", ["nl12_trained_en_greedy", "nl12_trained_zh_topk10"])
def test_live_reference_goldens_admitted_mid_call(name, arith):
    """the 600-frame live-reference rows wait behind four short fillers (max_batch 4): they enter the decode batch by admission"""
    c = TRAINED_CASES[name]
    row, us = inputs_row(c)
    m = case_model(c, arith=arith, max_new=608, max_prompt=400, max_text=256, max_batch=4)
    rows = _fillers(4, 64_000) + [row] + _fillers(2, 65_000)
    cols = [synth.uniforms(4096, 1, 66_000 + i)[:, 0] for i in range(len(rows))]
    if us is not None:
        cols[4] = us
    U = None if us is None else np.stack(cols, axis=1)
    outs = m.inference_batch(rows, top_k=c["top_k"], uniforms=U, force_eos_at=c["force_eos_at"], continuous=True)
    assert all(o.shape[0] <= 32 for i, o in enumerate(outs) if i != 4)
    _assert_golden(f"{name} [{arith}] admitted as row 4", outs[4], golden(name))


def test_range_fallback_on_an_admission():
    """out-of-range FFN channels (RANGE_CASES: the same fp32 function as the base case, f16x2 operands beyond fp16): the admission
    round of the golden row leaves the range and is re-run, prefill and first sample, on the fp32 kernels"""
    name = "nl2_range_ffn"
    base, kind = RANGE_CASES[name]
    c = all_cases()[name]
    row, us = inputs_row(c)
    m = case_model(c, max_batch=4)
    rows = _fillers(4, 67_000) + [row]
    cols = [synth.uniforms(4096, 1, 68_000 + i)[:, 0] for i in range(len(rows))]
    if us is not None:
        cols[4] = us
    outs = m.inference_batch(rows, top_k=c["top_k"], uniforms=np.stack(cols, axis=1), force_eos_at=c["force_eos_at"], continuous=True)
    fb = m.engine.last_fallbacks()
    assert fb["prefill"] >= 2, fb                   # the first fill and (at least) the admission round of row 4
    _assert_golden(f"{name} admitted as row 4", outs[4], golden(base))
    orc = VallexOracle(synth.vallex_state_dict(c["num_layers"], c["seed"], c["eos_gain"]), c["num_layers"])
    for i in range(4):
        ref = _oracle_row(rows[i], cols[i], top_k=c["top_k"], force_eos_at=c["force_eos_at"], orc=orc)
        np.testing.assert_array_equal(outs[i], ref, err_msg=f"filler {i}")


def test_edge_cases():
    from vallex_amd._capi import VX_EINVAL, Engine, ROW_DONE_FN, _ptr
    import ctypes as C
    m = _model(4)
    rows, cols = _fuzz_rows(3, 7400)
    U = np.stack(cols, axis=1)
    eng = m.engine
    # best_of > 1 is refused by the library itself, not only by the binding
    b = m.make_batch(rows)
    s, _keep = Engine._sampling(b.n, 10, 1.0, None, 1, CAP, 8, best_of=2)
    out = np.zeros((b.n, eng.max_new, 8), np.int64)
    lens = np.zeros(b.n, np.int32)
    rc = eng.lib.vx_infer_continuous(eng.ctx, C.byref(b.c), C.byref(s), ROW_DONE_FN(), None, _ptr(out, C.c_int64), eng.max_new,
                                     _ptr(lens, C.c_int32))
    assert rc == VX_EINVAL and b"best_of" in eng.lib.vx_last_error(eng.ctx)
    # batch <= max_batch: nothing to admit, the callback still sees every row
    seen = []
    outs = m.inference_batch(rows, top_k=10, uniforms=U, force_eos_at=CAP, continuous=True, on_row=lambda r, c: seen.append(r))
    assert sorted(seen) == [0, 1, 2]
    ref = m.inference_batch(rows, top_k=10, uniforms=U, force_eos_at=CAP)
    for a, r in zip(outs, ref):
        np.testing.assert_array_equal(a, r)
    # one row equals vx_infer, with injected uniforms and with the counter-based RNG
    one = m.inference_batch(rows[:1], top_k=10, uniforms=U[:, :1], force_eos_at=CAP, continuous=True)[0]
    np.testing.assert_array_equal(one, m.inference_batch(rows[:1], top_k=10, uniforms=U[:, :1], force_eos_at=CAP)[0])
    one = m.inference_batch(rows[:1], top_k=10, seed=5, force_eos_at=CAP, continuous=True)[0]
    np.testing.assert_array_equal(one, m.inference_batch(rows[:1], top_k=10, seed=5, force_eos_at=CAP)[0])
