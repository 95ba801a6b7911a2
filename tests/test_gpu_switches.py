"""GPU: every per-context kernel-selection switch of the README against the CPU oracle, row by row -- the sentence "the switched
paths give the same token ids", held by the suite.

The recipe of tests/test_gpu_fuzz.py: 2 layers, weight seed 12, eos_gain 2.5 (rows END AT DIFFERENT STEPS and ride along as dead
columns), cap 36, seeded ragged rows (prompts 0 .. 90 frames, texts 1 .. 30 tokens, three languages), top-k 10 with injected
uniforms.  Every row of every batch must equal VallexOracle.inference on that row alone: equality of ids, no trial dropped, no row
skipped.  A batch of n rows is rows 3 n, 3 n + 1, ... (mod 32) of one seeded list of 32 rows, so the oracle runs once per ROW for the
whole module, whatever switch asks.

Each line of SWITCH_LINES gets ONE fresh context created under its environment (tests/_util.py switched_model: never cached, dropped
at teardown, max_batch 32 only where the line has more than 16 rows), asserts what vx_dev_switches reports -- a test that sets a
switch and cannot show that the context read it proves nothing -- and runs its row counts.  tests/test_kernel_refs.py checks on the
CPU that every per-context switch the README names has a line here.  The chains behind the switches are held to float64 one launch
at a time by tests/test_gpu_kernel_dec_attn_switches.py."""
import numpy as np
import pytest

from oracle import synth
from oracle.vallex_oracle import VallexOracle
from tests import _kernel_refs as R
from tests._util import drop_switched, switched_model

pytestmark = pytest.mark.gpu

NL, SEED, EOS_GAIN, CAP = 2, 12, 2.5, 36
NROWS = 32
ARENA = dict(max_new=64, max_prompt=128, max_text=64)                      # tests/test_gpu_fuzz.py
SMALL_ARENA = dict(max_new=40, max_prompt=48, max_text=24)                 # Tmax = 24 + 1 + 48 + 40 + 1 = 114 < 128: fuse_out is cleared

# line -> environment, the fields vx_dev_switches must report besides the defaults, row counts
SWITCH_LINES = {
    "sb_qkv_0": dict(env={"VX_SB_QKV": "0"}, fields=dict(sb_qkv_rows=0), rows=(1, 2, 3, 4)),
    "sb_fuse_0": dict(env={"VX_SB_FUSE": "0"}, fields=dict(sb_fuse=0), rows=(1, 2, 3, 4)),
    "sb_qkv_nsplit_4": dict(env={"VX_SB_QKV_NSPLIT": "4"}, fields=dict(sb_qkv_nsplit=4), rows=(1, 2)),
    "fuse_out_0": dict(env={"VX_FUSE_OUT": "0"}, fields=dict(fuse_out=0), rows=(8, 12, 17, 32)),
    "fuse_split_0": dict(env={"VX_FUSE_SPLIT": "0"}, fields=dict(fuse_split=0), rows=(8, 9, 16)),
    "att_nsplit_1": dict(env={"VX_ATT_NSPLIT": "1"}, fields=dict(att_nsplit_force=1), rows=(5, 9, 20)),
    "att_nsplit_2": dict(env={"VX_ATT_NSPLIT": "2"}, fields=dict(att_nsplit_force=2), rows=(5, 9, 20)),
    "att_nsplit_8": dict(env={"VX_ATT_NSPLIT": "8"}, fields=dict(att_nsplit_force=8), rows=(8,)),
    "qkv_balanced_0": dict(env={"VX_QKV_BALANCED": "0"}, fields=dict(qkv_bal=0), rows=(5, 8, 17, 32)),
    "balance_rows_0": dict(env={"VX_BALANCE_ROWS": "0"}, fields=dict(balance_rows=0), rows=(8, 9, 17), ascending=True),
    "nar_trim_0": dict(env={"VX_NAR_TRIM": "0"}, fields=dict(nar_trim=0), rows=(1, 5)),
    "graph_multi_0": dict(env={"VX_GRAPH_MULTI": "0"}, fields=dict(graph_multi=0), rows=(1, 5)),
    # the arithmetic of the full-sequence path (prefill and NAR stages), as the environment selects it when vx_config.arith is left alone
    "gemm_x3": dict(env={"VX_GEMM_X3": "1"}, fields=dict(gemm_mode=1), rows=(1, 5)),
    "gemm_f32": dict(env={"VX_GEMM_F32": "1"}, fields=dict(gemm_mode=2), rows=(1, 5)),
    "attn_x3": dict(env={"VX_ATTN_X3": "1"}, fields=dict(attn_h2=0), rows=(1, 5)),
    "attn_f32": dict(env={"VX_ATTN_F32": "1"}, fields=dict(attn_x3=0), rows=(1, 5)),
    # no switch: a context with small arenas decodes 8 .. 32 rows on the unfused chain (weights.hip clears fuse_out below one tile)
    "small_arena": dict(env={}, fields=dict(fuse_out=0), rows=(8, 20, 32), arena=SMALL_ARENA),
}

_ROWS, _REFS, _ORC = {}, {}, []


def master_rows(small):
    """the 32 seeded rows of an arena class and their uniform columns: [(row dict, uniforms (4096,), key of the row's reference)].
    The small arenas take the rows of the other list that fit them (prompts up to 48 frames, texts up to 24 tokens), in order, and
    seeded rows of their own for the rest: a row's reference does not depend on the arena, so it is computed once."""
    if small not in _ROWS:
        rng = np.random.default_rng(9100 + int(small))
        out = []
        if small:
            out = [e for e in master_rows(False) if len(e[0]["text"]) <= SMALL_ARENA["max_text"] and e[0]["prompt"].shape[0] <= SMALL_ARENA["max_prompt"]]
            assert 16 <= len(out) < NROWS
        for i in range(len(out), NROWS):
            tp = int(rng.choice([0, 1, 2, int(rng.integers(3, 45 if small else 91))]))
            sp = 0 if tp == 0 else int(rng.integers(1, 13))
            nt = int(rng.integers(1, 11 if small else 19))
            a, t = synth.synth_prompt(tp, sp, seed=int(rng.integers(1, 1 << 30)))
            txt = np.concatenate([t[0], synth.synth_text(nt, int(rng.integers(1, 1 << 30)))])
            lang = ("en", "zh", "ja")[int(rng.integers(0, 3))]
            row = dict(text=txt, prompt=a[0], enroll=sp, prompt_language=lang, text_language=("en", "zh", "ja")[int(rng.integers(0, 3))])
            out.append((row, synth.uniforms(4096, 1, int(rng.integers(1, 1 << 30)))[:, 0], (small, i)))
        _ROWS[small] = out
    return _ROWS[small]


def reference(small, i):
    """VallexOracle.inference on master row i alone, computed once for the module"""
    r, u, key = master_rows(small)[i]
    if key not in _REFS:
        if not _ORC:
            _ORC.append(VallexOracle(synth.vallex_state_dict(NL, SEED, EOS_GAIN), NL))
        _REFS[key] = _ORC[0].inference(r["text"][None], np.array([len(r["text"])]), r["prompt"][None], r["enroll"], top_k=10,
                                       prompt_language=r["prompt_language"], text_language=r["text_language"], uniforms=u,
                                       force_eos_at=CAP)[0]
    return _REFS[key]


def batch_rows(n, small, ascending=False):
    """indices into the master list of the n rows of a batch; ascending: by context (text + prompt frames), shortest first"""
    idx = [(3 * n + i) % NROWS for i in range(n)]
    if ascending:
        rows = master_rows(small)
        idx.sort(key=lambda i: len(rows[i][0]["text"]) + rows[i][0]["prompt"].shape[0])
    return idx


@pytest.fixture
def context(monkeypatch):
    def make(line):
        spec = SWITCH_LINES[line]
        arena = spec.get("arena", ARENA)
        m = switched_model(monkeypatch, spec["env"], spec["fields"], NL, SEED, EOS_GAIN, max_batch=32 if max(spec["rows"]) > 16 else 16, **arena)
        if arena is SMALL_ARENA:
            sw = m.engine.dev_switches()
            assert sw["fuse_out"] == 0 and sw["Tmax"] == 114 and sw["Tmax"] < R.DEC_TILE, sw
        return m
    yield make
    drop_switched()


def run_line(context, line):
    spec = SWITCH_LINES[line]
    small = spec.get("arena") is SMALL_ARENA
    m = context(line)                                                      # asserts vx_dev_switches
    for n in spec["rows"]:
        idx = batch_rows(n, small, spec.get("ascending", False))
        rows, cols = [master_rows(small)[i][0] for i in idx], [master_rows(small)[i][1] for i in idx]
        if spec.get("ascending"):
            # batch order = ascending contexts: the identity launch order this switch selects is NOT the balanced one
            ctx = [len(r["text"]) + r["prompt"].shape[0] for r in rows]
            assert ctx == sorted(ctx) and list(R.balance_order(ctx)) != list(range(n)), (n, ctx)
        outs = m.inference_batch(rows, top_k=10, uniforms=np.stack(cols, axis=1), force_eos_at=CAP)
        lens = []
        for j, i in enumerate(idx):
            ref = reference(small, i)
            assert outs[j].shape == ref.shape, (line, n, j, i, outs[j].shape, ref.shape)
            np.testing.assert_array_equal(outs[j], ref, err_msg=f"{line}: row {j} (master row {i}) of {n}")
            lens.append(ref.shape[0])
        assert n < 5 or len(set(lens)) > 1, ("the rows of a batch must end at different steps", lens)
        print(f"[switches] {line}: {n} rows, generated lengths {lens}")


def test_sb_qkv_0(context):
    run_line(context, "sb_qkv_0")


def test_sb_fuse_0(context):
    run_line(context, "sb_fuse_0")


def test_sb_qkv_nsplit_4(context):
    run_line(context, "sb_qkv_nsplit_4")


def test_fuse_out_0(context):
    run_line(context, "fuse_out_0")


def test_fuse_split_0(context):
    run_line(context, "fuse_split_0")


def test_att_nsplit_1(context):
    run_line(context, "att_nsplit_1")


def test_att_nsplit_2(context):
    run_line(context, "att_nsplit_2")


def test_att_nsplit_8(context):
    run_line(context, "att_nsplit_8")


def test_qkv_balanced_0(context):
    run_line(context, "qkv_balanced_0")


def test_balance_rows_0(context):
    run_line(context, "balance_rows_0")


def test_nar_trim_0(context):
    run_line(context, "nar_trim_0")


def test_graph_multi_0(context):
    run_line(context, "graph_multi_0")


def test_gemm_x3(context):
    run_line(context, "gemm_x3")


def test_gemm_f32(context):
    run_line(context, "gemm_f32")


def test_attn_x3(context):
    run_line(context, "attn_x3")


def test_attn_f32(context):
    run_line(context, "attn_f32")


def test_small_arena(context):
    """no switch: Tmax 114 < 128 clears fuse_out, so 8, 20 and 32 rows decode on the unfused chain (2 | 1 | 1 splits)"""
    run_line(context, "small_arena")


def test_the_default_context_agrees_on_the_same_rows(context, monkeypatch):
    """the rows every switch is held to, on a context with no switch set: a seed at which the DEFAULT path disagreed with the oracle
    would say nothing about a switch"""
    m = switched_model(monkeypatch, {}, {}, NL, SEED, EOS_GAIN, max_batch=32, **ARENA)
    idx = list(range(NROWS))
    outs = m.inference_batch([master_rows(False)[i][0] for i in idx], top_k=10, uniforms=np.stack([master_rows(False)[i][1] for i in idx], axis=1),
                             force_eos_at=CAP)
    for i in idx:
        np.testing.assert_array_equal(outs[i], reference(False, i), err_msg=f"default context: master row {i}")
