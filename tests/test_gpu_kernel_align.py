"""GPU: align_rows_kernel (csrc/align.hip, the kernel behind vx_align) on caller-chosen operands, one launch each through
vx_dev_align_rows (include/vallex_hip_dev.h), against float64 and on exact probes.

Sequences (S, Tp, T) = text, BOS ++ prompt, reported frames; R = VX_DEV_ALIGN_ROW_TILE, Kt = VX_DEV_ALIGN_KEY_TILE (both 32): one row,
R - 1 / R / R + 1 reported rows, S + Tp + T at Kt, Kt + 1 and 2 Kt - 1, S = 31 and S = 32 against ld_out = 32 and 36, and one sequence
that reports a suffix of its audio rows only (q_first > S + Tp).

Tolerance of the float64 comparison: the rule and the factor of tests/test_gpu_kernel_attention.py -- per operand set the kernel's
rms and max error against float64 may each be at most 4 x those of the same definition in torch-CPU fp32 on the same operands
(the arithmetic is the yardstick's; the factor covers summation order).  A sequence run alone is held to the set's max bound (an rms
over one sequence's few rows is not the set's rms).  Measured on the MI355X (docs/log_r19.md), the launch of 7 sequences: rms 0.81 ..
0.88 x, max 0.51 .. 1.00 x the yardstick over the four operand / weight sets; single sequences max 0.06 .. 1.00 x."""
import numpy as np
import pytest

from tests import _align_refs as A
from tests import _kernel_refs as R
from tests._util import get_model

pytestmark = pytest.mark.gpu

FACTOR = 4.0
_REF = {}


@pytest.fixture(scope="module")
def eng():
    return get_model(2, 1, 0.0, max_new=160, max_prompt=96, max_text=32, max_batch=32).engine


def _tiles():
    from vallex_amd._capi import DEV_ALIGN_KEY_TILE, DEV_ALIGN_ROW_TILE
    return DEV_ALIGN_ROW_TILE, DEV_ALIGN_KEY_TILE


def _seqs():
    Rt, Kt = _tiles()
    seqs = [(1, 0, 1), (5, 0, Rt - 1), (32, 3, Rt), (17, 40, Rt + 1), (4, 8, Kt - 12), (4, 8, Kt - 11), (31, 2, 2 * Kt - 34)]
    assert [sum(s) for s in seqs[4:]] == [Kt, Kt + 1, 2 * Kt - 1] and min(s[2] for s in seqs) >= 1
    q_first = [None] * 7
    q_first[5] = 4 + 8 + 6                      # a suffix of the audio rows only
    return seqs, q_first


def _tab():
    seqs, qf = _seqs()
    return A.make_tab(seqs, qf)


def _operands(kind):
    tab, M, rows = _tab()
    return R.attention_operands(kind)[:M].copy()


def _weights(kind):
    rng = np.random.default_rng(17)
    return {"uniform": np.full(16, 1 / 16, np.float32), "random": rng.uniform(0.0, 1.0, 16).astype(np.float32),
            "sparse": (rng.uniform(0.0, 1.0, 16) * (np.arange(16) % 3 == 1)).astype(np.float32)}[kind]


def reference(kind, wkind):
    """(qkv, w, float64 rows per sequence, yardstick rms, yardstick max), once per operand set"""
    if (kind, wkind) not in _REF:
        tab, M, rows = _tab()
        qkv, w = _operands(kind), _weights(wkind)
        want = A.align_rows_ref(qkv, tab, w)
        y = A.align_rows_fp32_yardstick(qkv, tab, w)
        err = np.concatenate([(a.astype(np.float64) - b).ravel() for a, b in zip(y, want)])
        _REF[(kind, wkind)] = (qkv, w, want, float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max()))
    return _REF[(kind, wkind)]


def launch(eng, qkv, tab, w, ld_out=36, extra=3, fill=None):
    rows = int(tab[:, 4].sum())
    out = np.zeros((rows + extra, ld_out), np.float32) if fill is None else fill.copy()
    return eng.dev_align_rows(qkv, tab, w, out)


def split(out, tab):
    """(reported (T, S) block per sequence, mask of every element of `out` that belongs to no block)"""
    rest = np.ones(out.shape, bool)
    blocks = []
    for _, _, S, _, T, o in tab:
        blocks.append(out[o:o + T, :S])
        rest[o:o + T, :S] = False
    return blocks, rest


def alone(tab, qkv, i):
    """sequence i as a launch of its own: (tab (1, 6), its rows of qkv)"""
    off, n = int(tab[i, 0]), int(tab[i, 1])
    t = tab[i:i + 1].copy()
    t[0, 0], t[0, 5] = 0, 0
    return t, qkv[off:off + n]


# ---- 1. float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld_out", [32, 36])
@pytest.mark.parametrize("wkind", ["uniform", "random"])
@pytest.mark.parametrize("kind", ["uniform", "model"])
def test_align_rows_against_float64(eng, kind, wkind, ld_out):
    tab, M, rows = _tab()
    qkv, w, want, y_rms, y_max = reference(kind, wkind)
    print(f"\n[align] {kind} / w {wkind}: yardstick (torch-CPU fp32) rms {y_rms:.3e}, max {y_max:.3e}")
    runs = [("7 sequences", tab, qkv, want)] + [(f"sequence {i} alone",) + alone(tab, qkv, i) + ([want[i]],) for i in range(len(tab))]
    bad = []
    for tag, tb, x, wnt in runs:
        out = launch(eng, x, tb, w, ld_out)
        got, rest = split(out, tb)
        assert np.isfinite(out).all() and (out[rest] == 0).all(), (tag, "an element outside the reported ranges was written")
        err = np.concatenate([(g.astype(np.float64) - r).ravel() for g, r in zip(got, wnt)])
        assert err.size + int(rest.sum()) == out.size                  # every element of out is in one of the two checks
        rms, mx = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
        print(f"[align] {kind} / w {wkind} / ld {ld_out} / {tag}: " + (f"rms {rms:.3e} = {rms / y_rms:.2f} x, " if tag == "7 sequences" else "")
              + f"max {mx:.3e} = {mx / y_max:.2f} x yardstick")
        if tag == "7 sequences" and (rms > FACTOR * y_rms or mx > FACTOR * y_max):
            bad.append((tag, round(rms / y_rms, 2), round(mx / y_max, 2)))
        if tag != "7 sequences" and mx > FACTOR * y_max:               # a single sequence: the set's max bound holds for each of them
            bad.append((tag, round(mx / y_max, 2)))
    assert not bad, f"{kind} / {wkind}: error above {FACTOR} x the fp32 yardstick: {bad}"


# ---- 2. exact probes ------------------------------------------------------------------------------------------------------
def _ulp_close(got, want64, ulps=2):
    want32 = np.asarray(want64, np.float64).astype(np.float32)
    return np.abs(got.astype(np.float64) - want64) <= ulps * np.spacing(np.abs(want32)).astype(np.float64)


@pytest.mark.parametrize("wkind", ["uniform", "random", "sparse"])
def test_zero_queries_give_the_uniform_distribution(eng, wkind):
    tab, M, rows = _tab()
    qkv, w = _operands("model"), _weights(wkind)
    qkv[:, :1024] = 0
    got, rest = split(launch(eng, qkv, tab, w), tab)
    for g, (_, _, S, qf, T, _) in zip(got, tab):
        n = qf + np.arange(T) + 1
        want = np.repeat((w.astype(np.float64).sum() / n)[:, None], S, 1)
        ok = _ulp_close(g, want)
        assert ok.all(), (wkind, S, T, np.argwhere(~ok)[:3], g[~ok][:3], want[~ok][:3])


def test_an_aligned_key_takes_the_whole_row(eng):
    tab, M, rows = _tab()
    base = _operands("model")
    for i, t, s_star, h in ((3, 0, 16, 5), (3, 32, 0, 0), (6, 29, 30, 15), (2, 31, 31, 9)):
        off, n, S, qf, T, o = (int(v) for v in tab[i])
        qkv = base.copy()
        q = qkv[off + qf + t, h * 64:(h + 1) * 64].astype(np.float64)
        qkv[off + s_star, 1024 + h * 64: 1024 + (h + 1) * 64] = (80.0 * 8.0 / np.linalg.norm(q) ** 2 * q).astype(np.float32)   # score 80
        w = np.eye(16, dtype=np.float32)[h]
        p64 = A.align_rows_ref(qkv, tab[i:i + 1], w)[0][t]
        assert p64[s_star] > 1 - 1e-6, ("fixture", p64[s_star])
        got = split(launch(eng, qkv, tab, w), tab)[0][i][t]
        assert got[s_star] >= 1 - 1e-6 and got[s_star] <= 1.0, (i, t, got[s_star])
        assert (np.delete(got, s_star) <= 1e-6).all() and (got >= 0).all(), (i, t)


def test_the_first_masked_key_changes_nothing(eng):
    """key r + 1 scores 1e4 above every visible key of row r: row r must not move by a bit, where r is the last row of its tile
    (key r + 1 lies behind the tile's key range) and where it is the first (key r + 1 is inside it)"""
    Rt, _ = _tiles()
    tab, M, rows = A.make_tab([(10, 5, Rt + 8), (5, 0, Rt - 1)])
    base = R.attention_operands("model")[:M].copy()
    w = _weights("random")
    ref = split(launch(eng, base, tab, w), tab)[0]
    i = 0
    off, n, S, qf, T, o = (int(v) for v in tab[i])
    for t in (Rt - 1, Rt):
        qkv = base.copy()
        for h in range(16):
            q = qkv[off + qf + t, h * 64:(h + 1) * 64].astype(np.float64)
            qkv[off + qf + t + 1, 1024 + h * 64: 1024 + (h + 1) * 64] = (1e4 * 8.0 / np.linalg.norm(q) ** 2 * q).astype(np.float32)
        got = split(launch(eng, qkv, tab, w), tab)[0]
        np.testing.assert_array_equal(got[i][: t + 1].view(np.uint32), ref[i][: t + 1].view(np.uint32))
        assert (got[i][t + 1] != ref[i][t + 1]).any()                     # the row that sees the key does move
        for j in range(len(tab)):
            if j != i:
                np.testing.assert_array_equal(got[j].view(np.uint32), ref[j].view(np.uint32))


# ---- 3. weights -----------------------------------------------------------------------------------------------------------
def test_head_weights(eng):
    tab, M, rows = _tab()
    qkv = _operands("model")
    a, b = 3, 12
    one = {}
    for h in (a, b):
        w = np.eye(16, dtype=np.float32)[h]
        want = A.align_rows_ref(qkv, tab, w)
        y = A.align_rows_fp32_yardstick(qkv, tab, w)
        y_max = max(float(np.abs(p.astype(np.float64) - q).max()) for p, q in zip(y, want))
        one[h] = split(launch(eng, qkv, tab, w), tab)[0]
        mx = max(float(np.abs(g.astype(np.float64) - r).max()) for g, r in zip(one[h], want))
        print(f"[align] one-hot head {h}: max {mx:.3e} = {mx / y_max:.2f} x yardstick")
        assert mx <= FACTOR * y_max, (h, mx, y_max)
    w = np.zeros(16, np.float32)
    w[a] = w[b] = 0.5
    half = split(launch(eng, qkv, tab, w), tab)[0]
    for g, pa, pb in zip(half, one[a], one[b]):
        ok = _ulp_close(g, 0.5 * (pa.astype(np.float64) + pb.astype(np.float64)))
        assert ok.all(), np.argwhere(~ok)[:3]
    # a head with w = 0 is skipped, not multiplied by zero: NaN queries there leave no trace
    bad = qkv.copy()
    bad[:, 7 * 64: 8 * 64] = np.nan
    out = launch(eng, bad, tab, w)
    assert np.isfinite(out).all()
    for g, g0 in zip(split(out, tab)[0], half):
        np.testing.assert_array_equal(g.view(np.uint32), g0.view(np.uint32))


# ---- 4. accumulate, and leave the rest alone ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ld_out", [32, 36])
def test_out_is_accumulated_into_and_everything_else_is_left_alone(eng, ld_out):
    tab, M, rows = _tab()
    tab = tab.copy()
    tab[:, 5] += 2                                                   # two spare rows in front, three behind
    qkv, w = _operands("uniform"), _weights("random")
    zero = launch(eng, qkv, tab, w, ld_out, extra=5)
    pattern = np.random.default_rng(23).uniform(-1.0, 1.0, zero.shape).astype(np.float32)
    out = launch(eng, qkv, tab, w, ld_out, fill=pattern)
    got, rest = split(out, tab)
    assert rest[:2].all() and rest[-3:].all() and rest[:, 32:].all()
    np.testing.assert_array_equal(out[rest].view(np.uint32), pattern[rest].view(np.uint32))
    np.testing.assert_array_equal(out[~rest].view(np.uint32), (pattern + zero)[~rest].view(np.uint32))
    assert (zero[rest] == 0).all() and (zero[~rest] > 0).all()


# ---- 5. determinism -----------------------------------------------------------------------------------------------------------
def test_two_launches_and_a_sequence_alone_give_the_same_bits(eng):
    tab, M, rows = _tab()
    qkv, w = _operands("model"), _weights("random")
    first = launch(eng, qkv, tab, w)
    np.testing.assert_array_equal(first.view(np.uint32), launch(eng, qkv, tab, w).view(np.uint32))
    blocks = split(first, tab)[0]
    for i in range(len(tab)):
        tb, x = alone(tab, qkv, i)
        np.testing.assert_array_equal(split(launch(eng, x, tb, w), tb)[0][0].view(np.uint32), blocks[i].view(np.uint32), err_msg=f"sequence {i}")


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_entry_refuses_what_the_kernel_does_not_take(eng):
    import ctypes as C
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_EINVAL, VX_ESTATE, _ptr
    tab, M, rows = _tab()
    qkv, w = _operands("uniform"), _weights("uniform")
    out = np.zeros((rows, 32), np.float32)

    def refused(code, field, **kw):
        a = dict(qkv=qkv, tab=tab, w=w, out=out)
        a.update(kw)
        with pytest.raises(VallexHipError) as e:
            eng.dev_align_rows(a["qkv"], a["tab"], a["w"], a["out"])
        assert e.value.code == code and field in str(e.value), (field, str(e.value))

    def edit(i, col, v):
        t = tab.copy()
        t[i, col] = v
        return t

    refused(VX_EINVAL, "nseq", tab=np.zeros((0, 6), np.int32))
    refused(VX_EINVAL, "nseq", tab=np.repeat(tab[:1], 33, 0))
    refused(VX_EINVAL, "M", qkv=np.zeros((0, 3072), np.float32))
    refused(VX_EINVAL, "M", qkv=np.zeros((8193, 3072), np.float32), tab=tab[:1])
    refused(VX_EINVAL, "seq_off", tab=edit(6, 0, tab[6, 0] + 1))            # the last sequence leaves [0, M)
    refused(VX_EINVAL, "seq_off", tab=edit(0, 0, -1))
    refused(VX_EINVAL, "S", tab=edit(1, 2, 0))
    refused(VX_EINVAL, "q_first", tab=edit(1, 3, 4))                         # below S = 5
    refused(VX_EINVAL, "n_rows", tab=edit(1, 4, tab[1, 4] + 1))              # q_first + n_rows > seq_len
    refused(VX_EINVAL, "ld_out", out=np.zeros((rows, 31), np.float32))       # below max S = 32
    refused(VX_EINVAL, "out_off", tab=edit(6, 5, tab[6, 5] + 1))             # behind rows_out
    refused(VX_EINVAL, "overlap", tab=edit(1, 5, 0))
    for v in (np.nan, np.inf, -0.25):
        bw = w.copy()
        bw[3] = v
        refused(VX_EINVAL, "w[3]", w=bw)
    t32 = np.ascontiguousarray(tab, np.int32)
    for null in range(4):                                                     # null pointers: the raw entry
        args = [_ptr(t32, C.c_int32), _ptr(qkv, C.c_float), _ptr(w, C.c_float), _ptr(out, C.c_float)]
        args[null] = None
        assert eng.lib.vx_dev_align_rows(eng.ctx, M, len(tab), args[0], args[1], args[2], args[3], rows, 32) == VX_EINVAL
        assert b"null" in eng.lib.vx_last_error(eng.ctx)
    assert (out == 0).all()
    with eng.serve(top_k=1, force_eos_at=4):
        refused(VX_ESTATE, "session")
    # the context is still usable
    got = split(launch(eng, qkv, tab, w, 32, extra=0), tab)[0]
    want = A.align_rows_ref(qkv, tab, w)
    assert max(float(np.abs(g - r).max()) for g, r in zip(got, want)) < 1e-5
