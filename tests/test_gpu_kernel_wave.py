"""GPU: the glue kernels of the waveform half -- codebook_sum, im2col7, dwconv7, istft_prep, overlap_add (csrc/vocos.hip), im2col_seq,
lstm_cell, final_conv, enc_first_conv, enc_pad_elu, rvq_select (csrc/encodec.hip) -- one launch at a time through vx_dev_wave_op,
against the float64 references and derived bounds of tests/_wave_refs.py (pinned to the oracles and shown to bite on the CPU by
tests/test_wave_refs.py), and the tables built at load time (vc_dft, vc_win2, en_e2).

Every output carries EXTRA rows or samples behind its end that must still hold the sentinel; data movement and single fp32 operations
must be bit-identical (inputs row * C + c: every element names its place); input pad columns hold +1e30.

Worst observed err / bound per kernel on MI355X (printed by every test; 1.0 is the limit):
  codebook_sum 0 (exact)      im2col7 0 (exact)          dwconv7 0.307            istft_prep 0.299      overlap_add 0.372
  im2col_seq 0.286 (ELU; 0 without, the grid-stride launch included)   lstm_cell 0.977   final_conv 0.012      enc_first_conv 0.359
  enc_pad_elu 0.289           rvq_select 0.000 (612 of 637 rows decided by a clear gap, every chosen code the float64 argmin)
  tables: vc_dft 0.500 (correctly rounded), en_e2 0.078, vc_win2 bit-identical
lstm_cell's figure is a y element whose bound is little more than the half ulp of its own final addition; final_conv's bound is
gamma_225 of the sum of magnitudes, which 224 fused multiply-adds of mixed sign stay far below.
"""
import numpy as np
import pytest

from oracle.encodec_oracle import encodec_encoder_state_dict, encodec_state_dict
from tests import _wave_refs as R
from tests._util import get_model

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
EXTRA = R.EXTRA


@pytest.fixture(scope="module")
def eng():
    m = get_model(2, 0, 2.5, vocos=True, max_new=64, max_prompt=96, max_text=32, max_batch=4)
    sd = dict(encodec_state_dict(3))
    sd.update(encodec_encoder_state_dict(4))
    m.load_encodec_state_dict(sd)
    return m.engine


def launch(eng, kernel, kw, outs=None):
    """one vx_dev_wave_op launch of `kernel` on the keyword arguments of its reference; returns the output array (lstm_cell: cstate, h,
    y; rvq_select: codes, resid).  outs: caller arrays to use instead of fresh ones."""
    ex = kw.get("extra", 0)
    new = lambda shape, i=0: outs[i] if outs is not None else np.empty(shape, f32)
    if kernel == "codebook_sum":
        rows = len(kw["codes"])
        out = new((rows + ex, 128))
        eng.dev_wave_op(kernel, [rows, ex], a=kw["codebook"], ia=kw["codes"], out=out)
    elif kernel == "im2col7":
        rows = len(kw["x"])
        out = new((rows + ex, 896))
        eng.dev_wave_op(kernel, [rows, ex], a=kw["x"], ia=kw["row_t"], ib=kw["row_len"], out=out)
    elif kernel == "dwconv7":
        rows, C = kw["x"].shape
        out = new((rows + ex, C))
        eng.dev_wave_op(kernel, [rows, ex, C], a=kw["x"], w=kw["w"], bias=kw["bias"], ia=kw["row_t"], ib=kw["row_len"], out=out)
    elif kernel == "istft_prep":
        rows = len(kw["o"])
        out = new((rows + ex, 1312))
        eng.dev_wave_op(kernel, [rows, ex], a=kw["o"], out=out)
    elif kernel == "overlap_add":
        batch, frames, stride = len(kw["seq_off"]), len(kw["frames"]), kw["stride"]
        out = new(((batch * stride if stride else frames * 320) + ex,))
        eng.dev_wave_op(kernel, [batch, ex, frames, stride], a=kw["frames"], ia=kw["seq_off"], ib=kw["seq_len"], out=out)
    elif kernel == "im2col_seq":
        rows = len(kw["x"])
        out = new((rows + ex, kw["k"] * kw["C"]))
        eng.dev_wave_op(kernel, [len(kw["seq_off"]), ex, rows // max(kw["R"], 1), kw["C"], kw["k"], kw["mode"], kw["elu"], kw["R"]], a=kw["x"],
                        ia=kw["seq_off"], ib=kw["seq_len"], out=out)
    elif kernel == "final_conv":
        batch = len(kw["seq_off"])
        out = new((batch * kw["stride"] + ex,))
        eng.dev_wave_op(kernel, [batch, ex, len(kw["x"]) // max(kw["R"], 1), kw["R"], kw["stride"]], a=kw["x"], w=kw["w"], bias=kw["bias"],
                        ia=kw["seq_off"], ib=kw["seq_len"], out=out)
    elif kernel == "enc_first_conv":
        L = len(kw["wav"])
        out = new((L + ex, 32))
        eng.dev_wave_op(kernel, [L, ex], a=kw["wav"], w=kw["w"], bias=kw["bias"], out=out)
    elif kernel == "lstm_cell":
        frames = len(kw["xg"])
        c, h, y = (kw["cstate"].copy(), kw["h"].copy(), np.empty((frames + ex, 512), f32)) if outs is None else outs
        eng.dev_wave_op(kernel, [kw["batch"], kw["splitk"], frames, kw["t"], ex], a=kw["part"], b=kw["xg"], w=kw["skip"], ia=kw["seq_off"],
                        ib=kw["seq_len"], out=c, out2=h, out3=y)
        return c, h, y
    elif kernel == "rvq_select":
        rows = len(kw["resid"])
        codes, out = (np.empty((rows + ex, 8), np.int64), np.empty((rows + ex, 128), f32)) if outs is None else outs
        eng.dev_wave_op(kernel, [rows, ex, kw["q"]], a=kw["resid"], b=kw["scores"], w=kw["e2"], bias=kw["codebook"], out=out, codes=codes)
        return codes, out
    else:
        raise KeyError(kernel)
    return out


def run_cases(eng, kernel, cases):
    worst = 0.0
    for case in cases:
        ref, bound = R.expected(kernel, case)
        worst = max(worst, R.check(launch(eng, kernel, case["kw"]), ref, bound, f"{kernel} {case['name']}"))
    print(f"{kernel}: {len(cases)} launches, worst err / bound = {worst:.3f}")
    return worst


def test_codebook_sum_is_the_sequential_fp32_sum_in_ascending_q(eng):
    cases = R.codebook_sum_cases()
    for c in cases:                                                          # 0 and 1023 in every q (one row: one of them per q)
        cd = c["kw"]["codes"]
        assert ((cd == 0) | (cd == 1023)).any(0).all() and (len(cd) == 1 or ((cd == 0).any(0).all() and (cd == 1023).any(0).all()))
    assert run_cases(eng, "codebook_sum", cases) == 0.0                                                             # all of it exact


def test_im2col7_moves_rows_inside_their_own_sequence(eng):
    assert run_cases(eng, "im2col7", R.im2col7_cases()) == 0.0


def test_dwconv7_taps_and_accumulation(eng):
    run_cases(eng, "dwconv7", R.dwconv7_cases())


def test_istft_prep_clip_overflow_and_large_phases(eng):
    run_cases(eng, "istft_prep", R.istft_prep_cases())


def test_overlap_add_borders_envelope_and_stride(eng):
    win2 = np.empty(1280, f32)
    eng.dev_wave_op("tables", [], out2=win2)
    run_cases(eng, "overlap_add", R.overlap_add_cases(win2))


def test_tables_built_at_load_time(eng):
    dft, win2, e2 = np.empty((1280, 1312), f32), np.empty(1280, f32), np.empty((8, 1024), f32)
    eng.dev_wave_op("tables", [], out=dft, out2=win2, out3=e2)
    assert (R.bits(win2) == R.bits(R.hann_tables()[1])).all()
    M = R.dft_table_ref()
    # one fp32 ulp of the float64 value, plus what the float64 reference itself is uncertain by: an FFT of 1280 points carries about
    # eps log2(N) of its largest output (16 eps taken), which matters only where an element is an exact zero of the cosine
    allow = R.ulp32(M) + 16 * 2.0 ** -52 * np.abs(M).max()
    err = np.abs(dft.astype(f64) - M) / allow
    print(f"tables: vc_dft worst err / (1 ulp + reference error) = {err.max():.3f}")
    assert err.max() <= 1.0 and (R.bits(dft[:, 1282:]) == 0).all()
    dec = encodec_state_dict(3)
    cb = np.stack([dec[f"quantizer.{q}.embed"] for q in range(8)]).astype(f64)
    want = (cb ** 2).sum(2)
    over = np.abs(e2.astype(f64) - want) / (R.gamma(128) * want)
    print(f"tables: en_e2 worst err / bound = {over.max():.3f}")
    assert over.max() <= 1.0


@pytest.mark.parametrize("C", [32, 128, 512])
def test_im2col_seq_reflect_zero_extension_and_elu(eng, C):
    run_cases(eng, "im2col_seq", R.im2col_seq_cases(C))


def test_im2col_seq_grid_stride_loop(eng):
    assert run_cases(eng, "im2col_seq", [R.im2col_seq_big_case()]) == 0.0


def test_lstm_cell_live_and_finished_sequences(eng):
    worst = 0.0
    for case in R.lstm_cell_cases():
        refs, bounds = R.lstm_cell_ref(**case["kw"])
        for got, ref, bound, what in zip(launch(eng, "lstm_cell", case["kw"]), refs, bounds, ("cstate", "h", "y")):
            worst = max(worst, R.check(got, ref, bound, f"lstm_cell {case['name']} {what}"))
    print(f"lstm_cell: {len(R.lstm_cell_cases())} launches, worst err / bound = {worst:.3f}")


def test_final_conv_short_sequences_and_block_border(eng):
    run_cases(eng, "final_conv", R.final_conv_cases())


def test_enc_first_conv_reflect_of_short_inputs(eng):
    run_cases(eng, "enc_first_conv", R.enc_first_conv_cases())


def test_enc_pad_elu_geometry_and_padding(eng):
    worst = 0.0
    cases = R.enc_pad_elu_cases()
    for case in cases:
        kw = case["kw"]
        out = np.empty((kw["out_rows"], kw["x"].shape[1]), f32)
        geom = eng.dev_wave_op("enc_pad_elu", [len(kw["x"]), kw["out_rows"], kw["x"].shape[1], kw["r"]], a=kw["x"], out=out)
        assert tuple(geom) == R.enc_pad_geom_ref(len(kw["x"]), kw["r"]), (case["name"], geom)
        worst = max(worst, R.check(out, *R.enc_pad_elu_ref(**kw), f"enc_pad_elu {case['name']}"))
    print(f"enc_pad_elu: {len(cases)} launches, worst err / bound = {worst:.3f}")


def test_rvq_select_argmin_ties_and_rows_without_a_distance(eng):
    worst, decided, total = 0.0, 0, 0
    cases = R.rvq_cases() + [R.rvq_nan_case()]
    for case in cases:
        kw = case["kw"]
        codes, out = launch(eng, "rvq_select", kw)
        w, n = R.rvq_check(codes, out, name=f"rvq_select {case['name']}", expect=case["expect"], **kw)
        worst, decided, total = max(worst, w), decided + n, total + len(kw["resid"])
    print(f"rvq_select: {len(cases)} launches, worst (D[code] - min) / bound = {worst:.3f}, {decided} of {total} rows decided by a clear gap")
    codes, _ = launch(eng, "rvq_select", R.rvq_nan_case()["kw"])
    assert codes[2, 7] == 0


def _refused(eng, kernel, kw, outs):
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_EINVAL
    for o in outs:
        o[...] = 75
    with pytest.raises(VallexHipError) as e:
        launch(eng, kernel, kw, outs=outs)
    assert e.value.code == VX_EINVAL, e.value
    assert all((o == 75).all() for o in outs), kernel


def _with(kw, **changes):
    out = dict(kw)
    out.update(changes)
    return out


def test_refused_arguments_leave_the_outputs_untouched_vocos(eng):
    big = np.empty((5000, 1408), f32)
    kw = R.codebook_sum_cases()[0]["kw"]
    codes = kw["codes"].copy()
    codes[0, 3] = 1024
    _refused(eng, "codebook_sum", _with(kw, codes=codes), [big])                                     # a code outside 0 .. 1023
    codes[0, 3] = -1
    _refused(eng, "codebook_sum", _with(kw, codes=codes), [big])
    _refused(eng, "codebook_sum", _with(kw, codes=np.zeros((0, 8), np.int32)), [big])                 # rows below 1
    _refused(eng, "codebook_sum", _with(kw, codes=np.zeros((4097, 8), np.int32)), [np.empty((4200, 128), f32)])
    _refused(eng, "codebook_sum", _with(kw, extra=65), [big])
    kw = R.im2col7_cases()[0]["kw"]
    rl = kw["row_len"].copy()
    rl[-1] += 1                                                                                      # the last sequence runs past the buffer
    _refused(eng, "im2col7", _with(kw, row_len=rl), [big])
    rt = kw["row_t"].copy()
    rt[0] = 1                                                                                        # ... starts in front of it
    _refused(eng, "im2col7", _with(kw, row_t=rt), [big])
    kw = R.dwconv7_cases()[0]["kw"]
    _refused(eng, "dwconv7", _with(kw, row_len=rl), [big])
    _refused(eng, "dwconv7", _with(kw, x=np.zeros((len(rl), 256), f32), w=np.zeros((256, 7), f32), bias=np.zeros(256, f32)), [big])   # bad C
    _refused(eng, "istft_prep", dict(o=np.zeros((0, 1408), f32), extra=0), [big])
    kw = R.overlap_add_cases(np.ones(1280, f32))[0]["kw"]
    sl = kw["seq_len"].copy()
    sl[-1] += 1
    _refused(eng, "overlap_add", _with(kw, seq_len=sl), [big])                                       # a sequence running past the frames
    _refused(eng, "overlap_add", _with(kw, stride=9 * 320 - 1), [big])                               # stride shorter than the longest sequence
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_EINVAL
    for op in (12, -1):                                                                              # an unknown op
        big[...] = 75
        with pytest.raises(VallexHipError) as e:
            eng.dev_wave_op(op, [1, 0], a=big, out=big)
        assert e.value.code == VX_EINVAL and (big == 75).all()


def test_refused_arguments_leave_the_outputs_untouched_decoder(eng):
    big = np.empty((400, 3584), f32)
    kw = R.im2col_seq_cases(32)[0]["kw"]
    for bad in (dict(C=30), dict(C=516), dict(k=8), dict(k=0), dict(mode=2), dict(mode=1, k=3), dict(elu=2), dict(R=0)):
        _refused(eng, "im2col_seq", _with(kw, **bad), [big])
    sl = kw["seq_len"].copy()
    sl[-1] += 1
    _refused(eng, "im2col_seq", _with(kw, seq_len=sl), [big])                                        # a sequence running past the buffer
    so = kw["seq_off"].copy()
    so[0] = -1
    _refused(eng, "im2col_seq", _with(kw, seq_off=so), [big])
    kw = R.lstm_cell_cases()[4]["kw"]
    outs = [np.empty((32, 512), f32), np.empty((32, 512), f32), np.empty((len(kw["xg"]) + EXTRA, 512), f32)]
    sl = kw["seq_len"].copy()
    sl[-1] += 4
    for bad in (dict(splitk=3), dict(splitk=0), dict(t=-1), dict(batch=33), dict(batch=0), dict(seq_len=sl)):
        _refused(eng, "lstm_cell", _with(kw, **bad), outs)
    kw = R.final_conv_cases()[0]["kw"]
    sl = kw["seq_len"].copy()
    sl[-1] += 1
    for bad in (dict(seq_len=sl), dict(stride=1), dict(R=0), dict(extra=-1)):
        _refused(eng, "final_conv", _with(kw, **bad), [big])


def test_refused_arguments_leave_the_outputs_untouched_encoder(eng):
    big = np.empty((70000, 32), f32)
    kw = R.enc_first_conv_cases()[0]["kw"]
    _refused(eng, "enc_first_conv", _with(kw, wav=np.zeros(0, f32)), [big])
    _refused(eng, "enc_first_conv", _with(kw, wav=np.zeros(65537, f32)), [big])
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_EINVAL
    x = np.ones((5, 32), f32)
    for dims in ([5, 7, 32, 2], [5, 8 + 65, 32, 2], [5, 8, 30, 2], [5, 8, 32, 0], [0, 8, 32, 2]):      # out too small / too large, bad C, r, Lc
        out = np.full((80, 32), 75, f32)
        with pytest.raises(VallexHipError) as e:
            eng.dev_wave_op("enc_pad_elu", dims, a=x, out=out)
        assert e.value.code == VX_EINVAL and (out == 75).all()
    kw = R.rvq_nan_case()["kw"]
    outs = [np.empty((5 + EXTRA, 8), np.int64), np.empty((5 + EXTRA, 128), f32)]
    for bad in (dict(q=8), dict(q=-1), dict(extra=65)):
        _refused(eng, "rvq_select", _with(kw, **bad), outs)


def test_entry_is_refused_inside_a_serving_session(eng):
    from vallex_amd import VallexHipError
    from vallex_amd._capi import VX_ESTATE
    codes = np.random.default_rng(3).integers(0, 1024, (5, 8))
    before = eng.vocos_decode([codes])[0].copy(), eng.encodec_decode([codes])[0].copy()
    kw = R.codebook_sum_cases()[0]["kw"]
    launch(eng, "codebook_sum", kw)
    with eng.serve():
        out, win2 = np.full((1 + EXTRA, 128), 75, f32), np.full(1280, 75, f32)
        for op, args in (("codebook_sum", dict(dims=[1, EXTRA], a=kw["codebook"], ia=kw["codes"], out=out)), ("tables", dict(dims=[], out2=win2))):
            with pytest.raises(VallexHipError) as e:
                eng.dev_wave_op(op, **args)
            assert e.value.code == VX_ESTATE and (out == 75).all() and (win2 == 75).all()
    launch(eng, "codebook_sum", kw)
    # the entry works on private scratch: the product paths give the same bits before and after
    np.testing.assert_array_equal(eng.vocos_decode([codes])[0], before[0])
    np.testing.assert_array_equal(eng.encodec_decode([codes])[0], before[1])
