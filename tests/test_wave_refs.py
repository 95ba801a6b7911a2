"""CPU: the references of the waveform glue-kernel tests (tests/_wave_refs.py) against what the suite already pins -- the torch
convolutions and the padding rule of oracle/encodec_oracle.py, torch.nn.LSTM, the ISTFT head of oracle/vallex_oracle.py -- and the
evidence that every bound bites: on the GPU test's own inputs, each deliberately wrong kernel fails the assertion helper the GPU test
uses (tests/_wave_refs.check / rvq_check), while the correctly rounded reference passes it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import synth
from oracle.encodec_oracle import EncodecEncoderOracle, _pad1d_reflect, _pad_causal_reflect, encodec_state_dict
from oracle.vallex_oracle import VocosOracle
from tests import _wave_refs as R

f32, f64 = np.float32, np.float64
T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, f64))


def _close(a, b, tol=1e-11):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), np.abs(a - b).max()


def _cases(kernel):
    if kernel == "overlap_add":
        return R.overlap_add_cases(R.hann_tables()[1])
    if kernel == "im2col_seq":
        return [c for C in (32, 128, 512) for c in R.im2col_seq_cases(C)]
    return getattr(R, kernel + "_cases")()


KERNELS = ["codebook_sum", "im2col7", "dwconv7", "istft_prep", "overlap_add", "im2col_seq", "final_conv", "enc_first_conv", "enc_pad_elu"]


# ---- the correctly rounded reference passes its own check, with room -------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_rounded_reference_passes_the_check(kernel):
    worst = 0.0
    for case in _cases(kernel):
        ref, bound = R.expected(kernel, case)
        worst = max(worst, R.check(R.as_kernel_output(ref), ref, bound, case["name"]))
    print(kernel, "worst err / bound of float32(ref)", worst)
    assert worst <= 1.0                                  # (check raises beyond 1; half an ulp of the result is part of every bound)


def test_rounded_lstm_reference_passes_the_check():
    for case in R.lstm_cell_cases():
        refs, bounds = R.lstm_cell_ref(**case["kw"])
        for ref, bound, what in zip(refs, bounds, "chy"):
            R.check(R.as_kernel_output(ref), ref, bound, case["name"] + " " + what)
        # all three branches of the early return are in every launch with more than one sequence
        kw = case["kw"]
        live = kw["t"] < kw["seq_len"][: kw["batch"]]
        assert live.any() and (kw["batch"] == 1 or (~live).any())
        assert (kw["seq_len"] - 1 == kw["t"]).any()


# ---- pins to the oracles ----------------------------------------------------------------------------------------------------------
def test_im2col7_and_dwconv7_equal_the_oracles_convolutions():
    rng = np.random.default_rng(0)
    case = R.im2col7_cases()[0]["kw"]
    x = rng.standard_normal(case["x"].shape)
    W, b = rng.standard_normal((12, 128, 7)), rng.standard_normal(12)
    ref, _ = R.im2col7_ref(x.astype(f64), case["row_t"], case["row_len"], 0)
    got = ref @ R.im2col_weight(W).T + b
    for off, n in R.seqs_of_rows(case["row_t"], case["row_len"]):
        want = F.conv1d(T64(x[off: off + n].T)[None], T64(W), T64(b), padding=3)[0].numpy().T          # VocosOracle.backbone embed
        _close(got[off: off + n], want)
    for case in R.dwconv7_cases():
        kw = case["kw"]
        ref, _ = R.dwconv7_ref(**kw)
        C = kw["x"].shape[1]
        for off, n in R.seqs_of_rows(kw["row_t"], kw["row_len"]):
            want = F.conv1d(T64(kw["x"][off: off + n].T)[None], T64(kw["w"])[:, None, :], T64(kw["bias"]), padding=3, groups=C)   # convnext_branch
            _close(ref[off: off + n], want[0].numpy().T)


def test_codebook_sum_equals_codes_to_features():
    sd = synth.vocos_state_dict(2)
    orc = VocosOracle(sd)
    cb = sd["feature_extractor.codebook_weights"]
    codes = np.random.default_rng(1).integers(0, 1024, (9, 8))
    want = orc.codes_to_features(torch.from_numpy(codes.T[:, None, :]))[0].numpy().T                    # (8, B, T) -> (B, 128, T)
    ref, _ = R.codebook_sum_ref(codes, cb, 0)
    mag = np.abs(cb[1024 * np.arange(8) + codes]).sum(1)
    assert (np.abs(ref - want) <= R.gamma(8) * mag).all()                                                # torch's own order of the 8 adds


@pytest.mark.parametrize("C", [32])
def test_im2col_seq_equals_the_oracles_convolutions(C):
    rng = np.random.default_rng(2)
    for case in R.im2col_seq_cases(C):
        kw = case["kw"]
        ref, _ = R.im2col_seq_ref(**kw)
        k, Rr, r, O = kw["k"], kw["R"], 4, 6
        act = F.elu(T64(kw["x"])) if kw["elu"] else T64(kw["x"])
        for off, n in zip(kw["seq_off"], kw["seq_len"]):
            base, T = int(off) * Rr, int(n) * Rr
            if T == 0:
                continue
            seq = act[base: base + T].T[None]                                                           # (1, C, T)
            if kw["mode"] == 0:
                W, b = rng.standard_normal((O, C, k)), rng.standard_normal(O)
                want = F.conv1d(_pad_causal_reflect(seq, k - 1), T64(W), T64(b))[0].numpy().T           # EncodecDecoderOracle._conv
                _close(ref[base: base + T] @ R.im2col_weight(W).T + b, want, 1e-10)
            else:
                W, b = rng.standard_normal((C, O, 2 * r)), rng.standard_normal(O)
                want = F.conv_transpose1d(seq, T64(W), T64(b), stride=r)
                want = want[..., : want.shape[-1] - r][0].numpy().T                                     # (T r, O): decode()'s right trim
                got = (ref[base: base + T] @ R.convtr_weight(W, r).T).reshape(T * r, O) + b
                _close(got, want, 1e-10)


def test_final_and_first_conv_equal_the_oracles_convolutions():
    for case in R.final_conv_cases():
        kw = case["kw"]
        ref, _ = R.final_conv_ref(**kw)
        for b, (off, n) in enumerate(zip(kw["seq_off"], kw["seq_len"])):
            base, T = int(off) * kw["R"], int(n) * kw["R"]
            seq = F.elu(T64(kw["x"][base: base + T])).T[None]
            want = F.conv1d(_pad_causal_reflect(seq, 6), T64(kw["w"])[None], T64(kw["bias"]))[0, 0].numpy()     # decode(): "decoder.15"
            _close(ref[b * kw["stride"]: b * kw["stride"] + T], want, 1e-10)
    orc = EncodecEncoderOracle.__new__(EncodecEncoderOracle)
    for case in R.enc_first_conv_cases():
        kw = case["kw"]
        orc.w = {"c.weight": T64(kw["w"])[:, None, :], "c.bias": T64(kw["bias"])}
        want = orc._conv(T64(kw["wav"])[None, None], "c")[0].numpy().T                                  # embeddings(): "encoder.0"
        _close(R.enc_first_conv_ref(**kw)[0][: len(kw["wav"])], want, 1e-10)


def test_enc_pad_elu_equals_the_oracles_strided_conv():
    rng = np.random.default_rng(3)
    orc = EncodecEncoderOracle.__new__(EncodecEncoderOracle)
    for case in R.enc_pad_elu_cases():
        kw = case["kw"]
        x, r = kw["x"], kw["r"]
        Lc, C = x.shape
        rows, Le, n_out = R.enc_pad_geom_ref(Lc, r)
        assert n_out == -(-Lc // r) and rows == (n_out + 1) * r and Le >= Lc and (Le > Lc) == (Lc <= max(r, n_out * r - Lc))
        W, b = rng.standard_normal((5, C, 2 * r)), rng.standard_normal(5)
        orc.w = {"c.weight": T64(W), "c.bias": T64(b)}
        want = orc._conv(F.elu(T64(x)).T[None], "c", stride=r)[0].numpy().T                             # (n_out, 5)
        ref, _ = R.enc_pad_elu_ref(**kw)
        assert np.isnan(ref[rows:]).all() and not np.isnan(ref[:rows]).any()
        win = np.stack([ref[t * r: (t + 2) * r].reshape(-1) for t in range(n_out)])                     # overlapping rows, [pos][c]
        _close(win @ R.im2col_weight(W).T + b, want, 1e-10)
        # the torch padding itself, element by element
        _close(ref[:rows], _pad1d_reflect(F.elu(T64(x)).T, r, n_out * r - Lc).numpy().T, 1e-15)


def test_istft_references_equal_the_oracles_head():
    win, win2 = R.hann_tables()
    # torch.hann_window evaluated in float64 and rounded is the table's window bit for bit; evaluated in fp32 (what the oracle's head
    # calls) it is the same window to an ABSOLUTE 2^-21: the angle 2 pi n / N <= 2 pi carries two fp32 roundings (2 x 2^-24 x 2 pi),
    # |d/dx 0.5 cos x| <= 0.5 brings that to 3.8e-7, and the two roundings of the result add 2^-24 each
    window = torch.hann_window(1280, dtype=torch.float64).float()
    assert (window.numpy() == win.astype(f32)).all() and (window.square().numpy() == win2).all()
    assert np.abs(torch.hann_window(1280).double().numpy() - win).max() <= 2.0 ** -21
    # front + DFT table: reim . M^T == irfft(S) * window
    rng = np.random.default_rng(4)
    o = np.zeros((3, 1408), f32)
    o[:, :641], o[:, 641:1282] = rng.uniform(-3, 5, (3, 641)), rng.uniform(-7, 7, (3, 641))
    reim, _ = R.istft_prep_ref(o, 0)
    mag = torch.clip(torch.exp(T64(o[:, :641])), max=1e2)
    S = mag * (torch.cos(T64(o[:, 641:1282])) + 1j * torch.sin(T64(o[:, 641:1282])))
    want = torch.fft.irfft(S, 1280, dim=1, norm="backward") * window.double()
    _close(reim @ R.dft_table_ref().T, want.numpy(), 1e-12)
    # tail: fold, trim, divide by the folded envelope (VocosOracle.head)
    case = [c for c in R.overlap_add_cases(win2) if c["name"].startswith("random")][0]["kw"]
    ref, _ = R.overlap_add_ref(**case)
    for off, T in zip(case["seq_off"], case["seq_len"]):
        ifft = T64(case["frames"][off: off + T]).T[None]                                                # (1, 1280, T)
        size = (T - 1) * 320 + 1280
        yy = F.fold(ifft, output_size=(1, size), kernel_size=(1, 1280), stride=(1, 320))[:, 0, 0, 480:-480]
        wsq = window.square().double().expand(1, T, -1).transpose(1, 2)
        env = F.fold(wsq, output_size=(1, size), kernel_size=(1, 1280), stride=(1, 320)).squeeze()[480:-480]
        _close(ref[off * 320: (off + T) * 320], (yy / env)[0].numpy(), 1e-12)
    # the exact probes are exact by construction: fp32 evaluation == float64 reference for window frames
    for c in R.overlap_add_cases(win2):
        if c["name"].startswith("window"):
            ex, _ = R.overlap_add_exact(**c["kw"])
            assert (ex[~np.isnan(ex)] == 1.0).all()


def test_istft_inputs_keep_the_relative_bound_meaningful():
    for case in R.istft_prep_cases():
        o = case["kw"]["o"]
        p = o[:, 641:1282].astype(f64)
        nz = p != 0
        assert (p == 0).sum() == 2 * len(o)
        assert (np.abs(np.cos(p[nz])) >= 2.0 ** -10).all() and (np.abs(np.sin(p[nz])) >= 2.0 ** -10).all() and np.abs(p).max() > 9e3
        x = o[:, :641]
        for v in (-104.0, R.LN100, np.nextafter(R.LN100, f32(0)), np.nextafter(R.LN100, f32(9)), 89.0):
            assert (x == f32(v)).any()
        assert (o[:, 1282:] == f32(1e30)).all() and o[0, 2] == R.LN100 and o[0, 641 + 2] == 0      # p = 0 at the clip itself
        ref, bound = R.istft_prep_ref(**case["kw"])
        assert np.exp(89.0) > R.FLT_MAX and (np.abs(ref[: len(o), :1282]) <= 100).all() and (ref[: len(o), 1282:] == 0).all()
        assert (bound[: len(o), 1282:] == 0).all()


def test_lstm_cell_reference_equals_one_step_of_torch_lstm():
    torch.manual_seed(0)
    HD, B = 512, 3
    lstm = torch.nn.LSTM(HD, HD).double()
    x, h0, c0 = (torch.randn(1, B, HD, dtype=torch.float64) for _ in range(3))
    with torch.no_grad():
        y, (h1, c1) = lstm(x, (h0, c0))
        xg = F.linear(x[0], lstm.weight_ih_l0, lstm.bias_ih_l0 + lstm.bias_hh_l0).numpy()
        pt = F.linear(h0[0], lstm.weight_hh_l0).numpy()
    part = np.zeros((2, 32, 4 * HD))
    part[0, :B], part[1, :B] = 0.25 * pt, 0.75 * pt
    cst, hh = np.zeros((32, HD)), np.zeros((32, HD))
    cst[:B], hh[:B] = c0[0].numpy(), h0[0].numpy()
    refs, _ = R.lstm_cell_ref(part, 2, xg, np.arange(B), np.ones(B, int), 0, cst, hh, x[0].numpy(), B, 0)
    _close(refs[0][:B], c1[0].numpy(), 1e-13)
    _close(refs[1][:B], h1[0].numpy(), 1e-13)
    _close(refs[2][:B], (y[0] + x[0]).numpy(), 1e-13)                                                    # EncodecLSTM: lstm(x) + x


def test_rvq_distances_choose_the_oracles_codes():
    dec = encodec_state_dict(3)
    orc = EncodecEncoderOracle.__new__(EncodecEncoderOracle)
    orc.codebooks = [torch.from_numpy(dec[f"quantizer.{q}.embed"]) for q in range(8)]
    emb = (0.5 * np.random.default_rng(5).standard_normal((1, 128, 40))).astype(f32)
    codes = orc.quantize(torch.from_numpy(emb))[0]                                                       # (T, 8)
    cb = dec["quantizer.0.embed"]
    r = emb[0].T
    D, bnd = R.rvq_distances(r, (r.astype(f64) @ cb.astype(f64).T).astype(f32), (cb.astype(f64) ** 2).sum(1).astype(f32))
    srt = np.sort(D, 1)
    clear = srt[:, 1] - srt[:, 0] > 4 * bnd
    assert clear.sum() >= 36 and (np.argmin(D, 1)[clear] == codes[clear, 0]).all()


def test_rvq_inputs_have_a_clear_gap_in_most_rows():
    for case in R.rvq_cases():
        kw = case["kw"]
        D, bnd = R.rvq_distances(kw["resid"], kw["scores"], kw["e2"])
        srt = np.sort(D, 1)
        if case["expect"] is None:
            share = float((srt[:, 1] - srt[:, 0] > 4 * bnd).mean())
            assert share >= 0.9, (case["name"], share)
        else:                                                # the designed ties ARE ties in fp32 and in float64, and they lead the row
            assert (srt[:, 0] == srt[:, 1]).all() and (srt[:, 2] - srt[:, 0] > 40).all()
            assert (np.argmin(D, 1) == case["expect"]).all()


def test_tables_reference_matches_the_oracles_irfft():
    M = R.dft_table_ref()
    assert M.shape == (1280, 1312) and (M[:, 1282:] == 0).all() and (M[:, 641] == 0).all() and (M[:, 1281] == 0).all()
    S = torch.zeros(641, dtype=torch.complex128)
    S[7], S[640], S[0] = 1.0 + 2.0j, 3.0, -1.5
    want = torch.fft.irfft(S, 1280, norm="backward").numpy() * R.hann_tables()[0]
    reim = np.zeros(1312)
    reim[7], reim[641 + 7], reim[640], reim[0] = 1.0, 2.0, 3.0, -1.5
    _close(M @ reim, want, 1e-14)


# ---- every bound bites: wrong kernels fail the GPU test's assertion on the GPU test's inputs ---------------------------------------
MUTANTS = [("codebook_sum", "descending"),
           ("im2col7", "taps_reversed"), ("im2col7", "leak"),
           ("dwconv7", "taps_reversed"), ("dwconv7", "w_tap_major"), ("dwconv7", "leak"),
           ("istft_prep", "no_clip"), ("istft_prep", "clip_before_exp"),
           ("overlap_add", "env_short"), ("overlap_add", "trim_160"), ("overlap_add", "trim_800"),
           ("im2col_seq", "edge"), ("im2col_seq", "no_zero_extend"), ("im2col_seq", "leak"), ("im2col_seq", "elu_fp32"),
           ("final_conv", "edge"), ("final_conv", "no_zero_extend"), ("final_conv", "taps_reversed"), ("final_conv", "w_tap_major"),
           ("final_conv", "leak"),
           ("enc_first_conv", "edge"), ("enc_first_conv", "no_zero_extend"), ("enc_first_conv", "taps_reversed"), ("enc_first_conv", "w_tap_major"),
           ("enc_pad_elu", "edge"), ("enc_pad_elu", "no_zero_extend"), ("enc_pad_elu", "elu_fp32")]


def _rejected(kernel, case, mutant):
    ref, bound = R.expected(kernel, case)
    wrong, _ = R.expected(kernel, case, mutant)
    try:
        R.check(R.as_kernel_output(wrong), ref, bound, case["name"])
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("kernel,mutant", MUTANTS)
def test_wrong_kernel_fails_the_check(kernel, mutant):
    hit = [c["name"] for c in _cases(kernel) if _rejected(kernel, c, mutant)]
    print(kernel, mutant, "rejected on", len(hit), "cases, e.g.", hit[:3])
    assert hit, f"no input of the GPU test tells a {mutant} {kernel} from the right one"
    if mutant == "leak" and kernel == "im2col_seq":      # at a border of both modes
        assert any("mode=0" in n for n in hit) and any("mode=1" in n for n in hit)
    if mutant in ("edge", "no_zero_extend", "leak", "taps_reversed", "w_tap_major") and kernel in ("dwconv7", "final_conv", "enc_first_conv"):
        assert any(n.startswith("one-hot") for n in hit) and any(n.startswith("random") for n in hit)


def test_elu_bound_rejects_exp_minus_one_at_small_negative_inputs():
    """the evidence that the expm1f allowance is tight: at x = -1e-3 (part of every ELU input of the GPU test) exp(x) - 1 in fp32 is
    ~2^-24 off, a few hundred times the bound"""
    x = np.array([[-1e-3, -1e-6, -20.0, 0.5]], f32)
    ref, bound = R.elu64(x), R.elu_bound(x)
    wrong = R.elu64(x, "elu_fp32")
    over = np.abs(wrong - ref) / np.maximum(bound, 1e-300)
    print("exp(x) - 1 in fp32: err / bound at -1e-3, -1e-6:", over[0, 0], over[0, 1])
    assert over[0, 0] > 10 and over[0, 1] > 10 and R.check(R.as_kernel_output(ref), ref, bound, "elu") <= 1.0
    for case in R.enc_pad_elu_cases() + R.im2col_seq_cases(32)[1::2] + [c for c in R.final_conv_cases() if c["name"].startswith("random")]:
        assert (case["kw"]["x"] == f32(-1e-3)).any(), case["name"]


@pytest.mark.parametrize("mutant", ["gate_order", "skip_added"])
def test_wrong_lstm_cell_fails_the_check(mutant):
    hit = 0
    for case in R.lstm_cell_cases():
        refs, bounds = R.lstm_cell_ref(**case["kw"])
        wrong, _ = R.lstm_cell_ref(**case["kw"], mutant=mutant, mutant_skip=case["spare_skip"])
        try:
            for ref, bound, w in zip(refs, bounds, wrong):
                R.check(R.as_kernel_output(w), ref, bound, case["name"])
        except AssertionError:
            hit += 1
    print(mutant, "rejected on", hit, "of", len(R.lstm_cell_cases()))
    assert hit == (len(R.lstm_cell_cases()) if mutant == "gate_order" else len(R.lstm_cell_cases()) // 2)     # skip_added: the cases without a skip


def _rvq_kernel(kw, highest=False):
    """an fp32 evaluation of the select: (codes, resid_out) as the entry returns them"""
    rows = len(kw["resid"])
    a = (kw["resid"].astype(f32) ** 2).sum(1, dtype=f32)[:, None]
    d = -((a - f32(2) * kw["scores"]) + kw["e2"][None])
    code = 1023 - np.argmax(d[:, ::-1], 1) if highest else np.argmax(d, 1)
    code[np.isnan(kw["scores"]).all(1)] = 0
    codes = np.full((rows + kw["extra"], 8), R.SENT_L, np.int64)
    codes[:rows, kw["q"]] = code
    out = np.full((rows + kw["extra"], 128), R.SENT_F, f32)
    out[:rows] = kw["resid"] - kw["codebook"][code]
    return codes, out


def test_rvq_check_accepts_fp32_and_rejects_wrong_selects():
    for case in R.rvq_cases() + [R.rvq_nan_case()]:
        kw = case["kw"]
        codes, out = _rvq_kernel(kw)
        R.rvq_check(codes, out, name=case["name"], expect=case["expect"], **kw)
        if case["expect"] is not None:                       # tie resolved to the highest index
            with pytest.raises(AssertionError, match="lowest index"):
                R.rvq_check(*_rvq_kernel(kw, highest=True), name=case["name"], expect=case["expect"], **kw)
    kw = R.rvq_nan_case()["kw"]
    codes, out = _rvq_kernel(kw)
    bad = codes.copy()
    bad[2, kw["q"]] = 1024                                   # what the kernel wrote before it was fixed
    with pytest.raises(AssertionError):
        R.rvq_check(bad, out, name="nan", **kw)
    bad = codes.copy()
    bad[0, (kw["q"] + 1) % 8] = 5                            # a code in another column
    with pytest.raises(AssertionError, match="outside column"):
        R.rvq_check(bad, out, name="column", **kw)
    bad = codes.copy()
    bad[1, kw["q"]] = (codes[1, kw["q"]] + 1) % 1024         # not the nearest codeword (the residual follows it)
    out2 = out.copy()
    out2[1] = kw["resid"][1] - kw["codebook"][bad[1, kw["q"]]]
    with pytest.raises(AssertionError, match="further from the minimum"):
        R.rvq_check(bad, out2, name="argmin", **kw)
