"""Float64 references, derived error bounds and the shared inputs of the waveform glue-kernel tests (tests/test_gpu_kernel_wave.py runs
the kernels of csrc/vocos.hip and csrc/encodec.hip one launch at a time through vx_dev_wave_op; tests/test_wave_refs.py pins what is
here to the oracles on the CPU and shows that every bound rejects a wrong kernel).

The references restate the REFERENCE's arithmetic (EncodecConv1d._pad1d as in oracle/encodec_oracle.py, torch.nn.LSTM, the Vocos
ISTFT head as in oracle/vallex_oracle.py), not the kernels' index arithmetic.  A reference returns (ref, bound): float64 arrays of
the shape of the kernel's output buffer INCLUDING the rows behind its end; ref is NaN where the kernel must write nothing (the
sentinel must survive), bound is the largest |kernel - ref| the derivation below allows.  bound == 0 means bit-identical to
float32(ref): pure data movement, single fp32 operations, positions that hold a zero of the padding.

Bounds (u = 2^-24, gamma_n = n u / (1 - n u), ulp32(v) = the spacing of fp32 at |v|, 2^-149 at the bottom):
  * short fp32 accumulations: |err| <= gamma_n * sum |terms|, n = the roundings on the longest path of a term (one product, then
    every add behind it): DWCONV7 7 adds + the bias add + 1 = 9, ENC_FIRST_CONV 7 + 1 = 8, FINAL_CONV 224 + 1 = 225, OVERLAP_ADD 4
    per sum (numerator and envelope) and one division, pushed through the quotient.  A fused multiply-add only removes roundings.
  * device math functions: the result of f is within ULPS[f] ulp32 of the true value, then propagated in float64 through the rest of
    the formula (value, error) pair by pair, plus half an ulp32 of the result for every fp32 operation.
    ULPS: the accuracy table of the HIP math API was looked for under the ROCm installation's documentation (share/doc/hip holds the
    runtime API's HTML only; no file there or under share/doc/rocm-device-libs states a ulp figure), so the values are the OpenCL
    full-profile limits as remembered -- expf / expm1f 3, sinf / cosf 4, tanhf 5 -- and are NOT verified against a document here.
    They are not tuned to any kernel output.
"""
import numpy as np

U = 2.0 ** -24
ULPS = {"expf": 3, "expm1f": 3, "sinf": 4, "cosf": 4, "tanhf": 5}
SENT_F = np.float32(-1.0e30)
SENT_L = -1234567890123456789
FLT_MAX = float(np.finfo(np.float32).max)
f32, f64 = np.float32, np.float64


def gamma(n):
    return n * U / (1 - n * U)


def ulp32(v):
    a = np.abs(np.asarray(v, f64))
    e = np.frexp(a)[1]                                   # a = m 2^e, m in [0.5, 1)
    return np.where(a < 2.0 ** -126, 2.0 ** -149, np.ldexp(1.0, e - 24))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def as_kernel_output(ref):
    """what a kernel that computed `ref` exactly would leave in the buffer: float32(ref), the sentinel where ref is NaN"""
    with np.errstate(over="ignore", invalid="ignore"):
        out = np.asarray(ref, f64).astype(f32)
    out[np.isnan(ref)] = SENT_F
    return out


def check(got, ref, bound, name):
    """THE assertion of the GPU tests: every element of `got` (float32) is within bound of ref; bit-identical to float32(ref) where
    bound == 0; the sentinel where ref is NaN.  Returns the worst err / bound over the elements with a bound > 0."""
    got = np.asarray(got)
    assert got.dtype == f32 and got.shape == ref.shape == bound.shape, (name, got.dtype, got.shape, ref.shape, bound.shape)
    assert np.isfinite(bound).all() and (bound >= 0).all(), name
    want = as_kernel_output(ref)
    exact = np.isnan(ref) | (bound == 0)
    bad = exact & (bits(got) != bits(want))
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{name}: element {i} is {got[i]!r}, must be exactly {want[i]!r} ({int(bad.sum())} such elements)")
    loose = ~exact
    if not loose.any():
        return 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got[loose].astype(f64) - ref[loose])
    err[np.isnan(err)] = np.inf
    ratio = err / bound[loose]
    k = int(np.argmax(ratio))
    if ratio[k] > 1.0:
        i = tuple(int(v) for v in np.argwhere(loose)[k])
        raise AssertionError(f"{name}: element {i}: got {got[i]!r}, reference {ref[i]!r}, error {err[k]:.3e} > bound {bound[i]:.3e} "
                             f"({int((ratio > 1).sum())} elements over their bound)")
    return float(ratio[k])


# ---------------------------------------------------------------------------------------------------------------------------------
# shared pieces
# ---------------------------------------------------------------------------------------------------------------------------------
def rows_of_seqs(lens):
    """(row_t, row_len, seq_off) of sequences packed back to back"""
    row_t = np.concatenate([np.arange(n) for n in lens] + [np.zeros(0, int)]).astype(np.int32)
    row_len = np.concatenate([np.full(n, n) for n in lens] + [np.zeros(0, int)]).astype(np.int32)
    return row_t, row_len, np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)


def seqs_of_rows(row_t, row_len):
    return [(r, int(row_len[r])) for r in range(len(row_t)) if row_t[r] == 0]


def pad1d(x, left, right, mode="reflect", zero_extend=True):
    """EncodecConv1d._pad1d along axis 0: reflect padding; an input not longer than the larger pad is zero-extended first and the
    extension cut off again.  mode "edge" / zero_extend False are the wrong kernels of the mutation tests."""
    L, extra = x.shape[0], 0
    if mode == "reflect" and zero_extend and L <= max(left, right):
        extra = max(left, right) - L + 1
        x = np.concatenate([x, np.zeros((extra,) + x.shape[1:], x.dtype)])
    y = np.pad(x, ((left, right),) + ((0, 0),) * (x.ndim - 1), mode=mode)
    return y[: y.shape[0] - extra]


def _left_context(full, base, n, seg, mutant, left):
    """the padded copy of sequence rows `seg` = full[base : base + n] with `left` rows in front, as the reference pads it (per sequence,
    reflect) or as a wrong kernel would"""
    if mutant == "leak":                                 # the rows in front of the sequence in the PACKED buffer leak in
        ctx = full[max(0, base - left): base]
        ctx = np.concatenate([np.zeros((left - len(ctx),) + full.shape[1:], full.dtype), ctx])
        return np.concatenate([ctx, seg])
    return pad1d(seg, left, 0, mode="edge" if mutant == "edge" else "reflect", zero_extend=mutant != "no_zero_extend")


def _windows(xp, k, T, reverse=False):
    taps = range(k - 1, -1, -1) if reverse else range(k)
    return np.concatenate([xp[tap: tap + T] for tap in taps], axis=1)


def elu64(x, mutant=None):
    x = np.asarray(x, f64)
    if mutant == "elu_fp32":                             # exp(x) - 1 in fp32: loses the small negative inputs
        x32 = x.astype(f32)
        return np.where(x > 0, x, (np.exp(x32) - f32(1)).astype(f64))
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def elu_bound(x):
    x = np.asarray(x, f64)
    return np.where(x > 0, 0.0, ULPS["expm1f"] * ulp32(np.expm1(np.minimum(x, 0))))


# (value, error) arithmetic in float64: every function returns the exact result of the exact operands and a bound on
# |fp32 result of operands within their errors - that|
def _rnd(v):
    return 0.5 * ulp32(v)


def _add(a, ea, b, eb):
    v = a + b
    e = ea + eb
    return v, e + _rnd(np.abs(v) + e)


def _mul(a, ea, b, eb):
    v = a * b
    e = np.abs(a) * eb + np.abs(b) * ea + ea * eb
    return v, e + _rnd(np.abs(v) + e)


def _sigmoid(g, eg):
    """1.0f / (1.0f + expf(-g))"""
    with np.errstate(over="ignore"):
        ex = np.exp(-g)
        e_ex = ex * np.expm1(eg) + ULPS["expf"] * ulp32(ex * np.exp(eg))
    d, e_d = _add(1.0, 0.0, ex, e_ex)
    s = 1.0 / d
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e_s = e_d / (d * np.maximum(d - e_d, 1.0)) + _rnd(s)
    # expf overflows to +Inf in fp32 (1 / Inf = 0) or the divisor does: the kernel may return 0 for a true value below 2^-126
    over = (ex * np.exp(eg) * (1 + ULPS["expf"] * 2.0 ** -23) >= FLT_MAX) | ~np.isfinite(e_s)
    return s, np.where(over, s + 2.0 ** -149, e_s)


def _tanh(x, ex):
    t = np.tanh(x)
    return t, ex + ULPS["tanhf"] * ulp32(np.abs(t) + ex)     # |tanh'| <= 1


# ---------------------------------------------------------------------------------------------------------------------------------
# Vocos head (csrc/vocos.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def codebook_sum_ref(codes, codebook, extra, mutant=None):
    """vocos codes_to_features: embedding(codes + 1024 q).sum(dim = 0), fp32, q ascending"""
    rows = len(codes)
    order = range(7, -1, -1) if mutant == "descending" else range(8)
    acc = None
    for q in order:
        v = codebook[1024 * q + codes[:, q]].astype(f32)
        acc = v if acc is None else (acc + v).astype(f32)
    ref = np.full((rows + extra, 128), np.nan)
    ref[:rows] = acc
    return ref, np.zeros_like(ref)


def im2col7_ref(x, row_t, row_len, extra, mutant=None):
    """rows of the im2col of Conv1d(128, 384, k = 7, padding = 3): zeros outside the row's own sequence"""
    rows, C = x.shape
    ref = np.full((rows + extra, 7 * C), np.nan)
    x64 = x.astype(f64)
    if mutant == "leak":
        ref[:rows] = _windows(np.pad(x64, ((3, 3), (0, 0))), 7, rows)
    else:
        for off, n in seqs_of_rows(row_t, row_len):
            ref[off: off + n] = _windows(np.pad(x64[off: off + n], ((3, 3), (0, 0))), 7, n, reverse=mutant == "taps_reversed")
    return ref, np.zeros_like(ref)


def im2col_weight(w):
    """Conv1d weight (O, C, k) -> the GEMM operand [O][tap C + c] that goes with im2col rows"""
    return np.ascontiguousarray(np.transpose(w, (0, 2, 1))).reshape(w.shape[0], -1)


def dwconv7_ref(x, w, bias, row_t, row_len, extra, exact=False, mutant=None):
    """depthwise Conv1d(C, C, k = 7, padding = 3, groups = C): w is (C, 7) = weight[:, 0, :]"""
    rows, C = x.shape
    x64, w64 = x.astype(f64), w.astype(f64)
    if mutant == "w_tap_major":
        w64 = w64.reshape(-1).reshape(7, C).T            # reads w[tap][c] where the layout is w[c][tap]
    if mutant == "taps_reversed":
        w64 = w64[:, ::-1]
    ref = np.full((rows + extra, C), np.nan)
    mag = np.zeros_like(ref)
    seqs = [(0, rows)] if mutant == "leak" else seqs_of_rows(row_t, row_len)
    for off, n in seqs:
        win = _windows(np.pad(x64[off: off + n], ((3, 3), (0, 0))), 7, n).reshape(n, 7, C)
        ref[off: off + n] = bias.astype(f64) + np.einsum("ntc,ct->nc", win, w64)
        mag[off: off + n] = np.abs(bias.astype(f64)) + np.einsum("ntc,ct->nc", np.abs(win), np.abs(w64))
    return ref, np.zeros_like(ref) if exact else gamma(9) * mag


LN100 = f32(np.log(100.0))


def istft_prep_ref(o, extra, mutant=None):
    """ISTFTHead front: mag = clip(exp(o[:641]), max = 100), S = mag (cos p + i sin p) -> [re | im | zero pad] of 1312 columns"""
    rows = len(o)
    x, p = o[:, :641].astype(f64), o[:, 641:1282].astype(f64)
    with np.errstate(over="ignore"):
        ex = np.exp(np.minimum(x, 100.0)) if mutant == "clip_before_exp" else np.exp(x)
    m = ex if mutant in ("no_clip", "clip_before_exp") else np.minimum(ex, 100.0)
    # expf within ULPS of exp(x); min(., 100) is a contraction, and an exp(x) >= 128 clips to exactly 100 on both sides
    e_m = np.where(ex >= 128.0, 0.0, ULPS["expf"] * ulp32(np.minimum(ex, 128.0)))
    ref = np.full((rows + extra, 1312), np.nan)
    bound = np.zeros_like(ref)
    ref[:rows] = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for col, (t, name) in enumerate(((np.cos(p), "cosf"), (np.sin(p), "sinf"))):
            ref[:rows, 641 * col: 641 * (col + 1)], bound[:rows, 641 * col: 641 * (col + 1)] = _mul(m, e_m, t, ULPS[name] * ulp32(t))
    return ref, bound


def hann_tables():
    """(window as fp32 values in float64, win2 float32): torch.hann_window(1280) (periodic) and its square, rounded in the order
    csrc/weights.hip states: float32(float32(hann)^2 formed in double)"""
    n = np.arange(1280)
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * n / 1280)).astype(f32).astype(f64)
    return win, (win * win).astype(f32)


def overlap_add_ref(frames, seq_off, seq_len, win2, stride, extra, mutant=None):
    """ISTFT tail, padding = "same": fold the windowed frames (kernel 1280, hop 320), trim 480 on both sides, divide by the folded
    hann^2 envelope.  stride 0: the audio is packed like the frames."""
    hop, nfft = 320, 1280
    pad = {"trim_160": 160, "trim_800": 800}.get(mutant, 480)
    n_audio = (len(seq_off) * stride if stride else len(frames) * hop) + extra
    ref = np.full(n_audio, np.nan)
    bound = np.zeros(n_audio)
    fr, w2 = frames.astype(f64), win2.astype(f64)
    for b, (off, T) in enumerate(zip(seq_off, seq_len)):
        if T == 0:
            continue
        size = (T - 1) * hop + nfft
        y, ay, env = np.zeros(size), np.zeros(size), np.zeros(size)
        for f in range(T):
            y[f * hop: f * hop + nfft] += fr[off + f]
            ay[f * hop: f * hop + nfft] += np.abs(fr[off + f])
            if not (mutant == "env_short" and f == T - 1):
                env[f * hop: f * hop + nfft] += w2
        sl = slice(pad, pad + T * hop)
        y, ay, env = (np.pad(v, (0, 400))[sl] for v in (y, ay, env))
        start = b * stride if stride else off * hop
        with np.errstate(divide="ignore", invalid="ignore"):
            ref[start: start + T * hop] = y / env
            # numerator A (1 + t4) with |error| <= gamma_4 sum |f|, envelope E (1 + t4') (positive terms), one rounding of the quotient
            num = np.abs(y) + gamma(4) * ay
            bound[start: start + T * hop] = (gamma(4) * ay + (gamma(4) + U) * num / (1 - gamma(4))) / env
    return ref, bound


def overlap_add_exact(frames, seq_off, seq_len, win2, stride, extra):
    """the same in fp32 with the kernel's stated order of additions (frames ascending) and one correctly rounded division: the
    exact probes (small integers or the window itself in the frames: every sum is exact or formed of the same addends)"""
    hop, nfft = 320, 1280
    n_audio = (len(seq_off) * stride if stride else len(frames) * hop) + extra
    ref = np.full(n_audio, np.nan)
    for b, (off, T) in enumerate(zip(seq_off, seq_len)):
        if T == 0:
            continue
        size = (T - 1) * hop + nfft
        y, env = np.zeros(size, f32), np.zeros(size, f32)
        for f in range(T):
            y[f * hop: f * hop + nfft] += frames[off + f].astype(f32)
            env[f * hop: f * hop + nfft] += win2
        start = b * stride if stride else off * hop
        ref[start: start + T * hop] = (y[480: 480 + T * hop] / env[480: 480 + T * hop]).astype(f64)
    return ref, np.zeros(n_audio)


def dft_table_ref():
    """the [1280][1312] matrix frame = spectrum . M^T of the windowed inverse real DFT (irfft, n = 1280, norm "backward"), column by
    column from numpy's irfft of a unit spectrum"""
    win, _ = hann_tables()
    M = np.zeros((1280, 1312))
    eye = np.eye(641)
    M[:, :641] = np.fft.irfft(eye, n=1280, axis=1).T * win[:, None]
    M[:, 641:1282] = np.fft.irfft(1j * eye, n=1280, axis=1).T * win[:, None]
    return M


# ---------------------------------------------------------------------------------------------------------------------------------
# EnCodec (csrc/encodec.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def im2col_seq_ref(x, C, k, mode, elu, seq_off, seq_len, R, extra, mutant=None):
    """mode 0: rows of the im2col of a causal EncodecConv1d(k) (left pad k - 1, reflect, _pad1d) on every sequence; mode 1: rows
    [x[t] | x[t - 1]] of a ConvTranspose1d(k = 2 r, stride r) (x[-1] = 0).  Sequence b owns rows [seq_off R, (seq_off + seq_len) R)."""
    rows = len(x)
    act = elu64(x, mutant) if elu else x.astype(f64)
    eb = elu_bound(x) if elu else np.zeros(x.shape)
    ref = np.full((rows + extra, k * C), np.nan)
    bound = np.zeros_like(ref)
    left = k - 1 if mode == 0 else 1
    for off, n in zip(seq_off, seq_len):
        base, T = int(off) * R, int(n) * R
        if T == 0:
            continue
        for dst, src in ((ref, act), (bound, eb)):
            if mode == 0:
                xp = _left_context(src, base, T, src[base: base + T], mutant, left)
                dst[base: base + T] = _windows(xp, k, T)
            else:
                xp = _left_context(src, base, T, src[base: base + T], "leak", 1) if mutant == "leak" else np.pad(src[base: base + T], ((1, 0), (0, 0)))
                dst[base: base + T] = np.concatenate([xp[1:], xp[:-1]], axis=1)
    return ref, bound


def convtr_weight(w, r):
    """ConvTranspose1d weight (Cin, Cout, 2 r) -> the GEMM operand [(p, o)][tap Cin + c] = w[c][o][p + tap r]: the [T][r Cout] product of
    mode-1 im2col rows with it, read as [T r][Cout], is the transposed conv trimmed by r on the right"""
    cin, cout, _ = w.shape
    return np.ascontiguousarray(np.transpose(w.reshape(cin, cout, 2, r), (3, 1, 2, 0))).reshape(r * cout, 2 * cin)


def lstm_cell_ref(part, splitk, xg, seq_off, seq_len, t, cstate, h, skip, batch, extra, mutant=None, mutant_skip=None):
    """one step of torch.nn.LSTM (gate order i, f, g, o) for the sequences with t < seq_len: gates = xg[row] + sum of the split-K
    slabs of h_{t-1} W_hh^T; c = sigmoid(f) c + sigmoid(i) tanh(g), h = sigmoid(o) tanh(c), y[row] = h (+ skip[row]).
    Returns ((c, h, y) references, (c, h, y) bounds); finished sequences keep c and h bit for bit, their y rows are not written."""
    HD = cstate.shape[1]
    c_ref, h_ref = cstate.astype(f64), h.astype(f64)
    c_b, h_b = np.zeros_like(c_ref), np.zeros_like(h_ref)
    y_ref = np.full((len(xg) + extra, HD), np.nan)
    y_b = np.zeros_like(y_ref)
    order = (0, 2, 1, 3) if mutant == "gate_order" else (0, 1, 2, 3)     # where i, f, g, o are read from
    for b in range(batch):
        if t >= seq_len[b]:
            continue
        row = int(seq_off[b]) + t
        g, e = [], []
        for q in order:
            v, ev = part[0, b, q * HD: (q + 1) * HD].astype(f64), 0.0
            for ks in range(1, splitk):
                v, ev = _add(v, ev, part[ks, b, q * HD: (q + 1) * HD].astype(f64), 0.0)
            v, ev = _add(xg[row, q * HD: (q + 1) * HD].astype(f64), 0.0, v, ev)
            g.append(v)
            e.append(ev)
        (si, esi), (sf, esf), (so, eso) = _sigmoid(g[0], e[0]), _sigmoid(g[1], e[1]), _sigmoid(g[3], e[3])
        tg, etg = _tanh(g[2], e[2])
        c, ec = _add(*_mul(sf, esf, cstate[b].astype(f64), 0.0), *_mul(si, esi, tg, etg))
        hh, eh = _mul(so, eso, *_tanh(c, ec))
        c_ref[b], c_b[b], h_ref[b], h_b[b] = c, ec, hh, eh
        sk = skip if skip is not None else (mutant_skip if mutant == "skip_added" else None)
        y_ref[row], y_b[row] = (hh, eh) if sk is None else _add(hh, eh, sk[row].astype(f64), 0.0)
    return (c_ref, h_ref, y_ref), (c_b, h_b, y_b)


def final_conv_ref(x, w, bias, seq_off, seq_len, R, stride, extra, exact=False, mutant=None):
    """last decoder layer: ELU -> causal EncodecConv1d(32, 1, k = 7): w is (32, 7) = weight[0]"""
    K, C = 7, 32
    w64 = w.astype(f64)
    if mutant == "w_tap_major":
        w64 = w64.reshape(-1).reshape(K, C).T
    if mutant == "taps_reversed":
        w64 = w64[:, ::-1]
    act, eb = elu64(x, mutant), elu_bound(x)
    ref = np.full(len(seq_off) * stride + extra, np.nan)
    bound = np.zeros_like(ref)
    for b, (off, n) in enumerate(zip(seq_off, seq_len)):
        base, T = int(off) * R, int(n) * R
        if T == 0:
            continue
        win = _windows(_left_context(act, base, T, act[base: base + T], mutant, K - 1), K, T).reshape(T, K, C)
        wb = _windows(_left_context(eb, base, T, eb[base: base + T], mutant, K - 1), K, T).reshape(T, K, C)
        ref[b * stride: b * stride + T] = float(bias[0]) + np.einsum("tkc,ck->t", win, w64)
        e_in = np.einsum("tkc,ck->t", wb, np.abs(w64))                 # what the ELU's error contributes
        mag = abs(float(bias[0])) + np.einsum("tkc,ck->t", np.abs(win), np.abs(w64)) + e_in
        bound[b * stride: b * stride + T] = 0.0 if exact else gamma(K * C + 1) * mag + e_in
    return ref, bound


def enc_first_conv_ref(wav, w, bias, extra, exact=False, mutant=None):
    """first encoder layer: causal EncodecConv1d(1, 32, k = 7): w is (32, 7) = weight[:, 0, :]"""
    L, K = len(wav), 7
    w64 = w.astype(f64)
    if mutant == "w_tap_major":
        w64 = w64.reshape(-1).reshape(K, 32).T
    if mutant == "taps_reversed":
        w64 = w64[:, ::-1]
    x = wav.astype(f64)[:, None]
    win = _windows(_left_context(x, 0, L, x, mutant, K - 1), K, L)     # (L, 7)
    ref = np.full((L + extra, 32), np.nan)
    bound = np.zeros_like(ref)
    ref[:L] = bias.astype(f64) + win @ w64.T
    if not exact:
        bound[:L] = gamma(K + 1) * (np.abs(bias.astype(f64)) + np.abs(win) @ np.abs(w64).T)
    return ref, bound


def enc_pad_geom_ref(Lc, r):
    """EncodecConv1d(k = 2 r, stride r), causal: (rows of the padded input, length after the zero extension of _pad1d, output frames)"""
    k, pad_total = 2 * r, r
    n_frames = int(np.ceil((Lc - k + pad_total) / r + 1)) - 1                    # _get_extra_padding_for_conv1d
    extra = n_frames * r + k - pad_total - Lc
    Le = Lc + (max(pad_total, extra) - Lc + 1) if Lc <= max(pad_total, extra) else Lc
    return Lc + pad_total + extra, Le, n_frames + 1


def enc_pad_elu_ref(x, r, out_rows, mutant=None):
    """ELU, then the padding of the causal strided conv: left k - stride = r, right what completes the last frame, both reflect"""
    Lc = len(x)
    rows, _, n_out = enc_pad_geom_ref(Lc, r)
    right = n_out * r - Lc
    ref = np.full((out_rows, x.shape[1]), np.nan)
    bound = np.zeros_like(ref)
    kw = dict(mode="edge" if mutant == "edge" else "reflect", zero_extend=mutant != "no_zero_extend")
    ref[:rows] = pad1d(elu64(x, mutant), r, right, **kw)
    bound[:rows] = pad1d(elu_bound(x), r, right, **kw)
    return ref, bound


def rvq_distances(resid, scores, e2):
    """float64 distances |r|^2 - 2 s_c + |e_c|^2 of the kernel's own operands and the bound on the fp32 evaluation of one of them:
    |r|^2 is a product and an 8-level tree of adds (gamma_9), then two more roundings: (a - 2 s) and (. + e2)"""
    a = (resid.astype(f64) ** 2).sum(1, keepdims=True)
    D = a - 2.0 * scores.astype(f64) + e2.astype(f64)[None]
    mag = a * (1 + gamma(9)) + 2.0 * np.abs(scores.astype(f64)) + np.abs(e2.astype(f64))[None]
    return D, (gamma(2) * mag + gamma(9) * a).max(1)


def rvq_check(codes, resid_out, resid, scores, e2, codebook, q, extra, name, expect=None):
    """codes (rows + extra, 8) int64, resid_out (rows + extra, 128): column q only is written, in 0 .. 1023; the chosen code's float64
    distance is within twice the bound of the minimum, and IS the float64 argmin where the runner-up is further away than that (a row
    of NaN scores: code 0); expect (rows,) >= 0: the code a designed exact tie must give; the residual update is one fp32 subtraction.
    Returns (worst (D[code] - min) / (2 bound), rows decided by their gap)."""
    rows = len(resid)
    others = np.delete(codes, q, axis=1)
    assert (others == SENT_L).all() and (codes[rows:] == SENT_L).all(), f"{name}: a code outside column {q} or behind the rows was written"
    got = codes[:rows, q]
    assert ((got >= 0) & (got < 1024)).all(), (name, got[(got < 0) | (got >= 1024)])
    D, bnd = rvq_distances(resid, scores, e2)
    nanrow = np.isnan(scores).all(1)
    assert (got[nanrow] == 0).all(), f"{name}: a row without a comparable distance must get code 0, got {got[nanrow]}"
    live = ~nanrow
    srt = np.sort(D[live], axis=1)
    best = np.argmin(D[live], axis=1)
    over = (D[live, :][np.arange(live.sum()), got[live]] - srt[:, 0]) / (2 * bnd[live])
    assert (over <= 1.0).all(), (name, "chosen code further from the minimum than the bound", float(over.max()))
    clear = srt[:, 1] - srt[:, 0] > 2 * (2 * bnd[live])
    assert (got[live][clear] == best[clear]).all(), (name, "not the float64 argmin at a clear gap", np.argwhere(got[live][clear] != best[clear])[:4])
    if expect is not None:
        m = expect >= 0
        assert (got[m] == expect[m]).all(), (name, "exact tie not resolved to the lowest index", got[m], expect[m])
    want = np.full((rows + extra, 128), np.nan)
    want[:rows] = (resid - codebook[got]).astype(f32)
    check(resid_out, want, np.zeros_like(want), name + ": residual update")
    return float(over.max()) if live.any() else 0.0, int(clear.sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests (shared with the CPU mutation tests): lists of dicts; "kw" are the keyword arguments of the reference
# ---------------------------------------------------------------------------------------------------------------------------------
EXTRA = 3
RAGGED = [1, 2, 3, 4, 7, 8, 20]


def _ints(rows, C):
    """row * C + c: every element names its own place (exact in fp32: below 2^24)"""
    assert rows * C < 2 ** 24
    return (np.arange(rows * C).reshape(rows, C)).astype(f32)


def _normals(rng, shape, small=True):
    """standard normals with the values an ELU path must get right sprinkled in: small negatives, zero, large of both signs"""
    x = rng.standard_normal(shape).astype(f32)
    if small:
        flat = x.reshape(-1)
        special = np.array([-1e-3, -1e-6, 0.0, -0.0, -20.0, -104.0, 15.0, 1e-3], f32)
        idx = rng.permutation(flat.size)[: min(flat.size // 2, 4 * len(special))]
        flat[idx] = special[np.arange(len(idx)) % len(special)]
    return x


def codebook_sum_cases():
    out = []
    for rows in (1, 7, 8, 9, 65):
        rng = np.random.default_rng(100 + rows)
        codes = rng.integers(0, 1024, (rows, 8)).astype(np.int32)
        codes[0] = [0, 1023] * 4
        codes[-1] = [1023, 0] * 4
        cb = rng.standard_normal((8192, 128)).astype(f32)
        out.append(dict(name=f"random rows={rows}", kw=dict(codes=codes, codebook=cb, extra=EXTRA)))
        # order matters: 1e8, -1e8, 1, ... across the levels -- only ((1e8 - 1e8) + 1) + ... in ascending q gives the count of ones
        cb2 = np.empty((8192, 128), f32)
        for q, v in enumerate((1e8, -1e8, 1, 1, 1, 1, 1, 1)):
            cb2[1024 * q: 1024 * (q + 1)] = v
        out.append(dict(name=f"order rows={rows}", kw=dict(codes=codes, codebook=cb2, extra=EXTRA)))
    return out


def im2col7_cases():
    row_t, row_len, _ = rows_of_seqs(RAGGED)
    return [dict(name="ragged ints", kw=dict(x=_ints(len(row_t), 128) + 1, row_t=row_t, row_len=row_len, extra=EXTRA))]


def dwconv7_cases():
    out = []
    row_t, row_len, _ = rows_of_seqs(RAGGED)
    rows = len(row_t)
    for C in (384, 512):
        rng = np.random.default_rng(C)
        c = np.arange(C)
        w1 = np.zeros((C, 7), f32)
        w1[c, c % 7] = 1                                     # one-hot taps: out[r][c] = x[r + c % 7 - 3][c] + bias[c], exact
        out.append(dict(name=f"one-hot C={C}", kw=dict(x=_ints(rows, C) + 1, w=w1, bias=(c % 5).astype(f32), row_t=row_t, row_len=row_len,
                                                       extra=EXTRA, exact=True)))
        out.append(dict(name=f"random C={C}", kw=dict(x=_normals(rng, (rows, C), False), w=rng.standard_normal((C, 7)).astype(f32),
                                                      bias=rng.standard_normal(C).astype(f32), row_t=row_t, row_len=row_len, extra=EXTRA)))
    return out


def istft_prep_cases():
    out = []
    for rows in (1, 3):
        rng = np.random.default_rng(7 + rows)
        o = np.full((rows, 1408), 1e30, f32)                 # the pad columns 1282 .. 1407 must influence nothing
        x = rng.uniform(-10, 5, (rows, 641)).astype(f32)
        special = np.array([-104.0, np.nextafter(LN100, f32(0)), LN100, np.nextafter(LN100, f32(9)), 89.0, 0.0, 4.7, 4.5, 88.0, -87.0,
                            -20.0], f32)
        x[:, : len(special)] = special
        x[:, -len(special):] = special[::-1]
        p = rng.uniform(-1e4, 1e4, (rows, 641)).astype(f32)
        p[:, 100:200] = rng.uniform(-4, 4, (rows, 100)).astype(f32)
        while True:                                          # |cos p|, |sin p| >= 2^-10 keeps the relative bound meaningful
            bad = (np.abs(np.cos(p.astype(f64))) < 2.0 ** -10) | (np.abs(np.sin(p.astype(f64))) < 2.0 ** -10)
            if not bad.any():
                break
            p[bad] = rng.uniform(-1e4, 1e4, int(bad.sum())).astype(f32)
        p[:, 2] = 0.0                                        # the exact point: cos 0 = 1, sin 0 = 0, at the magnitude of the clip
        p[:, 300] = 0.0
        o[:, :641], o[:, 641:1282] = x, p
        out.append(dict(name=f"rows={rows}", kw=dict(o=o, extra=EXTRA)))
    return out


def overlap_add_cases(win2):
    out = []
    lens = [1, 2, 3, 4, 5, 9]
    _, _, seq_off = rows_of_seqs(lens)
    frames_n = sum(lens)
    rng = np.random.default_rng(11)
    probes = {"window": (np.broadcast_to(win2, (frames_n, 1280)).copy(), True),
              "frame index": (np.broadcast_to(np.arange(1, frames_n + 1, dtype=f32)[:, None], (frames_n, 1280)).copy(), True),
              "random": (rng.standard_normal((frames_n, 1280)).astype(f32), False)}
    for stride in (0, 9 * 320 + 7):
        for name, (fr, exact) in probes.items():
            out.append(dict(name=f"{name} stride={stride}", exact=exact,
                            kw=dict(frames=fr, seq_off=seq_off, seq_len=np.array(lens, np.int32), win2=win2, stride=stride, extra=EXTRA)))
    return out


def im2col_seq_cases(C):
    out = []
    lens = np.array([1, 2, 0, 3, 5, 8], np.int32)            # a sequence of length 0 between two live ones; T R < k for R = 1
    _, _, seq_off = rows_of_seqs(lens)
    for mode, k in ((0, 3), (0, 7), (1, 2)):
        for R in (1, 8):
            rows = int(lens.sum()) * R
            for elu in (0, 1):
                rng = np.random.default_rng(1000 * C + 100 * k + 10 * R + elu)
                x = _normals(rng, (rows, C)) if elu else _ints(rows, C) + 1
                out.append(dict(name=f"C={C} mode={mode} k={k} R={R} elu={elu}",
                                kw=dict(x=x, C=C, k=k, mode=mode, elu=elu, seq_off=seq_off, seq_len=lens, R=R, extra=EXTRA)))
    return out


def im2col_seq_big_case():
    """C = 512, k = 7, one sequence of 1200 rows: 1200 x 896 float4 > 4096 x 256, the launch's grid-stride loop runs"""
    assert 1200 * (7 * 512 // 4) > 4096 * 256
    return dict(name="grid-stride C=512 k=7 rows=1200",
                kw=dict(x=_ints(1200, 512) + 1, C=512, k=7, mode=0, elu=0, seq_off=np.zeros(1, np.int32), seq_len=np.array([1200], np.int32), R=1,
                        extra=EXTRA))


LSTM_SPECIAL = np.array([0.0, 30.0, -30.0, 100.0, -100.0, 88.0, -88.0, 1e-3], f32)


def lstm_cell_cases():
    out = []
    HD, t = 512, 3
    for batch in (1, 2, 32):
        # t = 3: lengths 4 (t = len - 1), 9 (t < len), 3 and 1 (finished), 0 (never started); two sequences: a finished one and its live neighbour
        lens = np.array({1: [4], 2: [3, 4]}.get(batch, [4, 9, 3, 1, 0, 4, 3, 9] * 4), np.int32)
        _, _, seq_off = rows_of_seqs(lens)
        frames = int(lens.sum()) + 2
        for splitk in (1, 2):
            for with_skip in (False, True):
                rng = np.random.default_rng(10000 + 100 * batch + 10 * splitk + with_skip)
                part = rng.standard_normal((2, 32, 4 * HD)).astype(f32)
                xg = (2 * rng.standard_normal((frames, 4 * HD))).astype(f32)
                for q in range(4):                           # chosen pre-activations: the slabs hold 0 there, xg the value
                    part[:, :, q * HD: q * HD + 64] = 0
                    xg[:, q * HD: q * HD + 64] = np.roll(np.tile(LSTM_SPECIAL, 8), q)
                if splitk == 1:
                    part[1] = 1e30                           # must not be read
                out.append(dict(name=f"batch={batch} splitk={splitk} skip={with_skip}", with_skip=with_skip,
                                spare_skip=rng.standard_normal((frames, HD)).astype(f32),
                                kw=dict(part=part, splitk=splitk, xg=xg, seq_off=seq_off, seq_len=lens, t=t,
                                        cstate=rng.standard_normal((32, HD)).astype(f32), h=rng.standard_normal((32, HD)).astype(f32),
                                        skip=rng.standard_normal((frames, HD)).astype(f32) if with_skip else None, batch=batch, extra=EXTRA)))
    return out


def final_conv_cases():
    out = []
    lens = np.array([2, 1, 2], np.int32)                     # ragged batch of 3: R, 2 R samples
    _, _, seq_off = rows_of_seqs(lens)
    for R in (1, 4, 320):
        rows = int(lens.sum()) * R
        stride = 2 * R + 5
        rng = np.random.default_rng(50 + R)
        for c, tap in ((0, 0), (31, 6), (5, 3)):
            w1 = np.zeros((32, 7), f32)
            w1[c, tap] = 1
            out.append(dict(name=f"one-hot ({c}, {tap}) R={R}", kw=dict(x=_ints(rows, 32), w=w1, bias=np.array([2.0], f32), seq_off=seq_off, seq_len=lens,
                                                                       R=R, stride=stride, extra=EXTRA, exact=True)))
        out.append(dict(name=f"random R={R}", kw=dict(x=_normals(rng, (rows, 32)), w=rng.standard_normal((32, 7)).astype(f32),
                                                      bias=rng.standard_normal(1).astype(f32), seq_off=seq_off, seq_len=lens, R=R, stride=stride,
                                                      extra=EXTRA)))
    return out


def enc_first_conv_cases():
    out = []
    c = np.arange(32)
    w1 = np.zeros((32, 7), f32)
    w1[c, c % 7] = 1
    for L in (1, 5, 6, 7, 8, 255, 256, 257, 600):
        rng = np.random.default_rng(70 + L)
        out.append(dict(name=f"one-hot L={L}", kw=dict(wav=np.arange(1, L + 1, dtype=f32), w=w1, bias=(c % 3).astype(f32), extra=EXTRA, exact=True)))
        out.append(dict(name=f"random L={L}", kw=dict(wav=rng.standard_normal(L).astype(f32), w=rng.standard_normal((32, 7)).astype(f32),
                                                      bias=rng.standard_normal(32).astype(f32), extra=EXTRA)))
    return out


def enc_pad_elu_cases():
    out = []
    for r, C in ((2, 32), (4, 64), (5, 128), (8, 256)):
        for Lc in sorted({1, 2, 3, r - 1, r, r + 1, 2 * r - 1, 2 * r, 2 * r + 1, 5 * r + 3}):
            rng = np.random.default_rng(1000 * r + Lc)
            x = _normals(rng, (Lc, C))
            x[x == 0] = -1e-3                                # an input zero would be indistinguishable from a zero of the padding
            out.append(dict(name=f"r={r} C={C} Lc={Lc}", kw=dict(x=x, r=r, out_rows=enc_pad_geom_ref(Lc, r)[0] + EXTRA)))
    return out


def rvq_cases():
    out = []
    for rows in (1, 3, 300):
        for q in (0, 7):
            rng = np.random.default_rng(900 + 10 * rows + q)
            cb = (0.5 * rng.standard_normal((1024, 128))).astype(f32)
            resid = (0.5 * rng.standard_normal((rows, 128))).astype(f32)
            scores = (resid.astype(f64) @ cb.astype(f64).T).astype(f32)
            e2 = (cb.astype(f64) ** 2).sum(1).astype(f32)
            out.append(dict(name=f"random rows={rows} q={q}", kw=dict(resid=resid, scores=scores, e2=e2, codebook=cb, q=q, extra=EXTRA), expect=None))
    # designed exact ties of the best distance: equal (score, e2) pairs in one thread (i, i + 256), in neighbouring threads (i, i + 1),
    # half a block apart (i, i + 128), at the two ends of the reduction tree (0, 1023)
    pairs = [(5, 261), (300, 556), (767, 1023), (9, 10), (255, 256), (63, 64), (17, 145), (640, 768), (0, 1023), (0, 512), (1022, 1023), (511, 767)]
    for q in (0, 7):
        rng = np.random.default_rng(990 + q)
        rows = len(pairs)
        cb = (0.5 * rng.standard_normal((1024, 128))).astype(f32)
        resid = (0.5 * rng.standard_normal((rows, 128))).astype(f32)
        scores = rng.standard_normal((rows, 1024)).astype(f32)
        e2 = rng.uniform(20, 40, 1024).astype(f32)
        # e2 is shared by the rows of a launch: the indices any pair uses get one common value, so that every row's pair ties exactly
        e2[np.unique(np.array(pairs))] = 25.0
        for r, (i, j) in enumerate(pairs):
            scores[r, [i, j]] = 50.0                         # far in front of every other candidate
        out.append(dict(name=f"ties q={q}", kw=dict(resid=resid, scores=scores, e2=e2, codebook=cb, q=q, extra=EXTRA),
                        expect=np.array([min(p) for p in pairs])))
    return out


def rvq_nan_case():
    c = rvq_cases()[0]
    rng = np.random.default_rng(77)
    cb = c["kw"]["codebook"]
    resid = (0.5 * rng.standard_normal((5, 128))).astype(f32)
    scores = (resid.astype(f64) @ cb.astype(f64).T).astype(f32)
    scores[2] = np.nan
    return dict(name="NaN row", kw=dict(resid=resid, scores=scores, e2=c["kw"]["e2"], codebook=cb, q=7, extra=EXTRA), expect=None)


REFS = {"codebook_sum": codebook_sum_ref, "im2col7": im2col7_ref, "dwconv7": dwconv7_ref, "istft_prep": istft_prep_ref,
        "overlap_add": overlap_add_ref, "im2col_seq": im2col_seq_ref, "final_conv": final_conv_ref, "enc_first_conv": enc_first_conv_ref,
        "enc_pad_elu": enc_pad_elu_ref}


def expected(kernel, case, mutant=None):
    """(ref, bound) of a single-output kernel on a case; with `mutant`, what that wrong kernel would compute"""
    if kernel == "overlap_add" and case.get("exact") and mutant is None:
        return overlap_add_exact(**case["kw"])
    kw = dict(case["kw"])
    if mutant is not None:
        kw.pop("exact", None)
        return REFS[kernel](**kw, mutant=mutant)
    return REFS[kernel](**kw)
