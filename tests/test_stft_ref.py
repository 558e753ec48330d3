"""The long-double reference of dsc_stft / dsc_istft and the per-frame / per-sample error bounds the GPU tests of
tests/test_gpu_stft_routes.py hold every short-time route to.  CPU only: the tests here pin the references against the f64 numpy
restatement of tests/test_stft_abi.py and against torch in f64, run numpy's own f32 / f64 transforms through the same framing and
overlap-add to show how much room the bounds leave, and plant four defects that a whole-array rel-L2 of 1e-5 lets through and
the per-frame / per-sample bounds reject.

Forward: every frame is one line of a real transform, so stft_err is the per-line bound of tests/test_fft_ref.py (fft_err) with
the frame as the line: the fused route is the register kernels behind dsc_rfft plus one multiply by the window.

Inverse: output sample p = sum_f w_j v_f[j] / sum_f w_j^2, j = p - f hop, over the frames f that cover p, v_f the irfft of frame f.
Each v_f[j] obeys the per-element irfft bound  tau (8 ||v_f||_2 / sqrt(n) + |v_f[j]| + max |v_f| / 8); carried through the sum,
    bound_p = sum_f |w_j| (8 ||v_f||_2 / sqrt(n) + |v_f[j]| + max |v_f| / 8) / sum_f w_j^2
and istft_err = max_p |y_p - ref_p| / (tau bound_p).  The sum itself has at most ceil(n / hop) terms; its own rounding (a few eps of
sum |w_j v_f[j]| / env) is far inside the first term.  tau is the project's TAU of the plain transforms, unchanged."""
import numpy as np
import pytest

from tests.test_fft_ref import TAU, fft_err, real_of
from tests.test_stft_abi import np_istft, np_stft

assert np.finfo(np.longdouble).eps < 1e-18, 'the STFT reference needs a long double wider than f64'

LD, CLD = np.longdouble, np.clongdouble
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)


def _window(window, n_fft):
    return np.ones(n_fft, LD) if window is None else np.asarray(window).astype(LD)


def _pad(x, n_fft, center, pad_mode):
    if not center:
        return x
    assert pad_mode in ('reflect', 'constant')
    return np.pad(x, [(0, 0)] * (x.ndim - 1) + [(n_fft // 2, n_fft // 2)], mode=pad_mode)


def ref_stft(x, n_fft, hop, window=None, center=True, pad_mode='reflect'):
    """dsc_stft in long double, from x and window exactly as passed: [.., T] -> [.., n_frames, n_fft / 2 + 1] (frames-major)"""
    x = _pad(np.asarray(x).astype(LD), n_fft, center, pad_mode)
    n_frames = 1 + (x.shape[-1] - n_fft) // hop
    idx = np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :]
    y = np.fft.rfft(x[..., idx] * _window(window, n_fft), axis=-1)
    assert y.dtype == CLD, y.dtype
    return y


def stft_err(y, ref, tau):
    """largest per-frame ratio of the error to the bound of fft_err (<= 1 passes); a frame whose reference is all zero must be
    exactly zero"""
    return fft_err(y, ref, -1, tau)


def ref_istft(X, n_fft, hop, window=None, center=True, length=None):
    """dsc_istft in long double, from X and window exactly as passed: [.., n_frames, n_fft / 2 + 1] -> (y, bound), both [.., length].
    The imaginary parts of bins 0 and n_fft / 2 are dropped; the output is cropped by n_fft / 2 when centred, trimmed to `length`
    and zero past the last frame, where bound is zero too.  bound: see the module docstring."""
    X = np.asarray(X).astype(CLD).copy()
    assert X.shape[-1] == n_fft // 2 + 1
    X[..., 0] = X[..., 0].real
    X[..., -1] = X[..., -1].real
    w = _window(window, n_fft)
    n_frames = X.shape[-2]
    v = np.fft.irfft(X, n_fft, axis=-1)
    assert v.dtype == LD, v.dtype
    nrm = np.sqrt(np.sum(v * v, axis=-1, keepdims=True))
    top = np.max(np.abs(v), axis=-1, keepdims=True)
    e = 8 * nrm / np.sqrt(LD(n_fft)) + np.abs(v) + top / 8
    expected = n_fft + hop * (n_frames - 1)
    y = np.zeros(X.shape[:-2] + (expected,), LD)
    b = np.zeros_like(y)
    env = np.zeros(expected, LD)
    for f in range(n_frames):
        y[..., f * hop:f * hop + n_fft] += v[..., f, :] * w
        b[..., f * hop:f * hop + n_fft] += e[..., f, :] * np.abs(w)
        env[f * hop:f * hop + n_fft] += w * w
    start = n_fft // 2 if center else 0
    end = start + length if length is not None else (expected - n_fft // 2 if center else expected)
    stop = min(end, expected)
    covered = env[start:stop] > 0                               # hop > n_fft leaves gaps: zero there, like past the last frame
    den = np.where(covered, env[start:stop], 1)
    y, b = np.where(covered, y[..., start:stop] / den, 0), np.where(covered, b[..., start:stop] / den, 0)
    if end > expected:
        tail = np.zeros(y.shape[:-1] + (end - expected,), LD)
        y, b = np.concatenate([y, tail], axis=-1), np.concatenate([b, tail], axis=-1)
    return y, b


def istft_err(y, ref, bound, tau):
    """max_p |y_p - ref_p| / (tau bound_p) (<= 1 passes); a sample whose bound is zero (past the last frame, or frames that are
    all zero) must be exactly zero"""
    y = np.asarray(y)
    assert y.shape == ref.shape == bound.shape, (y.shape, ref.shape, bound.shape)
    d = np.abs(y.astype(LD) - ref)
    zero = bound == 0
    if np.any(zero):
        assert not np.any(d[zero]), 'nonzero output where the reference is exactly zero'
    if np.all(zero):
        return 0.0
    return float(np.max(d[~zero] / (tau * bound[~zero])))


def rel_l2(a, b):
    """the whole-array yardstick the planted defects get past"""
    a, b = np.asarray(a).astype(CLD).ravel(), np.asarray(b).astype(CLD).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def rand_window(rng, n_fft, dt):
    """the asymmetric window of the GPU tests"""
    return rng.uniform(0.2, 1.8, n_fft).astype(dt)


def hann(n_fft, dt):
    """periodic Hann"""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)).astype(dt)


def rand_spectrum(rng, shape, cdt, spice=True):
    """random complex frames, not the stft of a signal, with nonzero imaginary parts in bins 0 and n_fft / 2; row 1 carries a
    strong bin 0 (a DC offset of 20 in every frame)"""
    X = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    if spice and len(shape) >= 3 and shape[-3] >= 2:
        X[..., 1, :, 0] += 20 * 2 * (shape[-1] - 1)
    return X.astype(cdt)


# working-precision pipelines: numpy's own f32 / f64 transforms through the same framing and overlap-add
def work_stft(x, n_fft, hop, window, center, pad_mode):
    dt = x.dtype
    w = np.ones(n_fft, dt) if window is None else window
    xp = _pad(x, n_fft, center, pad_mode)
    n_frames = 1 + (xp.shape[-1] - n_fft) // hop
    idx = np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :]
    y = np.fft.rfft((xp[..., idx] * w).astype(dt), axis=-1)
    assert real_of(y.dtype) == dt
    return y


def work_istft(X, n_fft, hop, window, center, length):
    dt = real_of(X.dtype).type
    w = np.ones(n_fft, dt) if window is None else window
    n_frames = X.shape[-2]
    v = np.fft.irfft(X, n_fft, axis=-1)
    assert v.dtype == dt
    expected = n_fft + hop * (n_frames - 1)
    y, env = np.zeros(X.shape[:-2] + (expected,), dt), np.zeros(expected, dt)
    for f in range(n_frames):
        y[..., f * hop:f * hop + n_fft] += v[..., f, :] * w
        env[f * hop:f * hop + n_fft] += w * w
    start = n_fft // 2 if center else 0
    end = start + length if length is not None else (expected - n_fft // 2 if center else expected)
    stop = min(end, expected)
    y = (y[..., start:stop] / env[start:stop]).astype(dt)
    if end > expected:
        y = np.concatenate([y, np.zeros(y.shape[:-1] + (end - expected,), dt)], axis=-1)
    return y


def odd_hop(n_fft):
    """the odd hop of the route tests: 3 up to 256, 125 up to 4096, n / 8 + 1 above"""
    return 3 if n_fft <= 256 else 125 if n_fft <= 4096 else n_fft // 8 + 1


# ---------------------------------------------------------------------------------------------------- the references themselves

CASES = [(64, 16, True, 'reflect', 'hann'), (64, 16, True, 'constant', 'rand'), (256, 3, False, 'reflect', 'rand'),
         (32, 64, True, 'reflect', None), (128, 125, True, 'constant', 'rand'), (4, 1, True, 'reflect', 'rand'),
         (1024, 256, False, 'reflect', None)]


def _win(kind, rng, n_fft, dt):
    return None if kind is None else hann(n_fft, dt) if kind == 'hann' else rand_window(rng, n_fft, dt)


@pytest.mark.parametrize('n_fft,hop,center,pad_mode,win', CASES)
def test_references_match_numpy_restatement_and_torch(n_fft, hop, center, pad_mode, win):
    """ref_stft / ref_istft against np_stft / np_istft (the oracle of tests/test_gpu_stft.py) and torch.stft / torch.istft in f64,
    to f64 rounding: a tenth of the f64 bound.  length: natural, shorter, and longer than the last frame reaches (zero tail)."""
    torch = pytest.importorskip('torch')
    rng = np.random.default_rng([n_fft, hop])
    tau = TAU[F64]
    w = _win(win, rng, n_fft, np.float64)
    wt = torch.ones(n_fft, dtype=torch.float64) if w is None else torch.from_numpy(w)
    x = rng.standard_normal((2, 3, 3 * n_fft + 5))
    x[0, 1] += 20
    ref = ref_stft(x, n_fft, hop, w, center, pad_mode)
    assert stft_err(np_stft(x, n_fft, hop, w, center, pad_mode), ref, tau) <= 0.2
    t = torch.stft(torch.from_numpy(x.reshape(6, -1)), n_fft, hop, window=wt, center=center, pad_mode=pad_mode, return_complex=True)
    assert stft_err(t.transpose(-2, -1).numpy().reshape(ref.shape), ref, tau) <= 0.2
    if hop > n_fft:
        return                                                      # NOLA fails: no inverse
    X = rand_spectrum(rng, (2, 3, 7, n_fft // 2 + 1), np.complex128)
    expected = n_fft + hop * 6
    natural = expected - n_fft if center else expected
    for length in (None, natural - min(5, natural - 1), expected + 2 * hop + 1):
        want, bound = ref_istft(X, n_fft, hop, w, center, length)
        assert want.shape == (2, 3, natural if length is None else length)
        assert istft_err(np_istft(X, n_fft, hop, w, center, length), want, bound, tau) <= 0.1
        Xr = X.copy()                                               # torch rejects nothing here but reads the imaginary parts as given
        Xr[..., 0] = Xr[..., 0].real
        Xr[..., -1] = Xr[..., -1].real
        ti = torch.istft(torch.from_numpy(Xr.reshape(6, 7, -1)).transpose(-2, -1), n_fft, hop, window=wt, center=center, length=length)
        assert istft_err(ti.numpy().reshape(want.shape), want, bound, tau) <= 0.1
        if length is not None and length > natural:
            assert not np.any(want[..., expected - (n_fft // 2 if center else 0):]) and np.any(want[..., :natural])


def test_zero_frames_and_the_zero_tail_must_be_exact():
    ref = np.zeros((3, 5), CLD)
    ref[1] = 1
    y = ref.astype(np.complex64)
    assert stft_err(y, ref, 2e-6) == 0
    y[2, 4] = 1e-30
    with pytest.raises(AssertionError):
        stft_err(y, ref, 2e-6)
    X = rand_spectrum(np.random.default_rng(0), (2, 9), np.complex64)
    want, bound = ref_istft(X, 16, 4, None, False, 40)
    assert np.all(bound[:20] > 0) and not np.any(bound[20:]) and not np.any(want[20:])
    y = want.astype(np.float32)
    assert istft_err(y, want, bound, 2e-6) <= 0.1
    y[33] = 1e-30
    with pytest.raises(AssertionError):
        istft_err(y, want, bound, 2e-6)


def test_istft_drops_the_imaginary_parts_of_bins_0_and_half():
    rng = np.random.default_rng(5)
    X = rand_spectrum(rng, (3, 4, 17), np.complex128)
    Y = X.copy()
    Y[..., 0] = Y[..., 0].real
    Y[..., -1] = Y[..., -1].real
    assert np.any(X[..., 0].imag) and np.any(X[..., -1].imag)
    a, b = ref_istft(X, 32, 8), ref_istft(Y, 32, 8)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------- room under the bounds

# numpy's own working-precision transforms through the same framing / overlap-add, over n_fft 64 .. 32768, hops n / 4, n and odd,
# no / random / Hann windows and rows with a DC offset of 20, reach 0.03 (stft f32), 0.17 (stft f64) and 0.04 (istft, both) of the
# bounds; the limits here leave the draw of another seed some room above those figures.  They are about numpy, not about a kernel.
WORK_MAX = {('stft', F32): 0.05, ('stft', F64): 0.25, ('istft', F32): 0.06, ('istft', F64): 0.06}


@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('n_fft', [64, 512, 4096, 32768])
def test_working_precision_pipelines_sit_far_inside_the_bounds(n_fft, dt):
    rng = np.random.default_rng([n_fft, dt.itemsize])
    cdt = np.complex64 if dt == F32 else np.complex128
    tau = TAU[dt]
    for hop in (n_fft // 4, n_fft, odd_hop(n_fft)):
        for center, pad_mode in ((True, 'reflect'), (True, 'constant'), (False, 'reflect')):
            for win in (None, 'rand', 'hann'):
                if n_fft == 32768 and (win == 'hann') != (pad_mode == 'constant'):
                    continue                                        # the longest length: each option once
                x = rng.standard_normal((3, 3 * n_fft + 7)).astype(dt)
                x[1] += 20
                w = _win(win, rng, n_fft, dt)
                r = stft_err(work_stft(x, n_fft, hop, w, center, pad_mode), ref_stft(x, n_fft, hop, w, center, pad_mode), tau)
                assert r <= WORK_MAX['stft', dt], ('stft', n_fft, hop, center, pad_mode, win, r)
                if win == 'hann' and (hop == n_fft or not center):
                    continue                                        # NOLA fails
                X = rand_spectrum(rng, (2, 9, n_fft // 2 + 1), cdt)
                for length in (None, max(1, hop * 8 - 5), n_fft + hop * 8 + 11):
                    want, bound = ref_istft(X, n_fft, hop, w, center, length)
                    r = istft_err(work_istft(X, n_fft, hop, w, center, length), want, bound, tau)
                    assert r <= WORK_MAX['istft', dt], ('istft', n_fft, hop, center, win, length, r)


# ---------------------------------------------------------------------------------------------------- the bounds are tight enough

def test_bound_rejects_one_wrong_bin_of_one_frame():
    """One bin of one of 1026 frames off by 50 tau ||frame||: 50 tau / sqrt(1026) = 3e-6 of the whole array, 50x the frame's bound."""
    rng = np.random.default_rng(31)
    n_fft, hop, tau = 64, 16, TAU[F32]
    x = rng.standard_normal((2, 8192)).astype(np.float32)
    want = ref_stft(x, n_fft, hop)
    assert want.shape[0] * want.shape[1] >= 500
    got = want.astype(np.complex64)
    assert stft_err(got, want, tau) <= 0.1
    bad = got.astype(CLD)
    bad[1, 300, 7] += 50 * tau * np.linalg.norm(want[1, 300])
    assert rel_l2(bad, want) < 1e-5
    assert stft_err(bad, want, tau) > 10


def test_bound_rejects_a_reflected_sample_from_the_wrong_side():
    """The last frame of the last row reads one sample past the end from the wrong side: x[k] (the rule of the left edge, -i)
    where 2 (T - 1) - i gives x[T - 1 - k].  The row is built so that the two differ by 1e-3 — a whole-array rel-L2 of 1e-5 can
    only miss a defect that small: over 1026 frames of 64 samples it is 4e-6, in its own frame 60x the bound."""
    rng = np.random.default_rng(32)
    n_fft, hop, tau, k = 64, 16, TAU[F32], 25
    x = rng.standard_normal((2, 8192)).astype(np.float32)
    T = x.shape[-1]
    x[1, k] = x[1, T - 1 - k] + np.float32(1e-3)
    w = rand_window(rng, n_fft, np.float32)
    want = ref_stft(x, n_fft, hop, w)
    xp = _pad(x.astype(LD), n_fft, True, 'reflect')
    assert xp[1, n_fft // 2 + T - 1 + k] == x[1, T - 1 - k]
    xp[1, n_fft // 2 + T - 1 + k] = x[1, k]                          # only the last frame reaches it: k > n_fft / 2 - hop
    n_frames = want.shape[-2]
    idx = np.arange(n_frames)[:, None] * hop + np.arange(n_fft)[None, :]
    bad = np.fft.rfft(xp[..., idx] * w.astype(LD), axis=-1)
    assert np.array_equal(bad[0], want[0]) and np.array_equal(bad[1, :-1], want[1, :-1]) and not np.array_equal(bad[1, -1], want[1, -1])
    assert rel_l2(bad, want) < 1e-5
    assert stft_err(bad, want, tau) > 10


def _ola(v, w, hop, skip=None, env_from=None):
    """overlap-add of frames v [F, n] under window w in long double, without crop; skip = (p, f): sample p is summed without frame f;
    env_from = (p, q): sample p is divided by the envelope of sample q"""
    n_frames, n = v.shape
    expected = n + hop * (n_frames - 1)
    y, env = np.zeros(expected, LD), np.zeros(expected, LD)
    for f in range(n_frames):
        t = v[f] * w
        if skip is not None and skip[1] == f:
            t = t.copy()
            t[skip[0] - f * hop] = 0
        y[f * hop:f * hop + n] += t
        env[f * hop:f * hop + n] += w * w
    den = env.copy()
    if env_from is not None:
        den[env_from[0]] = env[env_from[1]]
    with np.errstate(invalid='ignore'):                          # a Hann window without centre: 0 / 0 at the ends, outside the slices compared
        return y / den


def test_bound_rejects_a_sample_summed_without_its_last_frame():
    """One output sample is summed without the last frame that covers it, where that frame's Hann weight is small (j = 4 .. 12 of
    1024: w_j <= 1.4e-3): 1e-6 of the whole array, several times the sample's bound."""
    rng = np.random.default_rng(33)
    n_fft, hop, tau = 1024, 256, TAU[F32]
    X = rand_spectrum(rng, (48, n_fft // 2 + 1), np.complex64)
    w = hann(n_fft, np.float32)
    want, bound = ref_istft(X, n_fft, hop, w, False)
    s = slice(n_fft, want.shape[-1] - n_fft)                         # away from the ends, where the envelope is small
    assert istft_err(want.astype(np.float32)[s], want[s], bound[s], tau) <= 0.1
    Xr = X.astype(CLD)
    Xr[..., 0], Xr[..., -1] = Xr[..., 0].real, Xr[..., -1].real
    v = np.fft.irfft(Xr, n_fft, axis=-1)
    f = 20
    j = 4 + int(np.argmax(np.abs(v[f, 4:13])))
    p = f * hop + j                                                  # frames 17 .. 20 cover it, 20 is the last
    bad = _ola(v, w.astype(LD), hop, skip=(p, f))
    assert np.array_equal(np.delete(bad[s], p - s.start), np.delete(want[s], p - s.start)) and bad[p] != want[p]
    whole, r = rel_l2(bad[s], want[s]), istft_err(bad[s], want[s], bound[s], tau)
    print('whole-array', whole, 'per-sample', r)
    assert whole < 1e-5
    assert r > 1.5


def test_bound_rejects_a_sample_divided_by_its_neighbours_envelope():
    """One sample divided by the squared-window envelope of the sample next to it, under an asymmetric window.  With a window like
    uniform(0.2, 1.8) neighbouring envelopes differ by tens of percent, and a whole-array rel-L2 of 1e-5 would need 1e9 samples to
    miss that; the window here is 1 + 2e-4 uniform(-1, 1), whose envelope changes by about 1e-4 from one sample to the next: a few
    1e-6 of the whole array, several times the sample's bound."""
    rng = np.random.default_rng(34)
    n_fft, hop, tau = 1024, 256, TAU[F32]
    X = rand_spectrum(rng, (48, n_fft // 2 + 1), np.complex64)
    w = (1 + 2e-4 * rng.uniform(-1, 1, n_fft)).astype(np.float32)
    assert not np.allclose(w[1:], w[:0:-1])                         # asymmetric
    want, bound = ref_istft(X, n_fft, hop, w, False)
    s = slice(n_fft, want.shape[-1] - n_fft)
    assert istft_err(want.astype(np.float32)[s], want[s], bound[s], tau) <= 0.1
    Xr = X.astype(CLD)
    Xr[..., 0], Xr[..., -1] = Xr[..., 0].real, Xr[..., -1].real
    v = np.fft.irfft(Xr, n_fft, axis=-1)
    lo = 20 * hop + 300
    p = lo + int(np.argmax(np.abs(want[lo:lo + 64])))
    bad = _ola(v, w.astype(LD), hop, env_from=(p, p + 1))
    assert np.array_equal(np.delete(bad[s], p - s.start), np.delete(want[s], p - s.start)) and bad[p] != want[p]
    whole, r = rel_l2(bad[s], want[s]), istft_err(bad[s], want[s], bound[s], tau)
    print('whole-array', whole, 'per-sample', r)
    assert whole < 1e-5
    assert r > 1.5
