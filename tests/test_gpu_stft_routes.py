"""GPU tests of dsc_stft / dsc_istft on every route of stft.cpp (stft_regs at each of its lengths, stft_composed, istft_ola over
every irfft route underneath), every frame and every output sample against the long-double references of tests/test_stft_ref.py:
    forward   per frame   ||y - ref||_2 <= tau ||ref||_2,   |y_k - ref_k| <= tau (8 ||ref||_2 / sqrt(bins) + |ref_k| + max |ref| / 8)
    inverse   per sample  |y_p - ref_p| <= tau sum_f |w_j| (8 ||v_f||_2 / sqrt(n) + |v_f[j]| + max |v_f| / 8) / sum_f w_j^2
with the project's TAU (2e-6 f32, 5e-15 f64).  Every case asserts dsc.last_fft_path(), checks that the input (and the window) is
left bit for bit unchanged, and repeats the call with out= the start of a larger sentinel-filled buffer: the result must be
bit-identical and nothing past it may change.  Every ratio is recorded (record_property); profiles/stft_routes_err.md keeps the maxima.

Inputs: standard normal rows, row 1 with a DC offset of 20, row 2 with a strong tone at bin 5 of the frame; windows none, random
asymmetric uniform(0.2, 1.8) and (inverse) periodic Hann; T = 3 n_fft + 7 (odd, so the rows of a batch start on even and odd elements
in turn: direct pair loads and the sample-by-sample gather both run on interior frames).  Inverse spectra are random complex frames
with nonzero imaginary parts in bins 0 and n_fft / 2, not the stft of a signal.

Sizes kept down for the host reference, whose long-double transforms are the cost of a case: above n_fft 4096 the odd hop is
n / 8 + 1 (at most about 30 frames per row); at 262144 (forward) and from 131072 (inverse) signals are n_fft + n_fft / 2 + 7 long /
spectra have 5 frames instead of 9, and the batch shapes are [.], [2, .] and [1, 2, .]."""
import numpy as np
import pytest

from tests.helpers import CPX, F32, F64, assert_out_call, dsc, run_child, sync_fixture  # noqa: F401
from tests.test_fft_ref import TAU, real_of
from tests.test_stft_ref import hann, istft_err, odd_hop, rand_spectrum, rand_window, ref_istft, ref_stft, stft_err

pytestmark = pytest.mark.gpu

FUSED = tuple(1 << k for k in range(6, 16))                                                 # 64 .. 32768: dsc_stft_regs_supports
COMPOSED = (4, 8, 16, 32, 65536, 262144)
INVERSE = tuple(1 << k for k in range(2, 19))                                               # 4 .. 262144

# Lines (frames) per workgroup of the fused instantiations, restated from fft_regs_mid.hip: n_fft 64 .. 512 run fft_small_kernel with
# G = small_cfg<R, R2C_PACKED>::NT / B (B = n_fft / 64 threads per line; NT = DSC_SMALL_NT_F32 / DSC_SMALL_NT_F64 = 128), n_fft 1024 ..
# 32768 run fft_mid_kernel with G = mid_cfg<R, B, TWO>::G = NT / T (frames never take the persistent one-line form).
GROUP = {64: (128, 128), 128: (64, 64), 256: (32, 32), 512: (16, 16), 1024: (8, 16), 2048: (4, 4), 4096: (4, 2), 8192: (2, 1),
         16384: (2, 1), 32768: (1, 1)}                                                       # n_fft: (f32, f64)
_sync = sync_fixture()


# ---------------------------------------------------------------------------------------------------- inputs and checks

def make_signal(rng, shape, dt, n_fft):
    x = rng.standard_normal(shape)
    v = x.reshape(-1, shape[-1])
    if v.shape[0] >= 2:
        v[1] += 20
    if v.shape[0] >= 3:
        v[2] += 20 * np.cos(2 * np.pi * min(5, n_fft // 4) * np.arange(shape[-1]) / n_fft)
    return np.ascontiguousarray(x.astype(dt))


def make_window(kind, rng, n_fft, dt):
    return None if kind is None else hann(n_fft, dt) if kind == 'hann' else rand_window(rng, n_fft, dt)


def stft_route(n_fft):
    return 'stft_regs' if 64 <= n_fft <= 32768 else 'stft_composed'


def run_stft(dsc, record_property, x, n_fft, hop, w, center, pad_mode, want_path=None, label=''):
    """dsc.stft on the GPU: the route, the input and the window left alone, every frame within the bound, and a second call into a
    sentinel-filled buffer.  Returns err / bound."""
    want_path = want_path or stft_route(n_fft)
    what = f'{want_path} n_fft={n_fft} hop={hop} {x.dtype} {x.shape} center={center} {pad_mode} window={w is not None} {label}'
    X = dsc.from_numpy(x)
    W = None if w is None else dsc.from_numpy(w)
    y = dsc.stft(X, n_fft, hop, W, center, pad_mode)
    path = dsc.last_fft_path()
    assert path == want_path, (what, path)
    yh = y.numpy()
    want = ref_stft(x, n_fft, hop, w, center, pad_mode)
    assert yh.shape == want.shape and yh.dtype == CPX[x.dtype], (what, yh.shape, yh.dtype, want.shape)
    assert X.numpy().tobytes() == x.tobytes(), f'{what}: the input changed'
    assert w is None or W.numpy().tobytes() == w.tobytes(), f'{what}: the window changed'
    del y

    def again(out):
        dsc.stft(X, n_fft, hop, W, center, pad_mode, out=out)
        assert dsc.last_fft_path() == want_path
    assert_out_call(dsc, again, yh.shape, yh.dtype, yh, what)
    r = stft_err(yh, want, TAU[x.dtype])
    record_property(f'{want_path}:stft:{n_fft}:{x.dtype}', r)
    print(f'{what}: err / bound = {r:.3g}')
    assert r <= 1, f'{what}: err / bound = {r:.3g}'
    return r


def run_istft(dsc, record_property, X, n_fft, hop, w, center, length, label=''):
    """dsc.istft on the GPU, as run_stft: every output sample within its bound, samples past the last frame exactly zero"""
    rdt = real_of(X.dtype)
    what = f'istft_ola n_fft={n_fft} hop={hop} {X.dtype} {X.shape} center={center} length={length} window={w is not None} {label}'
    Xt = dsc.from_numpy(X)
    W = None if w is None else dsc.from_numpy(w)
    y = dsc.istft(Xt, n_fft, hop, W, center, length)
    assert dsc.last_fft_path() == 'istft_ola', (what, dsc.last_fft_path())
    yh = y.numpy()
    want, bound = ref_istft(X, n_fft, hop, w, center, length)
    assert yh.shape == want.shape and yh.dtype == rdt, (what, yh.shape, yh.dtype, want.shape)
    assert Xt.numpy().tobytes() == X.tobytes(), f'{what}: the input changed'
    assert w is None or W.numpy().tobytes() == w.tobytes(), f'{what}: the window changed'
    del y

    def again(out):
        dsc.istft(Xt, n_fft, hop, W, center, length, out=out)
        assert dsc.last_fft_path() == 'istft_ola'
    assert_out_call(dsc, again, yh.shape, yh.dtype, yh, what)
    r = istft_err(yh, want, bound, TAU[rdt])
    record_property(f'istft_ola:istft:{n_fft}:{rdt}', r)
    print(f'{what}: err / bound = {r:.3g}')
    assert r <= 1, f'{what}: err / bound = {r:.3g}'
    return r


def _signal_len(n_fft):
    return 3 * n_fft + 7 if n_fft < 262144 else n_fft + n_fft // 2 + 7


def _shapes(n_fft, T):
    return [(T,), (3, T), (2, 3, T)] if n_fft < 262144 else [(T,), (2, T), (1, 2, T)]


# ---------------------------------------------------------------------------------------------------- (a) every length, forward

PADS = ((True, 'reflect'), (True, 'constant'), (False, 'reflect'))


def forward_configs(n_fft):
    """the fixed list of a length: {centre + reflect, centre + constant, no centre} x {no window, asymmetric} x {hop n / 4, odd hop},
    then hop n and hop 2 n + 1 (skipped samples); shapes [T], [3, T], [2, 3, T] in turn"""
    out = []
    for center, pad_mode in PADS:
        for win in (None, 'rand'):
            for hop in (max(1, n_fft // 4), odd_hop(n_fft)):
                out.append((hop, center, pad_mode, win))
    out.append((n_fft, True, 'reflect', 'rand'))
    out.append((2 * n_fft + 1, False, 'reflect', None))
    return out


def _forward_cases():
    return [(n, dt, i) for n in FUSED + COMPOSED for dt in (F32, F64) for i in range(len(forward_configs(n)))]


@pytest.mark.parametrize('n_fft,dt,i', _forward_cases(), ids=str)
def test_forward_every_length(dsc, record_property, n_fft, dt, i):
    hop, center, pad_mode, win = forward_configs(n_fft)[i]
    rng = np.random.default_rng([n_fft, dt.itemsize, i])
    T = _signal_len(n_fft)
    shape = _shapes(n_fft, T)[i % 3]
    x = make_signal(rng, shape, dt, n_fft)
    run_stft(dsc, record_property, x, n_fft, hop, make_window(win, rng, n_fft, dt), center, pad_mode)


# ---------------------------------------------------------------------------------------------------- (b) edges of the signal

@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('n_fft', FUSED)
def test_shortest_signals(dsc, record_property, n_fft, dt):
    """T = n / 2 + 1 with centre + reflect: frame 0 reflects at both ends and reaches the last reflected sample, 2 (T - 1); the
    frames after it lie on the right edge.  T = n without centre: one frame per row."""
    rng = np.random.default_rng([n_fft, dt.itemsize, 77])
    w = rand_window(rng, n_fft, dt)
    T = n_fft // 2 + 1
    for hop in (n_fft // 4, odd_hop(n_fft)):
        for win in (w, None):
            run_stft(dsc, record_property, make_signal(rng, (3, T), dt, n_fft), n_fft, hop, win, True, 'reflect', label='T=n/2+1')
    run_stft(dsc, record_property, make_signal(rng, (3, T), dt, n_fft), n_fft, odd_hop(n_fft), w, True, 'constant', label='T=n/2+1')
    for hop in (n_fft // 4, odd_hop(n_fft)):
        run_stft(dsc, record_property, make_signal(rng, (3, n_fft), dt, n_fft), n_fft, hop, w, False, 'reflect', label='T=n')
    run_stft(dsc, record_property, make_signal(rng, (n_fft,), dt, n_fft), n_fft, n_fft // 4, None, False, 'reflect', label='T=n')


@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('n_fft', FUSED)
def test_impulse_rows(dsc, record_property, n_fft, dt):
    """One unit impulse per row, at the ends of the signal, around n / 2 and around the starts f hop - n / 2 of the first three
    frames that begin inside the signal.  The long-double reference is the known answer (w_j e^{-2 pi i j k / n} in the frames
    that reach the impulse); frames it does not reach must be exactly zero (stft_err asserts that)."""
    rng = np.random.default_rng([n_fft, dt.itemsize, 78])
    hop = odd_hop(n_fft)
    T = 3 * n_fft + 7 if n_fft <= 4096 else n_fft + n_fft // 2 + 7        # the reference of ~20 rows stays small
    pos = [0, 1, n_fft // 2 - 1, n_fft // 2, T - 2, T - 1]
    starts = [f * hop - n_fft // 2 for f in range(T // hop + 1) if 0 <= f * hop - n_fft // 2 - 1]
    for s in starts[:3]:
        pos += [s - 1, s, s + 1]
    pos = sorted(set(p for p in pos if 0 <= p < T))
    assert len(pos) >= 12
    x = np.zeros((len(pos), T), dt)
    x[np.arange(len(pos)), pos] = 1
    w = rand_window(rng, n_fft, dt)
    for pad_mode in ('reflect', 'constant'):
        run_stft(dsc, record_property, x, n_fft, hop, w, True, pad_mode, label='impulses')
    want = ref_stft(x, n_fft, hop, w, True, 'constant')
    assert np.any(np.all(want == 0, axis=-1)) and np.any(want != 0)          # there are frames that must be exactly zero


# ---------------------------------------------------------------------------------------------------- (c) workgroup geometry

@pytest.mark.parametrize('dt', [F32, F64], ids=str)
@pytest.mark.parametrize('n_fft', FUSED)
def test_workgroup_geometry(dsc, record_property, n_fft, dt):
    """Line counts rows x n_frames of 1, G - 1, G + 1 and 2 G + 1 (G = frames per workgroup, GROUP above) built from 1, 2 or 3 frames
    per row and many rows, so that one group spans several rows and the last group is one line full or one line short; odd T."""
    G = GROUP[n_fft][0 if dt == F32 else 1]
    rng = np.random.default_rng([n_fft, dt.itemsize, 79])
    w = rand_window(rng, n_fft, dt)
    hop = odd_hop(n_fft)
    done = set()
    for lines in (1, G - 1, G + 1, 2 * G + 1):
        for nf in (1, 2, 3):
            if lines < 1 or lines % nf or (lines, nf) in done:
                continue
            done.add((lines, nf))
            rows = lines // nf
            # without centre: n_frames = 1 + (T - n) / hop;  centre, hop n: n_frames = 1 + T / n
            T = n_fft + (nf - 1) * hop + 1
            T += 1 - T % 2
            assert 1 + (T - n_fft) // hop == nf
            run_stft(dsc, record_property, make_signal(rng, (rows, T), dt, n_fft), n_fft, hop, w, False, 'reflect', label=f'lines={lines}')
            T = (nf - 1) * n_fft + n_fft - 1
            assert T % 2 == 1 and 1 + T // n_fft == nf
            run_stft(dsc, record_property, make_signal(rng, (rows, T), dt, n_fft), n_fft, n_fft, None, True, 'reflect', label=f'lines={lines}')
    assert {k for k, _ in done} == {k for k in (1, G - 1, G + 1, 2 * G + 1) if k >= 1}


# ---------------------------------------------------------------------------------------------------- (d) the switch

SWITCHED = r'''
import numpy as np
import dsc_amd as dsc
dsc.init(2 << 30, 1 << 30)
rng = np.random.default_rng(41)
for n, hop, dt in CASES:
    x = rng.standard_normal((3, n + n // 2 + 7)).astype(dt)
    x[1] += 20
    w = rng.uniform(0.2, 1.8, n).astype(dt)
    X = dsc.from_numpy(x)
    y = dsc.stft(X, n, hop, dsc.from_numpy(w))
    path = dsc.last_fft_path()
    assert X.numpy().tobytes() == x.tobytes()
    np.savez('%s/%d_%s.npz' % (OUT, n, dt), x=x, w=w, y=y.numpy())
    print('PATH', n, dt, path, flush=True)
dsc.synchronize()
'''


def test_switch_takes_the_composed_route_at_every_fused_length(record_property, tmp_path):
    """DSC_NO_STFT_FUSED=1 in a child process: every fused length in both dtypes reports stft_composed and stay within the
    per-frame bound."""
    cases = [(n, odd_hop(n), dt.name) for n in FUSED for dt in (F32, F64)]
    code = 'CASES = %r\nOUT = %r\n' % (cases, str(tmp_path)) + SWITCHED
    r = run_child(code, env={'DSC_NO_STFT_FUSED': '1'}, check=True)
    paths = [ln.split()[3] for ln in r.stdout.splitlines() if ln.startswith('PATH')]
    assert paths == ['stft_composed'] * len(cases), paths
    for n, hop, dt in cases:
        z = np.load(tmp_path / f'{n}_{dt}.npz')
        rr = stft_err(z['y'], ref_stft(z['x'], n, hop, z['w']), TAU[np.dtype(dt)])
        record_property(f'stft_composed:stft:{n}:{dt}', rr)
        print(f'stft_composed (switch) n_fft={n} {dt}: err / bound = {rr:.3g}')
        assert rr <= 1, (n, dt, rr)


# ---------------------------------------------------------------------------------------------------- (e) inverse, every length

def inverse_configs(n_fft):
    """(hop, window, centre, length kind, shape index, frames): hops n / 4, n / 2, odd and n; windows none / Hann / asymmetric; centre
    on and off; length natural, shorter, and longer than the last frame reaches; three batch shapes; 1, 2 and about 9 frames"""
    many = 9 if n_fft < 131072 else 5
    q, h, odd = max(1, n_fft // 4), n_fft // 2, min(odd_hop(n_fft), n_fft - 1)
    return [(q, 'hann', True, 'natural', 0, many), (h, 'rand', True, 'shorter', 1, many), (odd, 'rand', False, 'longer', 2, 2),
            (n_fft, None, False, 'natural', 1, 1), (odd, None, True, 'longer', 0, many), (q, 'rand', False, 'shorter', 1, many),
            (h, 'hann', True, 'natural', 2, 2), (n_fft, None, False, 'longer', 2, many)]


def _inverse_cases():
    return [(n, dt, i) for n in INVERSE for dt in (F32, F64) for i in range(len(inverse_configs(n)))]


@pytest.mark.parametrize('n_fft,dt,i', _inverse_cases(), ids=str)
def test_inverse_every_length(dsc, record_property, n_fft, dt, i):
    hop, win, center, lk, si, frames = inverse_configs(n_fft)[i]
    rng = np.random.default_rng([n_fft, dt.itemsize, i, 1])
    bins = n_fft // 2 + 1
    lead = [(), (3,), (2, 3)][si] if n_fft < 131072 else [(), (2,), (1, 2)][si]
    X = rand_spectrum(rng, lead + (frames, bins), CPX[dt])
    expected = n_fft + hop * (frames - 1)
    natural = expected - n_fft if center else expected
    length = {'natural': None, 'shorter': max(1, natural - min(5, hop)), 'longer': expected + hop + 3}[lk]
    if length is None and natural < 1:
        length = n_fft // 4                                      # one centred frame has no natural length
    run_istft(dsc, record_property, X, n_fft, hop, make_window(win, rng, n_fft, dt), center, length)


# ---------------------------------------------------------------------------------------------------- (f) inverse, chunking

# dsc_chunk_lines (op_common.h), as stft.cpp calls it for a scratch arena of `cap` bytes with nothing else pinned and lines of
# frame_b = n_fft * sizeof(real) bytes, the reserve 2 frame_b + 1024:
#     chunk = min(min(cap / 2, 128 MB) / frame_b, (cap - 2 frame_b - 1024) / frame_b, rows * n_frames)
# and stft.cpp exits when cap < 3 frame_b + 1024.  A scratch arena of 2 c frame_b bytes (c >= 2) therefore gives chunk = c frames, and
# dsc_init takes the scratch size as passed (rounded up to 256 B).  With n_frames > chunk the frame-window branch runs and needs
# chunk > ceil(n_fft / hop); with n_frames <= chunk < rows * n_frames whole rows go chunk / n_frames at a time.
CHUNKED = r'''
import numpy as np
import dsc_amd as dsc
from tests.test_fft_ref import TAU, real_of
from tests.test_stft_ref import istft_err, rand_spectrum, rand_window, ref_istft
n, chunk = 1024, N_CHUNK
rng = np.random.default_rng(43)
first = True
for cdt, hop, center, rows, frames, lk in CASES:
    cdt = np.dtype(cdt)
    rdt = real_of(cdt)
    if first:                                              # the cases of one child share a dtype
        dsc.init(256 << 20, 2 * chunk * n * rdt.itemsize)
        first = False
    X = rand_spectrum(rng, (rows, frames, n // 2 + 1), cdt)
    w = rand_window(rng, n, rdt)
    expected = n + hop * (frames - 1)
    length = None if lk == 'natural' else expected + hop + 3
    Xt, W = dsc.from_numpy(X), dsc.from_numpy(w)
    y = dsc.istft(Xt, n, hop, W, center, length)
    assert dsc.last_fft_path() == 'istft_ola'
    yh = y.numpy()
    assert Xt.numpy().tobytes() == X.tobytes()
    want, bound = ref_istft(X, n, hop, w, center, length)
    r = istft_err(yh, want, bound, TAU[rdt])
    print('RATIO', cdt, hop, center, rows, frames, lk, r, flush=True)
    assert r <= 1, r
dsc.synchronize()
print('CHUNKED OK', flush=True)
'''


def _chunked(cases, chunk, timeout=300):
    code = 'CASES = %r\n' % (cases,) + CHUNKED.replace('N_CHUNK', str(chunk))
    return run_child(code, timeout=timeout)


def _record_chunked(record_property, r):
    assert r.returncode == 0 and 'CHUNKED OK' in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    for ln in r.stdout.splitlines():
        if ln.startswith('RATIO'):
            record_property(f'istft_ola:istft:1024:{real_of(ln.split()[1])} (chunked)', float(ln.split()[-1]))
            print(ln)


@pytest.mark.parametrize('cdt', ['complex64', 'complex128'])
def test_inverse_frame_windows(record_property, cdt):
    """n_frames = 40 > chunk: a row is cut into windows of frames, each window's span starting where the previous one ended.  The
    scratch arena holds 2 * 12 frames: chunk = 12, above ceil(1024 / 125) = 9 and below 40.  Hop 256 and
    the odd hop 125, centre on and off, 2 rows, natural length and one longer than the last frame reaches (the last window's launch
    fills the tail with zeros)."""
    cases = [(cdt, hop, center, 2, 40, lk) for hop in (256, 125) for center in (True, False) for lk in ('natural', 'longer')]
    _record_chunked(record_property, _chunked(cases, 12))


@pytest.mark.parametrize('cdt', ['complex64', 'complex128'])
def test_inverse_whole_rows_in_several_launches(record_property, cdt):
    """n_frames = 5 <= chunk = 12 < rows * n_frames = 35: two of the 7 rows per launch, four launches, three of them with r0 > 0"""
    cases = [(cdt, hop, center, 7, 5, lk) for hop, center, lk in ((256, True, 'natural'), (125, False, 'longer'))]
    _record_chunked(record_property, _chunked(cases, 12))


def test_inverse_arena_too_small_is_a_checked_exit():
    """A scratch arena of 2 * 4 frames: chunk = 4 = ceil(1024 / 256), not more, with 40 frames per row.  The host check exits
    non-zero with its message before anything is launched; nothing runs on the GPU after it in that child."""
    r = _chunked([('complex128', 256, True, 1, 40, 'natural')], 4)
    assert r.returncode != 0 and 'CHUNKED OK' not in r.stdout and 'RATIO' not in r.stdout, (r.returncode, r.stdout[-500:])
    assert 'scratch arena too small' in r.stdout + r.stderr, (r.stdout[-1500:], r.stderr[-1500:])


# ---------------------------------------------------------------------------------------------------- (g) rows too long for two per launch

def test_rows_too_long_for_an_even_launch_take_the_composed_route(dsc, record_property):
    """f32 [3, 180_000_001]: 31-bit byte offsets leave room for one row per launch, and with odd T the second launch would start on an
    odd element, where the kernel's "even element => aligned pair load" test (relative to the launch base) no longer means aligned
    in memory.  stft.cpp keeps rows per launch even, as conv.cpp does, and sends this case to stft_composed (64-bit gather indices).
    n_fft 1024, odd hop 2^22 + 1: 43 frames per row, every one checked against the reference built from slices of x."""
    n_fft, hop, T, rows = 1024, (1 << 22) + 1, 180_000_001, 3
    rng = np.random.default_rng(47)
    x = rng.random((rows, T), dtype=np.float32)
    w = rand_window(rng, n_fft, np.float32)
    y = dsc.stft(dsc.from_numpy(x), n_fft, hop, dsc.from_numpy(w))
    assert dsc.last_fft_path() == 'stft_composed'
    yh = y.numpy()
    n_frames = 1 + T // hop
    assert yh.shape == (rows, n_frames, n_fft // 2 + 1) and n_frames == 43
    idx = np.arange(n_frames)[:, None] * hop - n_fft // 2 + np.arange(n_fft)[None, :]
    idx = np.abs(idx)
    idx = np.where(idx >= T, 2 * (T - 1) - idx, idx)                      # torch's reflect: -i, 2 (T - 1) - i
    want = np.fft.rfft(x[:, idx].astype(np.longdouble) * w.astype(np.longdouble), axis=-1)
    r = stft_err(yh, want, TAU[F32])
    record_property('stft_composed:stft:1024:float32 (2 GiB rows)', r)
    print(f'stft_composed [3, 180000001]: err / bound = {r:.3g}')
    assert r <= 1, r
