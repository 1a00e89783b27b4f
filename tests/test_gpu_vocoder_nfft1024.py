"""n_fft = 1024 (513 bins) through the pair kernels (csrc/pair_kernels.h: two adjacent frames per 1024-point transform), both directions, against
oracle/vocoder_ref.py with the same hp.  Geometries: sr 16000 (hop 200, win 800, lpad 112: partial lane slots) and sr 20480 (hop 256, win 1024, lpad 0).
Odd frame counts with B = 2 are the cases that fail if a pair reaches into the next utterance.  Vocoder bounds are test_gpu_vocoder.py's.  Analysis:
test_gpu_analysis.py's metric (de-normalise in float64, error over the frame peak), e_gpu <= K * e32 and <= 1e-5, K = 1.5 x the worst e_gpu / e32
measured on the MI355X over these cases (table in DESIGN.md section 8)."""
import numpy as np
import pytest
import torch

from dc_tts_amd import audio
from dc_tts_amd.hyperparams import hp as hp0
from oracle import vocoder_ref as V
from test_gpu_vocoder import REL_TOL, dev, rel_err, speechlike_mag

pytestmark = pytest.mark.gpu
GEOMS = {"sr16000": (hp0.replace(sr=16000, n_fft=1024), 200, 800), "sr20480": (hp0.replace(sr=20480, n_fft=1024), 256, 1024)}
K = 1.5 * 1.44          # worst measured ratio (sr 20480, the 13-frame clip's mag rows)
_voc = {}


@pytest.fixture(params=sorted(GEOMS))
def geo(request):
    from dc_tts_amd.utils import Vocoder
    hp, hop, win = GEOMS[request.param]
    assert (hp.hop_length, hp.win_length, hp.n_linear) == (hop, win, 513)       # int(sr * 0.0125) must land exactly
    if request.param not in _voc:
        _voc[request.param] = Vocoder(hp)
    return hp, _voc[request.param]


def spec_batch(hp, F):
    return np.stack([V.denormalize(speechlike_mag(F, s)[:, ::2], hp, np.float32).T for s in (21, 22)])      # (2, F, 513), different content


@pytest.mark.parametrize("F", [4, 5, 31])
def test_istft_of_real_spectrogram(geo, F):
    """n_iter 0: istft_frames_pair_kernel + ola_kernel; F = 4 is the minimum (hop (F - 1) > 512), and F = 3 raises."""
    from dc_tts_amd.engine import DcttsError
    hp, v = geo
    spec = (np.random.default_rng(F).random((2, F, 513)) * 3).astype(np.float32)
    y = v.griffin_lim_device(dev(spec), n_iter=0).cpu().numpy()
    assert y.shape == (2, hp.hop_length * (F - 1))
    for b in range(2):
        assert rel_err(y[b], V.istft(spec[b].T, hp, np.float32)) < 1e-5
    with pytest.raises(DcttsError):
        v.griffin_lim_device(dev(spec[:, :3].copy()), n_iter=0)


def test_one_iteration_spectrum(geo):
    """X_best after one pass (stft_phase_pair_kernel), odd F; form and bounds of test_gpu_vocoder.test_one_iteration_spectrum."""
    hp, v = geo
    spec = (np.random.default_rng(11).random((1, 25, 513)) * 2 + 0.1).astype(np.float32)
    y, X = v.griffin_lim_device(dev(spec), n_iter=1, want_X=True)
    X = X.cpu().numpy()[0]
    est = V.stft(V.istft(spec[0].T, hp, np.float64), hp, np.float64).T
    ref = spec[0] * est / np.maximum(1e-8, np.abs(est))
    assert np.abs(np.abs(X) - spec[0]).max() < 1e-4
    w = np.minimum(1.0, np.abs(est) / np.median(np.abs(est)))
    assert (np.abs(X - ref) * w).max() < 2e-3 * spec.max()
    assert rel_err(y.cpu().numpy()[0], V.griffin_lim(spec[0].T, hp, np.float32, 1)) < REL_TOL


@pytest.mark.parametrize("n_iter,F,momentum", [(n, F, 0.0) for n in (1, 2, 7) for F in (30, 31)] + [(7, 31, 0.99)])
def test_griffin_lim_vs_oracle(geo, n_iter, F, momentum):
    """Plain: the oracle's loop.  Momentum: librosa.griffinlim(momentum=...)'s loop restated from V.stft / V.istft in float64, as test_gpu_vocoder_momentum.py."""
    from dc_tts_amd.utils import Vocoder
    hp, v = geo
    v = Vocoder(hp, momentum=momentum) if momentum else v
    spec, beta = spec_batch(hp, F), momentum / (1 + momentum)
    y = v.griffin_lim_device(dev(spec), n_iter=n_iter).cpu().numpy()
    for b in range(2):
        S = spec[b].T.astype(np.float64)
        X, c_prev = S.astype(np.complex128), 0
        for _ in range(n_iter if momentum else 0):
            c = V.stft(V.istft(X, hp, np.float64), hp, np.float64)
            t, c_prev = c - beta * c_prev, c
            X = S * t / np.maximum(1e-8, np.abs(t))
        ref = np.real(V.istft(X, hp, np.float64)) if momentum else V.griffin_lim(spec[b].T, hp, np.float32, n_iter)
        assert rel_err(y[b], ref) < REL_TOL, b
    assert torch.equal(v.griffin_lim_device(dev(spec[1:]), n_iter=n_iter)[0], dev(y[1]))      # utterance 1 alone: bitwise the same


def signal(hp, n, seed=0):
    t = np.arange(n) / hp.sr
    y = 0.3 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 3300.5 * t) + 0.05 * np.sin(2 * np.pi * 7000 * t)
    return (y + 0.01 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def reference(hp, y, dtype):
    """test_gpu_analysis.reference for any hp: normalised (mel (T, n_mels), mag (T, 513)) of an already trimmed clip."""
    y = np.append(y[0], y[1:] - np.float32(hp.preemphasis) * y[:-1])
    mag = np.abs(V.stft(y, hp, dtype)).astype(dtype)
    mel = np.dot(audio.mel_filterbank(hp.sr, hp.n_fft, hp.n_mels).astype(dtype), mag)
    norm = lambda x: np.clip((20 * np.log10(np.maximum(dtype(1e-5), x)) - dtype(hp.ref_db) + dtype(hp.max_db)) / dtype(hp.max_db), dtype(1e-8), dtype(1))
    return norm(mel).T, norm(mag).T


def err(hp, got, ref, per_frame):
    lin = lambda v: 10.0 ** ((v.astype(np.float64) * hp.max_db - hp.max_db + hp.ref_db) / 20)
    d, peak = np.abs(lin(got) - lin(ref)).max(axis=1), lin(ref).max(axis=1)
    return float((d / peak).max()) if per_frame else float(d.max() / peak.max())


def check_values(hp, mel, mag, y, r, what, per_frame=True):
    (mel64, mag64), (mel32, mag32) = reference(hp, y, np.float64), reference(hp, y, np.float32)
    F = mag64.shape[0]
    for name, got, r64, r32 in (("mag", mag[:F], mag64, mag32), ("mel", mel[:-(-F // r)], mel64[::r], mel32[::r])):
        e_gpu, e32 = err(hp, got, r64, per_frame), err(hp, r32, r64, per_frame)
        print(f"{what} {name}: F={F} e_gpu={e_gpu:.3e} e32={e32:.3e} ratio={e_gpu / e32:.2f}")
        assert e_gpu <= K * e32 and e_gpu <= 1e-5, (what, name, e_gpu, e32)
    assert not mag[F:].any() and not mel[-(-F // r):].any()                     # rows past n_frames are exactly zero


def analyse(v, clips, r, trim):
    wav = np.zeros((len(clips), max(len(c) for c in clips)), np.float32)
    for i, c in enumerate(clips):
        wav[i, :len(c)] = c
    lengths = torch.tensor([len(c) for c in clips], dtype=torch.int32).cuda()
    return [t.cpu().numpy() for t in v.wav2spectrograms_device(dev(wav), lengths, r=r, trim=trim)]


@pytest.mark.parametrize("r,trim", [(1, False), (1, True), (4, False), (4, True)])
def test_analysis_ragged(geo, r, trim):
    """Frame counts 25 (= Fpad for r = 1: odd), 8 and 13: live pairs, a live frame beside a dead one, dead pairs.  With trim the first clip loses
    leading silence, so its frames start at an offset; what is kept then begins with an onset (frames that barely touch the signal beside loud ones),
    which is no stationary clip but the cross-talk case below: that clip is measured over the utterance's peak."""
    hp, v = geo
    hop = hp.hop_length
    clips = [signal(hp, 24 * hop + 50, 0), signal(hp, 7 * hop + 10, 1), signal(hp, 12 * hop, 2)]
    if trim:
        clips[0][:1300] = 0.0
    mel, mag, n_frames, bounds = analyse(v, clips, r, trim)
    Fpad = -(-25 // r) * r
    assert mag.shape == (3, Fpad, 513) and mel.shape == (3, Fpad // r, hp.n_mels)
    want = [V.trim_bounds(c) if trim else (0, len(c)) for c in clips]
    assert bounds.tolist() == [list(w) for w in want] and n_frames.tolist() == [1 + (e - s) // hop for s, e in want]
    assert (not trim and n_frames.tolist() == [25, 8, 13]) or (trim and want[0][0] > 0)
    for i, (c, (s, e)) in enumerate(zip(clips, want)):
        check_values(hp, mel[i], mag[i], c[s:e], r, f"{hp.sr} r={r} trim={trim} [{i}]", per_frame=not (trim and i == 0))
    alone = analyse(v, clips[1:2], r, trim)
    assert np.array_equal(alone[1][0, :8], mag[1, :8]) and np.array_equal(alone[0][0, :-(-8 // r)], mel[1, :-(-8 // r)])      # independent of the batch


def test_analysis_cross_talk(geo):
    """A 40 dB amplitude step at a frame boundary: the quiet frames beside it share a transform with loud ones, so their rounding error is relative to
    the louder frame -- measured over the UTTERANCE's peak, under the same rule (the figures are in DESIGN.md section 8)."""
    hp, v = geo
    y = signal(hp, 20 * hp.hop_length, 3)
    y[:9 * hp.hop_length] *= 0.01
    mel, mag, n_frames, _ = analyse(v, [y], 1, False)
    assert n_frames.tolist() == [21]
    check_values(hp, mel[0], mag[0], y, 1, f"{hp.sr} cross-talk", per_frame=False)
