"""The vocoder tail of the reference's `utils.py` on the GPU: `spectrogram2wav` (utils.py:67-94), `griffin_lim`
(utils.py:96-106) and `invert_spectrogram` (utils.py:108-114), batched.

Same names and argument meaning as the reference, with two differences that the batching forces:
  * spectrograms are (T, 1 + n_fft//2) per utterance exactly as `synthesize.py:61-63` hands them over (`mag`), or a
    batch (B, T, 1 + n_fft//2); the reference's internal transpose to librosa's (1 + n_fft//2, T) never happens;
  * batched calls return a list of trimmed float32 waveforms (utterances trim to different lengths).
All arithmetic runs in libdctts_hip.so (csrc/vocoder_kernels.h); there is no CPU fallback.

The analysis direction, `get_spectrograms` (utils.py:18-65) and `load_spectrograms` (utils.py:147-165), is here too (csrc/analysis_kernels.h): one path as
in the reference, or a list of paths served by one batched call.  `dc_tts_amd.audio` keeps the host numpy form, which stays the default of prepo / get_batch.
"""
import ctypes
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .engine import DcttsError, _check, _ptr
from .hyperparams import Hyperparams, hp as _hp

TRIM_TOP_DB, TRIM_FRAME_LENGTH, TRIM_HOP_LENGTH = 60.0, 2048, 512     # librosa.effects.trim defaults (utils.py:92)


class Vocoder:
    """One vocoder handle per GPU (no weights; workspaces grow to the largest batch seen)."""

    def __init__(self, hp: Hyperparams = _hp, device: Optional[int] = None, momentum: float = 0.0):
        if not torch.cuda.is_available():
            raise DcttsError("dc_tts_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.lib = _lib.load()
        self.hp = hp
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        cfg = _lib.VocoderConfig(hp.n_fft, hp.hop_length, hp.win_length, hp.n_iter, hp.power, hp.preemphasis,
                                 float(hp.max_db), float(hp.ref_db), TRIM_TOP_DB, TRIM_FRAME_LENGTH, TRIM_HOP_LENGTH)
        h = ctypes.c_void_p()
        self._ok(self.lib.dctts_vocoder_create(ctypes.byref(h), self.device_index, ctypes.byref(cfg)))
        self._h = h
        if momentum != 0.0:
            self.set_momentum(momentum)

    def _ok(self, rc: int):
        if rc != 0:
            raise DcttsError(f"libdctts_hip error {rc}: {_lib.last_error()}")

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.dctts_vocoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_bytes(self) -> int:
        return int(self.lib.dctts_vocoder_device_bytes(self._h))

    def set_momentum(self, momentum: float):
        """Fast Griffin-Lim as librosa.griffinlim(momentum=...), 0 <= momentum < 1, from the next call on; 0 (the default) is the reference's loop."""
        self._ok(self.lib.dctts_vocoder_set_momentum(self._h, float(momentum)))

    def prof_enable(self, enable: bool):
        self._ok(self.lib.dctts_vocoder_prof_enable(self._h, int(bool(enable))))

    def prof_collect(self) -> Tuple[int, float]:
        """(launches, total ms) of the Griffin-Lim iteration kernel since prof_enable(True), by HIP events on the launch stream."""
        n = ctypes.c_int(0); ms = ctypes.c_double(0.0)
        self._ok(self.lib.dctts_vocoder_prof_collect(self._h, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    def n_samples(self, F: int) -> int:
        """Length of librosa.istft's output for F frames: hop_length * (F - 1)."""
        return self.hp.hop_length * (F - 1)

    def spectrogram2wav_device(self, mag: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """mag (B,F,1+n_fft//2) on the GPU -> (wav (B, hop*(F-1)) de-emphasised and untrimmed, bounds (B,2) int32)."""
        _check(mag, "mag", torch.float32, 3, self.device)
        B, F, nb = mag.shape
        if nb != self.hp.n_linear:
            raise ValueError(f"mag: last dim {nb} != 1 + n_fft//2 = {self.hp.n_linear}")
        wav = torch.empty(B, self.n_samples(F), dtype=torch.float32, device=self.device)
        bounds = torch.empty(B, 2, dtype=torch.int32, device=self.device)
        self._ok(self.lib.dctts_spectrogram2wav(self._h, _ptr(mag), B, F, _ptr(wav), _ptr(bounds), self._stream()))
        return wav, bounds

    def griffin_lim_device(self, spec: torch.Tensor, n_iter: Optional[int] = None, want_X: bool = False):
        """spec (B,F,1+n_fft//2) magnitudes on the GPU -> y (B, hop*(F-1)) [, X_best (B,F,1+n_fft//2) complex64]."""
        _check(spec, "spec", torch.float32, 3, self.device)
        B, F, nb = spec.shape
        if nb != self.hp.n_linear:
            raise ValueError(f"spec: last dim {nb} != 1 + n_fft//2 = {self.hp.n_linear}")
        n_iter = self.hp.n_iter if n_iter is None else int(n_iter)
        y = torch.empty(B, self.n_samples(F), dtype=torch.float32, device=self.device)
        X = torch.empty(B, F, nb, 2, dtype=torch.float32, device=self.device) if want_X else None
        self._ok(self.lib.dctts_griffin_lim(self._h, _ptr(spec), B, F, n_iter, _ptr(y), _ptr(X), self._stream()))
        return (y, torch.view_as_complex(X)) if want_X else y

    def set_mel_basis(self, basis: np.ndarray):
        """basis (n_mels, 1 + n_fft//2), what librosa.filters.mel returns: packed into the kernel's band table (banded rows only)."""
        basis = np.ascontiguousarray(basis, dtype=np.float32)
        if basis.ndim != 2 or basis.shape[1] != self.hp.n_linear:
            raise ValueError(f"basis: expected (n_mels, {self.hp.n_linear}), got {basis.shape}")
        self._ok(self.lib.dctts_vocoder_set_mel_basis(self._h, basis.ctypes.data_as(ctypes.c_void_p), basis.shape[0]))
        self._n_mels = basis.shape[0]

    def wav2spectrograms_device(self, wav: torch.Tensor, lengths: torch.Tensor, r: int = 1, trim: bool = True):
        """utils.py:18-65 for a ragged batch, nothing leaves the GPU: wav (B, Lmax) float32 zero-filled past each length, lengths (B) int32 ->
        mel (B, Fpad/r, n_mels) [frames 0, r, 2r, ...], mag (B, Fpad, 1+n_fft//2), n_frames (B) int32, bounds (B, 2) int32 [the trimmed range], with
        Fpad = 1 + Lmax//hop rounded up to a multiple of r.  Rows at or past n_frames[b] are zero (load_spectrograms' padding); n_frames 0 = nothing but
        zeros in the clip, -1 = too short to reflect-pad (at most n_fft//2 samples before or after the trim)."""
        _check(wav, "wav", torch.float32, 2, self.device)
        _check(lengths, "lengths", torch.int32, 1, self.device)
        B, Lmax = wav.shape
        if lengths.shape[0] != B:
            raise ValueError(f"lengths: {lengths.shape[0]} entries for {B} utterances")
        if r < 1:
            raise ValueError("r must be >= 1")
        if getattr(self, "_n_mels", None) is None:
            from .audio import mel_filterbank
            self.set_mel_basis(mel_filterbank(self.hp.sr, self.hp.n_fft, self.hp.n_mels))
        Fpad = -(-(1 + Lmax // self.hp.hop_length) // r) * r
        mel = torch.empty(B, Fpad // r, self._n_mels, dtype=torch.float32, device=self.device)
        mag = torch.empty(B, Fpad, self.hp.n_linear, dtype=torch.float32, device=self.device)
        n_frames = torch.empty(B, dtype=torch.int32, device=self.device)
        bounds = torch.empty(B, 2, dtype=torch.int32, device=self.device)
        self._ok(self.lib.dctts_wav2spectrograms(self._h, _ptr(wav), _ptr(lengths), B, Lmax, int(bool(trim)), int(r), _ptr(mel), _ptr(mag),
                                                 _ptr(n_frames), _ptr(bounds), self._stream()))
        return mel, mag, n_frames, bounds


_default: dict = {}


def _vocoder(hp: Hyperparams, device: Optional[int], momentum: Optional[float] = None) -> Vocoder:
    """The cached handle per (hp, device, momentum): a call that passes `momentum` never changes what a call without it computes."""
    key = (hp, torch.cuda.current_device() if device is None and torch.cuda.is_available() else device, float(momentum or 0.0))
    if key not in _default:
        _default[key] = Vocoder(hp, device, momentum=key[2])
    return _default[key]


def _pick(hp: Hyperparams, vocoder: Optional[Vocoder], momentum: Optional[float]) -> Vocoder:
    if vocoder is not None and momentum is not None:
        raise ValueError("pass either a Vocoder (its own momentum holds) or momentum=, not both")
    return vocoder or _vocoder(hp, None, momentum)


def _to_dev(a, device: torch.device) -> Tuple[torch.Tensor, bool]:
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) if isinstance(a, np.ndarray) else a
    single = t.dim() == 2
    if single:
        t = t[None]
    return t.to(device=device, dtype=torch.float32).contiguous(), single


def spectrogram2wav(mag, hp: Hyperparams = _hp, vocoder: Optional[Vocoder] = None, momentum: Optional[float] = None):
    """utils.py:67-94.  mag: (T, 1+n_fft//2) -> 1-D float32 numpy waveform (trimmed), as the reference returns it;
    or a batch (B, T, 1+n_fft//2) (numpy or torch) -> list of B such waveforms.  momentum: fast Griffin-Lim (Vocoder.set_momentum)."""
    v = _pick(hp, vocoder, momentum)
    m, single = _to_dev(mag, v.device)
    wav, bounds = v.spectrogram2wav_device(m)
    wav_h, b_h = wav.cpu().numpy(), bounds.cpu().numpy()
    out: List[np.ndarray] = [wav_h[i, b_h[i, 0]:b_h[i, 1]].copy() for i in range(wav_h.shape[0])]
    return out[0] if single else out


def _spectrograms(fpath_or_list, hp: Hyperparams, r: int, vocoder: Optional[Vocoder]):
    """The files' waveforms, padded to the longest, through ONE wav2spectrograms_device call -> per file (fname, mel rows, mag rows, n_frames)."""
    from .audio import load_wav
    single = isinstance(fpath_or_list, (str, os.PathLike))
    fpaths = [fpath_or_list] if single else list(fpath_or_list)
    v = vocoder or _vocoder(hp, None)
    ys = [load_wav(f, hp.sr) for f in fpaths]
    Lmax = max([len(y) for y in ys] + [hp.n_fft // 2 + 1])             # (a batch of too-short clips is reported per file below, not by the call)
    wav = torch.zeros(len(ys), Lmax, dtype=torch.float32).pin_memory()
    for i, y in enumerate(ys):
        wav[i, :len(y)] = torch.from_numpy(y)
    lengths = torch.tensor([len(y) for y in ys], dtype=torch.int32)
    mel, mag, n_frames, _ = v.wav2spectrograms_device(wav.to(v.device, non_blocking=True), lengths.to(v.device), r=r, trim=True)
    mel, mag, n_frames = mel.cpu().numpy(), mag.cpu().numpy(), n_frames.cpu().numpy()
    out = []
    for i, f in enumerate(fpaths):
        nf = int(n_frames[i])
        if nf <= 0:
            raise ValueError(f"get_spectrograms: {f}: " + ("nothing left after trimming (silent file)" if nf == 0 else
                                                            f"at most n_fft/2 = {hp.n_fft // 2} samples (before or after trimming)"))
        rows = -(-nf // r)
        out.append((os.path.basename(f), mel[i, :rows].copy(), mag[i, :rows * r].copy()))
    return out, single


def get_spectrograms(fpath_or_list, hp: Hyperparams = _hp, vocoder: Optional[Vocoder] = None):
    """utils.py:18-65 on the GPU: one path -> (mel (T, n_mels), mag (T, 1+n_fft//2)) float32 as `audio.get_spectrograms`; a list of paths ->
    a list of such pairs from one batched call.  WAV decoding stays on the host."""
    out, single = _spectrograms(fpath_or_list, hp, 1, vocoder)
    out = [(mel, mag) for _, mel, mag in out]
    return out[0] if single else out


def load_spectrograms(fpath_or_list, hp: Hyperparams = _hp, vocoder: Optional[Vocoder] = None):
    """utils.py:147-165 on the GPU: (fname, mel (T/r, n_mels), mag (T, 1+n_fft//2)) with T padded to a multiple of hp.r, as `audio.load_spectrograms`;
    a list of paths -> a list of such triples from one batched call."""
    out, single = _spectrograms(fpath_or_list, hp, hp.r, vocoder)
    return out[0] if single else out


def griffin_lim(spectrogram, hp: Hyperparams = _hp, vocoder: Optional[Vocoder] = None, momentum: Optional[float] = None):
    """utils.py:96-106, on (T, 1+n_fft//2) magnitudes (or a batch): returns the real waveform(s) as numpy.  momentum: as spectrogram2wav."""
    v = _pick(hp, vocoder, momentum)
    s, single = _to_dev(spectrogram, v.device)
    y = v.griffin_lim_device(s).cpu().numpy()
    return y[0] if single else y


def invert_spectrogram(spectrogram, hp: Hyperparams = _hp, vocoder: Optional[Vocoder] = None):
    """utils.py:108-114 (librosa.istft with the Hann window) for a REAL (T, 1+n_fft//2) spectrogram (zero phase) --
    the only real-input use the reference has is griffin_lim's first pass."""
    v = vocoder or _vocoder(hp, None)
    s, single = _to_dev(spectrogram, v.device)
    y = v.griffin_lim_device(s, n_iter=0).cpu().numpy()
    return y[0] if single else y
