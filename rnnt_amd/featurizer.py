"""The featurizers of the reference (rnnt/featurizer.py) — waveform to the features the encoder reads — with its constructor
arguments, whose forward runs on the HIP engine (C ABI rnnt_engine_featurizer_*; rnnt_amd/csrc/featurizer.hip):
whole utterances, ragged batches and streaming pushes that carry the window overlap on the device.

    featurizer:
      _target_: rnnt_amd.TFJSSpectrogram              # was rnnt.featurizer.TFJSSpectrogram

One definition, two paths, as AudioEncoder.  The torch path is the module stated with torch.stft: any device, any float dtype
(int16 samples are scaled by 1 / 32768 to fp32 first); it serves the CPU, float64, and is the oracle of the engine path.  The
engine path takes fp32 or int16 samples on a HIP device; `backend` ("auto" | "torch" | "engine") forces either, "engine" raises
where it does not apply.  The modules hold no parameters and run under no_grad.

Definition.  Frame f covers samples f * hop .. f * hop + n_fft - 1 (of the signal reflected by n_fft / 2 at both ends when
`center`); an utterance of `len` samples has (len - n_fft) // hop + 1 frames (0 below n_fft), or (len + 2 * (n_fft // 2) - n_fft) // hop + 1
centred (torch.stft's count: len // hop + 1 for an even n_fft, (len - 1) // hop + 1 for an odd one).  The
power |stft|^2 (periodic Hann window of win_length, centred in n_fft) goes through an optional filterbank, one of three log
stages and (v - mean) * invstddev per bin.  Streaming: the state is the samples not yet consumed, (N, len) fp32; a push reads
state followed by chunk, emits the frames they complete and keeps the samples from frames * hop on.  Every length is host
arithmetic.  On the engine a streamed utterance equals the whole one bit for bit.
"""
import ctypes
import math

import torch

from . import engine

LOG_PLAIN, LOG_PIECEWISE, LOG_GAIN = 0, 1, 2  # include/rnnt_engine.h RNNT_FEAT_LOG_*
PCM_F32, PCM_S16 = 0, 1                       # RNNT_FEAT_PCM_*
# the reference's `_gain`: pow(10, 0.05 * 2 * 20 * log10(32767)) = 32767^2
INT16_GAIN = pow(10, 0.05 * (2 * 20 * math.log10(torch.iinfo(torch.int16).max)))
# backend "auto" takes the engine path wherever it applies, without a size threshold: at the reference's sizes it was faster than the
# torch path on the same device, and than the torch path on the host plus the feature upload, at every shape timed, from a 1-frame push
# to a ragged batch of 32 (tools/bench_featurizer.py, profiles/featurizer_bench.txt).


class _Desc(ctypes.Structure):  # include/rnnt_engine.h: rnnt_featurizer_desc
    _fields_ = [("n_fft", ctypes.c_int), ("win_length", ctypes.c_int), ("hop_length", ctypes.c_int), ("center", ctypes.c_int),
                ("log_kind", ctypes.c_int), ("gain", ctypes.c_float), ("n_filters", ctypes.c_int)]


def frame_count(length, n_fft, hop_length, center=False):
    """Frames of an utterance of `length` samples."""
    if center:
        return (length + 2 * (n_fft // 2) - n_fft) // hop_length + 1
    return (length - n_fft) // hop_length + 1 if length >= n_fft else 0


def stream_lengths(state_len, chunk_len, n_fft, hop_length):
    """(frames a push completes, samples of state it leaves) for `state_len` carried samples and a chunk of `chunk_len`."""
    total = state_len + chunk_len
    frames = frame_count(total, n_fft, hop_length)
    return frames, total - frames * hop_length


def mel_filterbank(n_freqs, f_min, f_max, n_mels, sample_rate):
    """HTK triangular filters without area normalisation, (n_freqs, n_mels) float64: filter m rises from f[m] to 1 at f[m+1] and falls
    to 0 at f[m+2], the f[] equally spaced on the mel scale 2595 log10(1 + f / 700) between f_min and f_max; bin k sits at
    k * (sample_rate // 2) / (n_freqs - 1) Hz."""
    freqs = torch.linspace(0, sample_rate // 2, n_freqs, dtype=torch.float64)
    m_lo, m_hi = (2595.0 * math.log10(1.0 + f / 700.0) for f in (f_min, f_max))
    f_pts = 700.0 * (10.0 ** (torch.linspace(m_lo, m_hi, n_mels + 2, dtype=torch.float64) / 2595.0) - 1.0)
    diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - freqs[:, None]
    down, up = -slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:]
    return torch.clamp(torch.minimum(down, up), min=0.0)


class _Featurizer(torch.nn.Module):
    backend = "auto"     # "auto" | "torch" | "engine"
    time_major = False   # True: the (N, F, L) result is a view of (N, L, F) memory, frames' bins contiguous (both paths)

    def _setup(self, n_fft, hop_length, win_length, center, log_kind, mean, invstddev, fbank=None):
        self.n_fft, self.hop_length, self.win_length = int(n_fft), int(hop_length), int(win_length)
        self.center, self.log_kind = bool(center), log_kind
        self.mean = mean if isinstance(mean, float) else torch.tensor(mean)
        self.invstddev = invstddev if isinstance(invstddev, float) else torch.tensor(invstddev)
        self.fbank = fbank  # (n_freqs, n_filters) float64 or None
        self.n_features = self.n_fft // 2 + 1 if fbank is None else int(fbank.shape[1])
        for name, v in (("mean", self.mean), ("invstddev", self.invstddev)):
            if torch.is_tensor(v) and v.numel() != 1 and tuple(v.shape) != (self.n_features,):
                raise ValueError(f"{type(self).__name__}: {name} holds {tuple(v.shape)} values, the features have {self.n_features} bins")
        self._gain = INT16_GAIN
        self._cache = {}  # device -> (desc, basis, fbank, mean, invstd)
        self.last_backend = None

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_cache"] = {}
        return state

    # ------------------------------------------------------------------------------------------------- torch path
    def _log_stage(self, p):
        if self.log_kind == LOG_PIECEWISE:  # rnnt/featurizer.py:9-15
            cut, slope = 10e-3, 50
            return torch.where(p > cut, torch.log(p), slope * p + (math.log(cut) - slope * cut))
        if self.log_kind == LOG_GAIN:
            # what the in-place three-branch statement of rnnt/featurizer.py:129-133 evaluates to: (p + 1e-6) * gain >= 1073 > e^e,
            # so only its log branch is ever taken, and the second statement finds log(.) > e again
            return torch.log((p + 1e-6) * self._gain)
        return torch.log(p + 1e-6)

    def _vec(self, v, like):
        if not torch.is_tensor(v):
            return v
        return v.to(device=like.device, dtype=like.dtype).reshape(-1, 1)

    def _torch(self, x):
        """(N, time) float -> (N, F, L)."""
        spec = torch.stft(x, self.n_fft, self.hop_length, self.win_length,
                          window=torch.hann_window(self.win_length, dtype=x.dtype, device=x.device),
                          center=self.center, pad_mode="reflect", onesided=True, normalized=False, return_complex=True)
        p = spec.abs().pow(2.0)
        if self.fbank is not None:
            p = torch.matmul(p.transpose(-1, -2), self.fbank.to(device=x.device, dtype=x.dtype)).transpose(-1, -2)
        return (self._log_stage(p) - self._vec(self.mean, p)) * self._vec(self.invstddev, p)

    def _torch_ragged(self, x, lens):
        """(N, T) float, sample counts -> (N, F, max frames), zeros behind each utterance's own frames."""
        counts = [frame_count(n, self.n_fft, self.hop_length, self.center) for n in lens]
        out = torch.zeros((x.shape[0], self.n_features, max(counts, default=0)), dtype=x.dtype, device=x.device)
        for i, (n, c) in enumerate(zip(lens, counts)):
            if c:
                out[i, :, :c] = self._torch(x[i:i + 1, :n])[0]
        return out

    @staticmethod
    def _as_float(x):
        if x.dtype == torch.int16:
            return x.to(torch.float32) * (1.0 / 32768.0)
        if not x.is_floating_point():
            raise TypeError(f"samples must be a float dtype or int16, got {x.dtype}")
        return x

    def _layout(self, y):
        return y.permute(0, 2, 1).contiguous().permute(0, 2, 1) if self.time_major else y

    # ------------------------------------------------------------------------------------------------- dispatch
    def _stage_words(self):
        """Floats of LDS k_feat_power stages for a 32-frame tile: the span, one pad word per hop samples when the hop is even."""
        span = 31 * self.hop_length + self.n_fft
        return span + (span // self.hop_length if self.hop_length % 2 == 0 else 0) + 1

    def _use_engine(self, x, frames):
        if self.backend not in ("auto", "torch", "engine"):
            raise ValueError(f"{type(self).__name__}.backend {self.backend!r}: 'auto', 'torch' or 'engine'")
        if self.backend == "torch":
            return False
        why = None
        if x.device.type != "cuda" or x.dtype not in (torch.float32, torch.int16):
            why = f"samples are {x.dtype} on {x.device} (needs fp32 or int16 on a HIP device)"
        elif self._stage_words() > 16384 or max(self.n_fft, self.hop_length, self.n_features) > 65536:
            why = "31 * hop_length + n_fft samples beyond the kernel's 64 KB stage"  # (RNNT_ERR_UNSUPPORTED on the C side)
        elif x.shape[0] * max(frames, 1) > 2 ** 28 or frames * self.hop_length + self.n_fft >= 2 ** 31:
            why = "more than 2^28 frames in the batch or 2^31 samples in an utterance"
        if why is not None:
            if self.backend == "engine":
                raise RuntimeError(f"{type(self).__name__}(backend='engine'): the engine path does not apply: {why}")
            return False
        return True

    def _check_lengths(self, lens):
        pad = self.n_fft // 2
        for n in lens:
            if self.center and n <= pad:
                raise ValueError(f"{type(self).__name__}: an utterance of {n} samples is not longer than the reflect pad of {pad}")

    @torch.no_grad()
    def forward(self, waveform):
        """(time,) -> (F, L); (N, time) -> (N, F, L); a list of 1-D tensors of any lengths -> ((N, F, max L), frame counts int64 on
        the CPU), every utterance's frames followed by zeros."""
        if isinstance(waveform, (list, tuple)):
            if not waveform or any(w.dim() != 1 for w in waveform):
                raise ValueError(f"{type(self).__name__}: a ragged batch is a non-empty list of 1-D tensors")
            lens = [int(w.shape[0]) for w in waveform]
            self._check_lengths(lens)
            counts = [frame_count(n, self.n_fft, self.hop_length, self.center) for n in lens]
            x = torch.nn.utils.rnn.pad_sequence(list(waveform), batch_first=True)
            if self._use_engine(x, max(counts)):
                self.last_backend = "engine"
                y = self._engine(x, lens, max(counts))[0]
            else:
                self.last_backend = "torch"
                y = self._layout(self._torch_ragged(self._as_float(x), lens))
            return y, torch.tensor(counts, dtype=torch.int64)
        if waveform.dim() not in (1, 2):
            raise ValueError(f"{type(self).__name__} takes (time,), (N, time) or a list of 1-D tensors, got {tuple(waveform.shape)}")
        x = waveform if waveform.dim() == 2 else waveform[None]
        if x.shape[0] < 1:
            raise ValueError(f"{type(self).__name__}: empty batch")
        T = int(x.shape[1])
        self._check_lengths([T])
        frames = frame_count(T, self.n_fft, self.hop_length, self.center)
        if frames < 1:
            raise ValueError(f"{type(self).__name__}: {T} samples are shorter than one frame of {self.n_fft}")
        if self._use_engine(x, frames):
            self.last_backend = "engine"
            y = self._engine(x, None, frames)[0]
        else:
            self.last_backend = "torch"
            y = self._layout(self._torch(self._as_float(x)))
        return y if waveform.dim() == 2 else y[0]

    def streaming_init_state(self, batch_size):
        """No samples carried yet: (batch_size, 0) fp32 on the CPU (move it to the samples' device, as the encoder's state)."""
        if self.center or self.hop_length > self.n_fft:
            raise ValueError(f"{type(self).__name__}: a centred featurizer cannot stream (the reflected end is not known yet), nor one "
                             "whose hop_length exceeds n_fft")
        return torch.zeros(batch_size, 0)

    @torch.no_grad()
    def streaming_forward(self, chunk, state):
        """chunk (N, time) of any length, 0 included; state (N, carried samples).  Returns ((N, F, frames completed), next state);
        a push that completes no frame returns (N, F, 0) and the longer state."""
        if self.center or self.hop_length > self.n_fft:
            raise ValueError(f"{type(self).__name__}: a centred featurizer cannot stream (the reflected end is not known yet), nor one "
                             "whose hop_length exceeds n_fft")
        if chunk.dim() != 2 or state.dim() != 2 or state.shape[0] != chunk.shape[0] or chunk.shape[0] < 1:
            raise ValueError(f"{type(self).__name__}.streaming_forward takes chunk (N, time) and state (N, carried), got "
                             f"{tuple(chunk.shape)} and {tuple(state.shape)}")
        frames, left = stream_lengths(int(state.shape[1]), int(chunk.shape[1]), self.n_fft, self.hop_length)
        if self._use_engine(chunk, frames):
            if state.device != chunk.device or state.dtype != torch.float32:
                raise RuntimeError(f"{type(self).__name__}.streaming_forward: the state must be fp32 on the samples' device")
            self.last_backend = "engine"
            return self._engine(chunk, None, frames, state, left)
        self.last_backend = "torch"
        c = self._as_float(chunk)
        x = torch.cat((state.to(device=c.device, dtype=c.dtype), c), dim=1)
        if frames:
            y = self._layout(self._torch(x[:, :(frames - 1) * self.hop_length + self.n_fft]))
        else:
            y = torch.zeros((x.shape[0], self.n_features, 0), dtype=x.dtype, device=x.device)
        return y, x[:, frames * self.hop_length:]

    # ------------------------------------------------------------------------------------------------- engine path
    def _prepared(self, dev):
        """(description, basis, filterbank, mean, invstd) on `dev`, packed on first use."""
        hit = self._cache.get(dev)
        if hit is not None:
            return hit
        lib = engine.lib()
        d = _Desc(self.n_fft, self.win_length, self.hop_length, int(self.center), self.log_kind, float(self._gain),
                  0 if self.fbank is None else int(self.fbank.shape[1]))
        F = self.n_features
        vec = lambda v: (v.to(torch.float32).reshape(-1).expand(F) if torch.is_tensor(v) else torch.full((F,), float(v))).contiguous().to(dev)
        n = ctypes.c_size_t(0)
        with torch.cuda.device(dev):
            engine._check(lib.rnnt_engine_featurizer_basis_bytes(ctypes.byref(d), ctypes.byref(n)))
            basis = torch.empty(int(n.value), dtype=torch.uint8, device=dev)
            window = torch.hann_window(self.win_length, dtype=torch.float32, device=dev)
            engine._check(lib.rnnt_engine_featurizer_pack(ctypes.byref(d), engine._p(window), engine._p(basis),
                                                          ctypes.c_size_t(basis.numel()), engine._stream(dev)))
            fb = None if self.fbank is None else self.fbank.to(torch.float32).contiguous().to(dev)
        self._cache[dev] = (d, basis, fb, vec(self.mean), vec(self.invstddev))
        return self._cache[dev]

    def _engine(self, x, lens, frames, state=None, left=0):
        """x (N, T) fp32 / int16 on a HIP device; lens: host sample counts or None; `frames` stored per utterance.  Returns
        ((N, F, frames), next state or None)."""
        dev = x.device
        d, basis, fb, mean, invstd = self._prepared(dev)
        if x.stride(1) != 1 and x.shape[1] > 1:
            x = x.contiguous()
        N, T = int(x.shape[0]), int(x.shape[1])
        F = self.n_features
        lib = engine.lib()
        with torch.cuda.device(dev):
            if self.time_major:
                out = torch.empty((N, frames, F), dtype=torch.float32, device=dev).permute(0, 2, 1)
            else:
                out = torch.empty((N, F, frames), dtype=torch.float32, device=dev)
            strides = (ctypes.c_int64 * 3)(*out.stride())
            n = ctypes.c_size_t(0)
            engine._check(lib.rnnt_engine_featurizer_workspace_bytes(ctypes.byref(d), N, frames, ctypes.byref(n)))
            ws = engine.workspace(dev, n.value) if n.value else None
            pcm = PCM_S16 if x.dtype == torch.int16 else PCM_F32
            args = (N, T)
            tail = (pcm, engine._p(mean), engine._p(invstd), engine._p(out) if frames else None, strides, frames)
            wsa = (engine._p(ws), ctypes.c_size_t(ws.numel() if ws is not None else 0), engine._stream(dev))
            xp = engine._p(x) if T else None
            if state is None:
                lens_c = None if lens is None else (ctypes.c_int32 * N)(*lens)
                engine._check(lib.rnnt_engine_featurizer_fwd(ctypes.byref(d), engine._p(basis), engine._p(fb), xp, ctypes.c_int64(x.stride(0)),
                                                             *args, lens_c, *tail, *wsa))
                return out, None
            if not state.is_contiguous():
                state = state.contiguous()
            slen = int(state.shape[1])
            new = torch.empty((N, left), dtype=torch.float32, device=dev)
            engine._check(lib.rnnt_engine_featurizer_stream_push(
                ctypes.byref(d), engine._p(basis), engine._p(fb), engine._p(state) if slen else None, slen, xp, ctypes.c_int64(x.stride(0)),
                *args, *tail, engine._p(new) if left else None, left, *wsa))
            return out, new


class TFJSSpectrogram(_Featurizer):
    """rnnt.featurizer.TFJSSpectrogram: |stft|^2 (center=False) -> piecewise linear / log (or log(p + 1e-6)) -> (v - mean) * invstddev;
    `mean` / `invstddev` a float or one value per bin."""

    def __init__(self, n_fft: int, hop_length: int, win_length: int, apply_linear_log: bool = True, mean=15.0, invstddev=0.25) -> None:
        super().__init__()
        self.apply_linear_log = apply_linear_log
        self._setup(n_fft, hop_length, win_length, False, LOG_PIECEWISE if apply_linear_log else LOG_PLAIN, mean, invstddev)


class TFJSOldPiecewiseSpectrogram(_Featurizer):
    """rnnt.featurizer.TFJSOldPiecewiseSpectrogram: as TFJSSpectrogram with the older log stage, log((p + 1e-6) * 32767^2)."""

    def __init__(self, n_fft: int, hop_length: int, win_length: int, apply_linear_log: bool = True, mean=15.0, invstddev=0.25) -> None:
        super().__init__()
        self.apply_linear_log = apply_linear_log
        self._setup(n_fft, hop_length, win_length, False, LOG_GAIN if apply_linear_log else LOG_PLAIN, mean, invstddev)


class NormalizedMelSpectrogram(_Featurizer):
    """rnnt.featurizer.NormalizedMelSpectrogram restated without torchaudio: center=True with reflect padding, power 2, an HTK
    triangular filterbank without area normalisation (mel_filterbank, float64, from the published formula), log((p + 1e-6) * 32767^2),
    (v - mean) * invstddev.  Offline only: a centred featurizer cannot stream.  torchaudio is not imported anywhere in this package;
    the module's parity is pinned to the float64 restatement of tests/featurizer_oracle.py alone, never to torchaudio itself."""

    def __init__(self, apply_linear_log: bool = True, mean=15.0, invstddev=0.25, sample_rate: int = 16000, n_fft: int = 400,
                 win_length=None, hop_length=None, f_min: float = 0.0, f_max=None, n_mels: int = 128) -> None:
        super().__init__()
        if not apply_linear_log:
            raise ValueError("NormalizedMelSpectrogram: apply_linear_log=False (the reference then normalises the raw power) is not stated here")
        win_length = n_fft if win_length is None else win_length
        hop_length = win_length // 2 if hop_length is None else hop_length
        self.apply_linear_log, self.sample_rate, self.n_mels = apply_linear_log, sample_rate, n_mels
        self.f_min, self.f_max = float(f_min), float(sample_rate // 2 if f_max is None else f_max)
        fb = mel_filterbank(n_fft // 2 + 1, self.f_min, self.f_max, n_mels, sample_rate)
        self._setup(n_fft, hop_length, win_length, True, LOG_GAIN, mean, invstddev, fb)
