"""Float64 restatement of the reference's featurizers (rnnt/featurizer.py): the torch.stft call of its lines 86-105, the three
log stages, the HTK filterbank of its mel variant (the published formula; torchaudio is not used) and the streaming carry of
rnnt/tests/test_streaming.py:60-65 (keep the samples no frame has consumed yet).  Written apart from rnnt_amd/featurizer.py:
the tests hold both the module's torch path and the engine to this file."""
import math

import numpy as np
import torch

PLAIN, PIECEWISE, GAIN = "plain", "piecewise", "gain"
INT16_GAIN = pow(10, 0.05 * (2 * 20 * math.log10(32767)))


def frame_count(length, n_fft, hop, center=False):
    if center:
        return (length + 2 * (n_fft // 2) - n_fft) // hop + 1
    return 0 if length < n_fft else (length - n_fft) // hop + 1


def stream_step(state_len, chunk_len, n_fft, hop):
    """(frames completed, samples carried on) of one push."""
    total = state_len + chunk_len
    frames = frame_count(total, n_fft, hop)
    return frames, total - frames * hop


def power(x, n_fft, hop, win_length, center=False):
    """x (..., time) -> |stft|^2 (..., n_fft // 2 + 1, frames), float64."""
    x = x.to(torch.float64)
    spec = torch.stft(x, n_fft, hop, win_length, window=torch.hann_window(win_length, dtype=torch.float64, device=x.device),
                      center=center, pad_mode="reflect", onesided=True, normalized=False, return_complex=True)
    return spec.abs().pow(2.0)


def power_dft(x, n_fft, hop, win_length, center=False):
    """The same by an O(n^2) DFT in numpy: x (time,) -> (bins, frames) float64."""
    x = np.asarray(x, dtype=np.float64)
    if center:
        x = np.pad(x, n_fft // 2, mode="reflect")
    j = np.arange(win_length)
    w = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    w[left:left + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * j / win_length)  # periodic Hann
    frames = frame_count(len(x), n_fft, hop)
    k = np.arange(n_fft // 2 + 1)[:, None]
    n = np.arange(n_fft)[None, :]
    ang = 2.0 * np.pi * ((k * n) % n_fft) / n_fft
    out = np.zeros((n_fft // 2 + 1, frames))
    for f in range(frames):
        seg = w * x[f * hop:f * hop + n_fft]
        out[:, f] = (np.cos(ang) @ seg) ** 2 + (np.sin(ang) @ seg) ** 2
    return out


def log_stage(p, kind):
    if kind == PLAIN:
        return torch.log(p + 1e-6)
    if kind == PIECEWISE:  # featurizer.py:9-15
        cut, slope = 10e-3, 50
        return torch.where(p > cut, torch.log(p), slope * p + (math.log(cut) - slope * cut))
    if kind == GAIN:
        return torch.log((p + 1e-6) * INT16_GAIN)
    raise ValueError(kind)


def gain_three_branch(p):
    """What the reference's older log stage (featurizer.py:129-133, applied to p + 1e-6) computes, branch by branch: scale by the gain;
    values above e become their logarithm; then — on the tensor as the first assignment left it, which is what two in-place masked
    assignments in a row do — values at or below e are divided by e.  GAIN stands for this."""
    y = (p + 1e-6) * INT16_GAIN
    y = torch.where(y > math.e, torch.log(y), y)
    return torch.where(y <= math.e, y / math.e, y)


def htk_fbank(n_freqs, f_min, f_max, n_mels, sample_rate):
    """(n_freqs, n_mels) float64 triangles, HTK mel scale, no area normalisation."""
    hz = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
    pts = [hz(mel(f_min) + (mel(f_max) - mel(f_min)) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    fb = np.zeros((n_freqs, n_mels))
    for k in range(n_freqs):
        f = (sample_rate // 2) * k / (n_freqs - 1)
        for m in range(n_mels):
            lo, mid, hi = pts[m], pts[m + 1], pts[m + 2]
            fb[k, m] = max(0.0, min((f - lo) / (mid - lo), (hi - f) / (hi - mid)))
    return torch.from_numpy(fb)


def features(x, n_fft, hop, win_length, kind, mean, invstd, center=False, fbank=None):
    """x (..., time) -> (..., F, frames) float64; mean / invstd: float or a sequence of F values."""
    p = power(x, n_fft, hop, win_length, center)
    if fbank is not None:
        p = (p.transpose(-1, -2) @ fbank.to(torch.float64)).transpose(-1, -2)
    v = log_stage(p, kind)
    # per-bin values are what featurizer.py:77,82 holds: torch.tensor(list), i.e. rounded to fp32
    col = lambda t: t if isinstance(t, float) else torch.tensor(t).to(torch.float64).reshape(-1, 1)
    return (v - col(mean)) * col(invstd)


def ragged(waves, n_fft, hop, win_length, kind, mean, invstd, center=False, fbank=None):
    """List of 1-D waveforms -> ((N, F, max frames) float64 with zeros behind each utterance's frames, [frame counts])."""
    counts = [frame_count(len(w), n_fft, hop, center) for w in waves]
    F = n_fft // 2 + 1 if fbank is None else fbank.shape[1]
    out = torch.zeros(len(waves), F, max(counts), dtype=torch.float64)
    for i, (w, c) in enumerate(zip(waves, counts)):
        if c:
            out[i, :, :c] = features(w, n_fft, hop, win_length, kind, mean, invstd, center, fbank)
    return out, counts


def streamed(x, sizes, n_fft, hop, win_length, kind, mean, invstd):
    """x (time,) pushed in chunks of `sizes`: the per-push feature blocks [(F, frames)], and the samples left over."""
    carry = x[:0].to(torch.float64)
    outs, t = [], 0
    for k in sizes:
        carry = torch.cat((carry, x[t:t + k].to(torch.float64)))
        t += k
        frames, left = stream_step(0, len(carry), n_fft, hop)
        if frames:
            outs.append(features(carry[:(frames - 1) * hop + n_fft], n_fft, hop, win_length, kind, mean, invstd))
        else:
            outs.append(torch.zeros(n_fft // 2 + 1, 0, dtype=torch.float64))
        carry = carry[frames * hop:]
        assert len(carry) == left
    return outs, carry
