"""Stand-in modules for the streaming-decode tests (tests/test_stream_*.py): the reference's ConvPredictor in plain torch, a small
stateful predictor with the reference LSTMPredictor's call signature, and a causal encoder with the reference's streaming interface
(rnnt/jasper.py streaming_forward / streaming_init_state, rnnt/causalconv.py:32-40) whose output does not depend on how its input
is chunked, bit for bit."""
import numpy as np
import torch


class TorchConvPredictor(torch.nn.Module):
    """The reference's ConvPredictor (rnnt/predictor.py:189-229, rnnt/causalconv.py) in plain torch, with its state-dict keys."""

    class _Causal(torch.nn.Module):
        def __init__(self, c, k):
            super().__init__()
            self.k = k
            self.conv = torch.nn.Conv1d(c, c, k)

        def forward(self, x):
            return self.conv(torch.nn.functional.pad(x, (self.k - 1, 0)))

    def __init__(self, V, O, E):
        super().__init__()
        self.embedding = torch.nn.Embedding(V, E)
        self.input_layer_norm = torch.nn.LayerNorm(E)
        self.conv1 = self._Causal(E, 3)
        self.conv2 = self._Causal(E, 5)
        self.linear = torch.nn.Linear(E, O)
        self.output_layer_norm = torch.nn.LayerNorm(O)

    def forward(self, ids):
        x = self.input_layer_norm(self.embedding(ids)).permute(0, 2, 1)
        x = torch.nn.functional.gelu(self.conv1(x))
        x = torch.nn.functional.gelu(self.conv2(x)).permute(0, 2, 1)
        return self.output_layer_norm(self.linear(x))


class LSTMLikePredictor(torch.nn.Module):
    """A stateful predictor with the reference LSTMPredictor's signature: forward(ids, lengths, state=None) -> (features, lengths, state)."""

    def __init__(self, V, O, E, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.embedding = torch.nn.Embedding(V, E)
        self.lstm = torch.nn.LSTM(E, E, batch_first=True)
        self.linear = torch.nn.Linear(E, O)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 if p.dim() == 2 and p.shape == self.embedding.weight.shape else 0.3))

    def forward(self, ids, lengths, state=None):
        y, state = self.lstm(self.embedding(ids), state)
        return torch.tanh(self.linear(y)) * 3.0, lengths, state


class PassThroughEncoder(torch.nn.Module):
    """Encoder output handed over as is: the test's frames as the (N, C, L) tensor an encoder would return."""

    def forward(self, x):
        return x

    def calc_output_lens(self, lens):
        return lens


class StreamingCausalEncoder(torch.nn.Module):
    """Two causal stages with the reference's streaming interface: y[t] = x[t] + x[t-1] / 2 + x[t-2] / 4 (zeros before the start), then
    a stride-2 stage keeping y[2t + 1].  Elementwise arithmetic only, so the streamed output equals the whole-input output exactly.
    streaming_init_state returns CPU tensors, as rnnt/jasper.py:159-170 does; the stride remainder rides in the second state tensor
    (rnnt/causalconv.py:38)."""

    def forward(self, x):
        y, _ = self.streaming_forward(x, [t.to(x.device) for t in self.streaming_init_state(x.shape[0])])
        return y

    def streaming_init_state(self, batch_size):
        return [torch.zeros(batch_size, 0, 2), torch.zeros(batch_size, 0, 0)]  # (channels fill in on first use)

    def streaming_forward(self, x, state):
        s0, s1 = state
        if s0.shape[1] != x.shape[1]:
            s0 = torch.zeros(x.shape[0], x.shape[1], 2, dtype=x.dtype, device=x.device)
            s1 = torch.zeros(x.shape[0], x.shape[1], 0, dtype=x.dtype, device=x.device)
        xp = torch.cat([s0, x], dim=2)
        y = xp[..., 2:] + 0.5 * xp[..., 1:-1] + 0.25 * xp[..., :-2]
        yp = torch.cat([s1, y], dim=2)
        n = yp.shape[2] // 2
        return yp[..., 1:2 * n:2], [xp[..., xp.shape[2] - 2:], yp[..., 2 * n:]]

    def calc_output_lens(self, lens):
        return lens // 2


def load_into(mod, sd):
    res = mod.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def cpu_model(spec, pred_sd, joint_sd, encoder=None):
    import rnnt_amd
    pred = TorchConvPredictor(spec["V"], spec["O"], spec["E"])
    joint = rnnt_amd.JointNetwork(spec["fa"], spec["ft"], spec["H"], spec["V"])
    load_into(pred, pred_sd)
    load_into(joint, joint_sd)
    return rnnt_amd.RNNTModel(pred, encoder or PassThroughEncoder(), joint).eval()


def engine_model(spec, pred_sd, joint_sd, encoder=None):
    import rnnt_amd
    rnnt_amd.engine.lib()  # fail loudly if the HIP extension is missing
    pred = rnnt_amd.ConvPredictor(spec["V"], spec["O"], spec["E"], 0.3)
    joint = rnnt_amd.JointNetwork(spec["fa"], spec["ft"], spec["H"], spec["V"])
    load_into(pred, pred_sd)
    load_into(joint, joint_sd)
    return rnnt_amd.RNNTModel(pred, encoder or PassThroughEncoder(), joint).cuda().eval()


def partitions(T, seed=0):
    """Chunkings of T frames: {name: [chunk lengths]}; "random" holds empty pushes."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in (1, 2, 3, 7, 16, 17):
        out[str(k)] = [k] * (T // k) + ([T % k] if T % k else [])
    out["all"] = [T]
    rnd, left = [], T
    while left > 0:
        k = int(rng.choice([0, 0, 1, 2, 5, 9, 13, 31]))
        k = min(k, left)
        rnd.append(k)
        left -= k
    out["random"] = [0] + rnd + [0]
    return out


def stream_frames(stream, frames_ct, sizes):
    """Push `frames_ct` (C, T) tensor chunk by chunk through stream.push_encoded; returns (labels, [(labels of the push, path)])."""
    got, pushes, t = [], [], 0
    for k in sizes:
        new = stream.push_encoded(frames_ct[None, :, t:t + k])
        t += k
        got += new
        pushes.append((new, stream.last_path, k))
    assert got == stream.tokens
    return got, pushes
