"""Streaming greedy decode: RNNTModel.greedy_stream() returns a GreedyStream that decodes chunk by chunk, carrying
the loop of the reference's greedy decode (rnnt/model.py:108-125) from one push of encoder frames to the next.  For every way of
cutting an utterance into pushes, empty ones included, the labels of the pushes concatenated equal RNNTModel.greedy_decode of all
frames at once with the same max_length, wherever the argmax is not a rounding-level tie.

HostGreedyLoop is greedy_decode's host loop made resumable; greedy_decode and the host path of GreedyStream both run it.

RNNTModel.greedy_streams(n) returns a GreedyStreamGroup: n independent greedy streams of one model.  With an rnnt_amd.LSTMPredictor
model the streams rest on the device between pushes and advance in lockstep (DESIGN.md §4p "Device stream").

Streaming beam search: RNNTModel.beam_stream() / beam_streams(n) return a BeamStream / a BeamStreamGroup whose n-best
list after any sequence of pushes equals RNNTModel.beam_search of the frames pushed so far — on the device bit for bit, from a block of
device memory the stream owns; HostBeamLoop is the host search made resumable, which beam_search's host path runs too.
"""
import math
import warnings

import torch


class HostGreedyLoop:
    """The host loop of greedy_decode (reference rnnt/model.py:95-125) over any number of calls of `run`: the tokens, the predictor's
    features (and a stateful predictor's state), the frame position and the labels emitted at it carry from one call to the next.
    `max_length` None: no cap.  `scan_frames` > 0 on a HIP device: the joint + argmax of that many frames per engine call
    (JointNetwork.greedy_scan); else the per-frame single_forward loop."""

    def __init__(self, model, max_length=None, max_symbols_per_frame=10, scan_frames=0):
        self.model = model
        self.max_length = max_length
        self.max_symbols_per_frame = int(max_symbols_per_frame)
        self.scan_frames = int(scan_frames)
        self.stateful = model._predictor_is_stateful()
        self.tokens = [model.joint.blank_idx]
        self.t, self.emitted = 0, 0
        self.feats, self.state = self._predict(self.tokens)

    @property
    def done(self):
        return self.max_length is not None and len(self.tokens) >= self.max_length

    def _predict(self, ids, state=None):
        dev = self.model.device
        ids_t = torch.tensor([ids], dtype=torch.int64, device=dev)
        if self.stateful:
            lens = torch.tensor([len(self.tokens)], dtype=torch.int64, device=dev)
            feats, _, st = (self.model.predictor(ids_t, lens) if state is None
                            else self.model.predictor(ids_t, lens, state))
            return feats, st
        return self.model.predictor(ids_t), None

    def run(self, audio):
        """Decode the frames of `audio` (1, n, C) — the encoder output after the permute of rnnt/model.py:93 — from the carried state.
        Returns (labels emitted, frames consumed); the position pauses at the end of the frames."""
        joint, tokens, m = self.model.joint, self.tokens, self.max_symbols_per_frame
        start = len(tokens)
        T = audio.shape[1]
        use_scan = self.scan_frames > 0 and audio.is_cuda
        if use_scan:
            frames = audio[0]  # [T,C] view of the encoder output; projected once for all frames
            if hasattr(joint, "audio_ln"):
                frames = joint.audio_ln(frames)
            frames = frames.float()
        t, emitted = self.t, self.emitted
        while t < T and (self.max_length is None or len(tokens) < self.max_length):
            if emitted >= m:  # reference: max_outputs_per_step reached -> next frame, whatever the token
                t += 1
                emitted = 0
                continue
            if use_scan:
                n = min(self.scan_frames, T - t)
                res = joint.greedy_scan(frames, self.feats[0, -1, :].float(), t, n)
                t_hit, tok = res[:2].tolist()  # the one sync of this block
                if t_hit > t:
                    emitted = 0
                t = t_hit
                if tok == joint.blank_idx:  # every scanned frame said blank
                    continue
            else:
                logits = joint.single_forward(audio[:, t, :], self.feats[:, -1, :])
                tok = int(logits.argmax(dim=-1))
                if tok == joint.blank_idx:
                    t += 1
                    emitted = 0
                    continue
            tokens.append(tok)
            self.feats, self.state = self._predict([tok], self.state) if self.stateful else self._predict(tokens)
            emitted += 1
        consumed = min(t, T)
        self.t, self.emitted = t - consumed, emitted
        return tokens[start:], consumed


def _to_device(x, dev):
    if torch.is_tensor(x):
        return x.to(dev)
    if isinstance(x, (list, tuple)):
        return type(x)(_to_device(v, dev) for v in x)
    return x


def _featurize_push(stream, samples, what):
    """push_audio's front half, shared by GreedyStream and BeamStream: featurize one chunk of samples — (time,) or (1, time), fp32 or
    int16, any length — from the sample state the stream keeps on the model's device (model.featurizer.streaming_forward) and append
    the new frames to the stream's pending buffer.  Returns the pending (1, F, L) frames when the encoder can take them now, else None.
    An rnnt_amd.AudioEncoder is asked through its own length arithmetic (`_lengths`: host ints, no launch) whether the push would
    raise — no prologue output frame yet, or an instance norm over a single frame — and the frames are held back while it would; any
    other encoder gets them as soon as there is one."""
    from .encoder import AudioEncoder
    model = stream.model
    feat = getattr(model, "featurizer", None)
    if feat is None:
        raise TypeError(f"{what} needs model.featurizer (e.g. rnnt_amd.TFJSSpectrogram); push takes mel features directly")
    if samples.dim() == 1:
        samples = samples[None]
    if samples.dim() != 2 or samples.shape[0] != 1:
        raise ValueError(f"{what} takes one chunk of samples (time,) or (1, time), got {tuple(samples.shape)}")
    dev = model.device
    if stream._audio_state is None:
        stream._audio_state = feat.streaming_init_state(1).to(dev)
    frames, stream._audio_state = feat.streaming_forward(samples.to(dev), stream._audio_state)
    if frames.shape[2]:
        stream._pending = frames if stream._pending is None else torch.cat((stream._pending, frames), dim=2)
    if stream._pending is None:
        return None
    enc = model.encoder
    if isinstance(enc, AudioEncoder):
        if stream._enc_state is None:
            stream._enc_state = _to_device(enc.streaming_init_state(1), dev)
        try:
            enc._lengths(int(stream._pending.shape[2]), [int(s.shape[2]) for s in stream._enc_state])
        except ValueError:
            return None
    return stream._pending


class GreedyStream:
    """One utterance decoded push by push (RNNTModel.greedy_stream).  `push_encoded(audio_features)` takes a chunk of encoder output
    (1, C, n) as `encoder(...)` / `encoder.streaming_forward` return it and returns the labels it emitted; `push(mel_chunk)` runs the
    encoder's streaming_forward on a (1, F, L) mel chunk first.  `tokens`: every label so far, `frames`: frames consumed, `done`: the
    max_length cap was reached (later pushes consume nothing and return []), `last_path`: "persistent", "loop" or "host" — the path
    that served the last push with frames.

    With the engine's ConvPredictor in eval mode and fp32 HIP tensors of sizes the decode kernels cover, every push runs on the device
    from a state block it keeps there (rnnt_engine_greedy_stream_decode): the persistent launch where the engine takes the push's sizes,
    else the kernel-per-layer loop (`persistent=True/False` forces one), with ONE host synchronisation per push — two when a persistent
    push meets an activation beyond +-30 or gives up waiting for a hand-off and is redone on the loop.  The decode tables are built when
    the stream is created: the model's weights must not change while a stream is open.  Everything else, the CPU included, runs
    HostGreedyLoop — with `device_loop=None` that includes every rnnt_amd.LSTMPredictor model, as before; `device_loop=True` makes such a
    stream a device GreedyStreamGroup of one (`last_path` "lstm_stream", one synchronisation per push; DESIGN.md §4p "Device stream") and
    raises where no device path applies, `device_loop=False` forces the host loop for any model.  The encoder's mode is the caller's business: the reference's BatchNorm encoder must be in eval() for its streaming
    output to equal its whole-utterance output."""

    def __init__(self, model, max_length=None, max_symbols_per_frame=10, persistent=None, device_loop=None, scan_frames=32):
        from . import engine
        self.model = model
        self.max_length = None if max_length is None else int(max_length)
        self.max_symbols_per_frame = int(max_symbols_per_frame)
        if self.max_symbols_per_frame < 1:
            raise ValueError(f"greedy_stream: max_symbols_per_frame={max_symbols_per_frame} must be >= 1")
        self.persistent = persistent
        self.tokens = []
        self.frames = 0
        self.last_path = None
        self._done = self.max_length is not None and self.max_length < 2  # (the reference's loop never runs: tokens = [blank] is full)
        self._enc_state = None
        self._audio_state = None  # push_audio: the samples no frame has consumed yet (1, n), on the model's device
        self._pending = None      # push_audio: frames featurized but not yet taken by the encoder (1, F, L)
        dev = model.device
        self._on_device = (device_loop is not False and dev.type == "cuda" and not model._predictor_is_stateful()
                           and model._device_loop_ok(torch.zeros(1, 1, device=dev)))
        self._host = None
        self._tables = None
        self._group = None
        if device_loop and not self._on_device:
            # an LSTM model: a device group of one (raises where the device path does not apply, as for any other predictor)
            self._group = GreedyStreamGroup(model, 1, max_length, max_symbols_per_frame, scan_frames, device_loop=True)
        elif self._on_device:
            self._sizes = model._decode_sizes()
            if persistent is not False and engine.greedy_decode_persistent_supported(8, *self._sizes):
                self._tables = model._decode_tables()  # once per stream, from the weights as they are now
            self._buf = torch.empty(engine.STREAM_STATE_WORDS + 16, dtype=torch.int32, device=dev)  # state block | the push's labels
            engine.greedy_stream_init(self._buf[:engine.STREAM_STATE_WORDS], model.joint.blank_idx)
        else:
            self._host = HostGreedyLoop(model, self.max_length, self.max_symbols_per_frame, scan_frames=max(0, min(int(scan_frames), 128)))

    @property
    def done(self):
        return self._done

    def lstm_state(self):
        """Test aid: clones of (LSTM state [L, 2, Hd], text vector [H]) of a stream that is a device group of one."""
        return self._group.lstm_state(0)

    @torch.no_grad()
    def push(self, mel_chunk):
        """Run the encoder's streaming_forward on `mel_chunk` (1, F, L) with the state it carries (streaming_init_state(1) on the first
        push, moved to the model's device), then push_encoded its output.  Returns the new labels."""
        enc = self.model.encoder
        if not (callable(getattr(enc, "streaming_forward", None)) and callable(getattr(enc, "streaming_init_state", None))):
            raise TypeError(f"GreedyStream.push needs an encoder with streaming_forward(x, state) and streaming_init_state(batch_size); "
                            f"{type(enc).__name__} lacks them (push_encoded takes encoder output directly)")
        if mel_chunk.dim() != 3 or mel_chunk.shape[0] != 1:
            raise ValueError(f"GreedyStream.push takes one mel chunk (1, F, L), got {tuple(mel_chunk.shape)}")
        if self._done:
            return []
        if self._enc_state is None:
            self._enc_state = _to_device(enc.streaming_init_state(1), self.model.device)
        out, self._enc_state = enc.streaming_forward(mel_chunk, self._enc_state)
        return self.push_encoded(out)

    @torch.no_grad()
    def push_audio(self, samples):
        """Featurize one chunk of samples — (time,) or (1, time), fp32 or int16, any length — with model.featurizer from the sample
        state the stream carries, then `push` the frames that are pending.  Frames an rnnt_amd.AudioEncoder cannot take yet (no
        prologue output frame, an instance norm over one frame) wait for the next push; if `push` raises, they are kept.  Returns
        the new labels."""
        if self._done:
            return []
        mel = _featurize_push(self, samples, "GreedyStream.push_audio")
        if mel is None:
            return []
        new = self.push(mel)
        self._pending = None
        return new

    @torch.no_grad()
    def push_encoded(self, audio_features):
        """Decode one chunk of encoder output (1, C, n), n >= 0, from where the stream stands.  Returns the new labels (list of int)."""
        if audio_features.dim() != 3 or audio_features.shape[0] != 1:
            raise ValueError(f"GreedyStream.push_encoded takes one chunk of encoder output (1, C, n), got {tuple(audio_features.shape)}")
        if self._done:
            return []
        if self._group is not None:
            new = self._group.push_encoded([audio_features])[0]
            self.frames, self._done = self._group.frames[0], self._group.done[0]
            self.last_path = self._group.last_path or self.last_path
            self.tokens.extend(new)
            return new
        audio = audio_features.permute(0, 2, 1)  # (1, n, C), as rnnt/model.py:93
        new = self._push_device(audio) if self._on_device else self._push_host(audio)
        self.tokens.extend(new)
        return new

    def _push_host(self, audio):
        if audio.shape[1] == 0:
            return []
        new, consumed = self._host.run(audio)
        self.frames += consumed
        self._done = self._host.done
        self.last_path = "host"
        return new

    def _push_device(self, audio):
        from . import engine
        frames = self.model._decode_frames(audio)
        if frames.device != self._buf.device:
            raise ValueError(f"GreedyStream: the stream lives on {self._buf.device}, the chunk on {frames.device}")
        n = frames.shape[0]
        if n == 0:
            return []
        W, m, ml = engine.STREAM_STATE_WORDS, self.max_symbols_per_frame, self.max_length or 0
        cap = n * m if ml == 0 else min(n * m, ml - 1)
        if self._buf.numel() < W + cap:  # grows with the largest push, never with the stream
            buf = torch.empty(W + cap, dtype=torch.int32, device=self._buf.device)
            buf[:W].copy_(self._buf[:W])
            self._buf = buf
        persistent = self.persistent
        if persistent is None:
            persistent = self._tables is not None and engine.greedy_stream_supported(n, *self._sizes, ml, m)
        args = (frames, *self.model._decode_bundle(), ml, m, self._tables)

        def run(persist):
            engine.greedy_stream_decode(*args, persist, self._buf[:W], self._buf[W:W + cap])
            h = self._buf[:W + cap].cpu()  # the push's one synchronisation
            return h[:W].tolist(), h

        st, h = run(bool(persistent))
        path = "persistent" if persistent else "loop"
        if st[engine.STREAM_STATUS] != 0:
            # the persistent launch did not decode this push and left the stream's state as it was: 10 / 11 an audio frame or a text
            # vector beyond +-30 (exact on the loop, which takes tanh of the sum: no warning), else a hand-off that never arrived
            code = st[engine.STREAM_STATUS]
            if code not in engine.DECODE_RANGE_CODES:
                warnings.warn(f"rnnt_amd: the persistent stream decode gave up at hand-off {code}; "
                              "redoing the push on the kernel-per-layer loop", RuntimeWarning)
            st, h = run(False)
            path = "loop"
            if st[engine.STREAM_STATUS] != 0:
                raise RuntimeError(f"rnnt_engine: the stream decode's loop reported status {st[engine.STREAM_STATUS]}")
        self.frames = st[engine.STREAM_FRAMES]
        self._done = bool(st[engine.STREAM_DONE])
        self.last_path = path
        return h[W:W + st[engine.STREAM_PUSH_LABELS]].tolist()


class GreedyStreamGroup:
    """`n` (1 .. 32) independent utterances greedy-decoded push by push (RNNTModel.greedy_streams; DESIGN.md §4p "Device stream").
    `push_encoded(chunks)` takes a list of n chunks of encoder output, each (1, C, k_i) with k_i >= 0, or None for a stream that sits
    the push out, and returns the list of each stream's new labels.  Per stream i: `tokens[i]` every label so far — `greedy_decode` of
    the frames stream i has been pushed so far with the same max_length and max_symbols_per_frame, whatever the chunking and whatever the
    other streams do —, `frames[i]` the frames consumed, `done[i]` the max_length cap was reached (later pushes consume nothing and
    return []); `reset(i)` starts a new utterance in slot i; `last_path`: "lstm_stream" or "host".

    With an rnnt_amd.LSTMPredictor model that the device decode loop takes (eval mode or p = 0, fp32 HIP tensors, backend not "torch",
    sizes the kernels cover) the streams rest on the device between pushes, in ONE block the group owns: LSTM state, text vectors and
    the loop's words (rnnt_engine_greedy_stream_lstm_push).  A push advances all streams in lockstep through one kernel sequence per
    iteration and ends in ONE host synchronisation; a stream's labels and state are bit for bit those of the same frames decoded alone
    by the offline device loop.  The parameters are read live at every push, but the carried state is a function of the weights that
    produced it: do not change them while a group is open.  Everything else — the CPU, backend "torch", a training-mode predictor with
    dropout, sizes the kernels refuse, any other predictor (ConvPredictor models included) — runs n host streams (HostGreedyLoop) and
    returns the same results; `device_loop=True` raises where the device path does not apply, `device_loop=False` forces the host.
    `device_loop=None` takes the device path where it applies AND n >= DEVICE_MIN_STREAMS: at the reference's widths the device group beat
    n host streams at every timed shape from n = 4 on (1000 frames in 50-frame pushes: 4.5x at n = 4, 16x at n = 32; in 1-frame pushes:
    1.45x and 3.5x), but ONE stream lost in 1-frame pushes (0.24 ms against 0.06 ms per push: a push enqueues 34 launches where the host
    loop makes one scan call) while winning 2.5x in 50-frame pushes; n = 2 and 3 were not timed and stay on the host
    (profiles/lstm_stream_bench.txt)."""

    DEVICE_MIN_STREAMS = 4

    def __init__(self, model, n, max_length=None, max_symbols_per_frame=10, scan_frames=32, device_loop=None):
        from . import engine
        n, m = int(n), int(max_symbols_per_frame)
        if not 1 <= n <= engine.LSTM_STREAM_MAX:
            raise ValueError(f"greedy_streams: n={n} outside [1, {engine.LSTM_STREAM_MAX}]")
        if m < 1:
            raise ValueError(f"greedy_streams: max_symbols_per_frame={max_symbols_per_frame} must be >= 1")
        self.model, self.n = model, n
        self.max_length = None if max_length is None else int(max_length)
        self.max_symbols_per_frame = m
        self.scan_frames = max(1, min(int(scan_frames) if int(scan_frames) > 0 else 32, 128))
        self.tokens = [[] for _ in range(n)]
        self.frames = [0] * n
        self.last_path = None
        self._capped = self.max_length is not None and self.max_length < 2  # (the reference's loop never runs: tokens = [blank] is full)
        self._done = [self._capped] * n
        dev = model.device
        ok = dev.type == "cuda" and model._predictor_is_lstm() and model._device_loop_ok(torch.zeros(1, 1, device=dev))
        if ok:
            joint = model.joint
            self._dims = (*model.predictor._decode_sizes(), joint.joint_ln.in_features, joint.joint_ln.out_features, hasattr(joint, "text_ln"))
            ok = engine.greedy_stream_lstm_supported(n, *self._dims, self.scan_frames)
        if device_loop and not ok:
            raise RuntimeError("greedy_streams(device_loop=True) needs the engine's LSTMPredictor in eval mode on a HIP device "
                               "(fp32, backend not \"torch\", sizes the decode kernels cover)")
        self._on_device = (ok and n >= self.DEVICE_MIN_STREAMS) if device_loop is None else bool(device_loop)
        if self._on_device:
            _, _, Hd, _, L, _, H, _, _ = self._dims
            self._block = torch.zeros(engine.greedy_stream_lstm_bytes(n, *self._dims), dtype=torch.uint8, device=dev)
            self._state, self._hc, self._text = engine.greedy_stream_lstm_views(self._block, n, L, Hd, H)
            self._out = torch.zeros(n, 16, dtype=torch.int32, device=dev)  # the push's labels; grows with the largest push, never with a stream
            engine.greedy_stream_lstm_init(self._block, n, L, Hd, H, model.joint.blank_idx)
        else:
            self._streams = [self._host_stream() for _ in range(n)]

    def _host_stream(self):
        return GreedyStream(self.model, self.max_length, self.max_symbols_per_frame, device_loop=False, scan_frames=self.scan_frames)

    @property
    def done(self):
        return list(self._done)

    def reset(self, i):
        """Stream i starts a new utterance (the others are untouched)."""
        i = range(self.n)[i]
        if self._on_device:
            from . import engine
            _, _, Hd, _, L, _, H, _, _ = self._dims
            engine.greedy_stream_lstm_init(self._block, self.n, L, Hd, H, self.model.joint.blank_idx, index=i)
        else:
            self._streams[i] = self._host_stream()
        self.tokens[i] = []
        self.frames[i] = 0
        self._done[i] = self._capped

    def lstm_state(self, i):
        """Test aid: clones of (LSTM state [L, 2, Hd], text vector [H]) of stream i as it rests — after the last label taken in, the zero
        state before the stream's first frame."""
        i = range(self.n)[i]
        if self._on_device:
            return self._hc[:, :, i].clone(), self._text[i].clone()
        loop = self._streams[i]._host
        text = loop.feats[0, -1]
        if hasattr(self.model.joint, "text_ln"):
            text = self.model.joint.text_ln(text)
        return torch.stack([torch.stack((h[0], c[0])) for h, c in loop.state]), text.clone()

    @torch.no_grad()
    def push_encoded(self, chunks):
        """One push: `chunks[i]` is stream i's next chunk of encoder output (1, C, k_i), k_i >= 0, or None.  Returns the list of the
        streams' new labels."""
        chunks = list(chunks)
        if len(chunks) != self.n:
            raise ValueError(f"GreedyStreamGroup.push_encoded takes {self.n} chunks (None for a stream without new frames), got {len(chunks)}")
        for c in chunks:
            if c is not None and (c.dim() != 3 or c.shape[0] != 1):
                raise ValueError(f"a greedy stream takes one chunk of encoder output (1, C, n), got {tuple(c.shape)}")
        # (a done stream consumes nothing: it sits every later push out)
        chunks = [None if c is None or c.shape[2] == 0 or self._done[i] else c for i, c in enumerate(chunks)]
        new = [[] for _ in range(self.n)]
        if any(c is not None for c in chunks):
            (self._push_device if self._on_device else self._push_host)(chunks, new)
            for i, labels in enumerate(new):
                self.tokens[i].extend(labels)
        return new

    def _push_host(self, chunks, new):
        for i, c in enumerate(chunks):
            if c is None:
                continue
            s = self._streams[i]
            new[i] = s.push_encoded(c)
            self.frames[i], self._done[i] = s.frames, s.done
        self.last_path = "host"

    def _push_device(self, chunks, new):
        from . import engine
        model, n, m = self.model, self.n, self.max_symbols_per_frame
        frames = [None if c is None else model._decode_frames(c.permute(0, 2, 1)) for c in chunks]  # (1, k, C), as rnnt/model.py:93
        for f in frames:
            if f is not None and f.device != self._block.device:
                raise ValueError(f"greedy streams: the group lives on {self._block.device}, the chunk on {f.device}")
        cap = max(f.shape[0] for f in frames if f is not None) * m
        if self._out.shape[1] < cap:
            self._out = torch.zeros(n, cap, dtype=torch.int32, device=self._block.device)
        joint = model.joint
        tl = getattr(joint, "text_ln", None)
        engine.greedy_stream_lstm_push(frames, model.predictor._decode_bundle(), tl.weight if tl is not None else None,
                                       tl.bias if tl is not None else None, joint.joint_ln.weight, joint.joint_ln.bias, joint.blank_idx,
                                       self.max_length or 0, m, self.scan_frames, self._block, self._out)
        W = engine.LSTM_STREAM_STATE_WORDS
        host = torch.cat((self._state.reshape(-1), self._out.reshape(-1))).cpu()  # the push's one synchronisation
        sts, out = host[:n * W].view(n, W).tolist(), host[n * W:].view(n, -1)
        for i, (f, st) in enumerate(zip(frames, sts)):
            if f is None:
                continue
            done = bool(st[engine.LSTM_STREAM_DONE])
            if not st[engine.LSTM_STREAM_AT_REST] or (not done and st[engine.LSTM_STREAM_FRAMES] != self.frames[i] + f.shape[0]):
                raise RuntimeError(f"rnnt_engine: greedy stream {i} did not consume its push (frames={st[engine.LSTM_STREAM_FRAMES]}, "
                                   f"{st[engine.LSTM_STREAM_PUSH_ITERATIONS]} iterations)")
            new[i] = out[i, :st[engine.LSTM_STREAM_PUSH_LABELS]].tolist()
            self.frames[i], self._done[i] = st[engine.LSTM_STREAM_FRAMES], done
        model.predictor.last_backend = "engine"
        self.last_path = "lstm_stream"


class HostBeamLoop:
    """The search of DESIGN.md §4h as a host loop over any number of calls of `run`: the predictor on the whole history of each new
    hypothesis (cached by sequence), single_forward batched over the round's active hypotheses, scores as Python floats (double).  The
    beam after the last frame carries to the next call; `nbest` is beam_search's result for the frames so far.  With an
    rnnt_amd.LSTMPredictor (DESIGN.md §4h "LSTM") the cache holds (text vector, LSTM state) by sequence and a new hypothesis takes ONE
    predictor step from its parent's state — the parent is always cached: an active of the round before or a member of the carried beam.
    With a `context`
    (ContextGraph; DESIGN.md §4h "Context") a label candidate takes delta(node, k) — the WHOLE log-probability row is biased before the
    slot's top-`beam` is taken, never only the labels the raw row would have offered —, the carried beam holds internal scores and `nbest`
    is its finalised view."""

    def __init__(self, model, beam_size, max_length, max_symbols_per_frame=10, context=None):
        self.model = model
        self.context = context
        self._nodes = {}  # sequence -> node of the context graph (a function of the sequence)
        self.beam_size, self.max_length, self.m = int(beam_size), int(max_length), int(max_symbols_per_frame)
        self.beam = [((), 0.0)]
        self.frames = 0
        self._feats = {}
        self._lstm = model._predictor_is_lstm()

    @property
    def nbest(self):
        if self.context is not None:
            return self.context.finalise(self.beam)
        return [(list(y), s) for y, s in self.beam]

    def _node(self, y):
        if not y:
            return 0
        if y not in self._nodes:  # (a new hypothesis extends one of the beam's: one step)
            self._nodes[y] = self.context.step(self._node(y[:-1]), y[-1])[0]
        return self._nodes[y]

    def _text(self, y):
        if self._lstm:
            if y not in self._feats:  # one step from the state after y[:-1], fed y[-1]; the start: the blank from zero state
                dev = self.model.device
                ids = torch.tensor([[y[-1] if y else self.model.joint.blank_idx]], dtype=torch.int64, device=dev)
                out, _, state = self.model.predictor(ids, torch.ones(1, dtype=torch.int64, device=dev),
                                                     self._feats[y[:-1]][1] if y else None)
                self._feats[y] = (out[0, -1], state)
            return self._feats[y][0]
        if y not in self._feats:
            ids = torch.tensor([[self.model.joint.blank_idx, *y]], dtype=torch.int64, device=self.model.device)
            self._feats[y] = self.model.predictor(ids)[0, -1]
        return self._feats[y]

    @staticmethod
    def _lae(a, b):
        hi, lo = max(a, b), min(a, b)
        return hi if lo == -math.inf else hi + math.log1p(math.exp(lo - hi))

    def run(self, audio):
        """Search the frames of `audio` (1, n, C) from the carried beam."""
        joint, blank, beam_size, max_length, m, lae, text = (self.model.joint, self.model.joint.blank_idx, self.beam_size, self.max_length,
                                                             self.m, self._lae, self._text)
        beam = self.beam
        for t in range(audio.shape[1]):
            active, fin = beam, []  # fin: [[y, score]] in order of arrival
            for r in range(m):
                frame = audio[:, t, :].expand(len(active), -1)
                lp = joint.single_forward(frame, torch.stack([text(y) for y, _ in active])).double().log_softmax(-1).cpu()
                for i, (y, s) in enumerate(active):  # blank candidates join N, merged by sequence
                    b = s + float(lp[i, blank])
                    hit = next((e for e in fin if e[0] == y), None)
                    if hit is not None:
                        hit[1] = lae(hit[1], b)
                    else:
                        fin.append([y, b])
                cands = [(s, 0, f, 0, y) for f, (y, s) in enumerate(fin)]
                for i, (y, s) in enumerate(active):
                    if len(y) >= max_length - 1:
                        continue
                    row = lp[i].clone()
                    if self.context is not None:
                        row += torch.from_numpy(self.context.delta_row(self._node(y), row.shape[0]))
                    row[blank] = -math.inf
                    vals, idx = torch.sort(row, descending=True, stable=True)  # lower id first among equal values
                    for v, k in zip(vals[:beam_size].tolist(), idx[:beam_size].tolist()):
                        if v != -math.inf:
                            cands.append((s + v, 1, i, k, y + (k,)))
                cands.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
                kept = cands[:beam_size]
                fin = [[c[4], c[0]] for c in kept if c[1] == 0]
                active = [(c[4], c[0]) for c in kept if c[1] == 1]
                if not active:
                    break
            # the cap: labels still active after round m-1 move on without a blank term, merged with N by sequence
            for y, s in active:
                hit = next((e for e in fin if e[0] == y), None)
                if hit is not None:
                    hit[1] = lae(hit[1], s)
                else:
                    fin.append([y, s])
            order = sorted(range(len(fin)), key=lambda i: (-fin[i][1], i))
            beam = [(fin[i][0], fin[i][1]) for i in order]
        self.beam = beam
        self.frames += audio.shape[1]
        live = {y for y, _ in beam}  # (only the beam's text vectors are needed again; the others would only grow with the stream)
        if self._lstm:  # (a capped label has not taken its step yet: take it while its parent's state is still cached)
            for y, _ in beam:
                text(y)
        self._feats = {y: f for y, f in self._feats.items() if y in live}
        if self.context is not None:
            self._nodes = {y: self._node(y) for y in live}


def _common_prefix(lists):
    out = list(lists[0])
    for y in lists[1:]:
        k = 0
        while k < len(out) and k < len(y) and out[k] == y[k]:
            k += 1
        del out[k:]
    return out


class BeamStreamGroup:
    """`n` (1 .. 64) independent utterances beam-searched push by push (RNNTModel.beam_streams).
    `push_encoded(chunks)` takes a list of n chunks of encoder output, each (1, C, k_i) or None, and returns every stream's current best
    token list.  Per stream i: `nbest[i]` = [(tokens, log-probability), ...] best first — exactly `beam_search(..., return_nbest=True)` of
    the frames stream i has been pushed so far, whatever the chunking and whatever the other streams do; `tokens[i]` the best entry;
    `stable[i]` the longest common prefix of the beam's entries (every later hypothesis extends one of them, so it can only grow and
    stays a prefix of every later best entry); `frames[i]` the frames consumed; `reset(i)` starts a new utterance in slot i.  A beam stream
    has no `done`: max_length only stops hypotheses growing, as in beam_search.

    With the engine's ConvPredictor in eval mode, fp32 HIP tensors, sizes the beam kernels cover and beam_size <= 16 the searches rest on
    the device between pushes, in a block the group owns (rnnt_engine_beam_stream_push: all streams advance through ONE kernel sequence
    per round, one host synchronisation per push); the decode tables are built when the group is created, so the model's weights must not
    change while it is open.  Everything else, the CPU and every rnnt_amd.LSTMPredictor model included (a device stream with LSTM state is
    out of scope, DESIGN.md §4h "LSTM"), runs one HostBeamLoop per stream (`last_path`: "device" or "host").
    With a `context` (ContextGraph; DESIGN.md §4h "Context") every stream runs the host loop — the device stream with a context graph is
    out of scope so far (§4l) —, the carried beams are internal and `nbest`, `tokens`, `stable` their finalised views."""

    def __init__(self, model, n, beam_size=4, max_length=200, max_symbols_per_frame=10, context=None):
        from . import engine
        self.context = context  # (a ContextGraph that can change the search, or None: RNNTModel._beam_context)
        n, beam_size, max_length, m = int(n), int(beam_size), int(max_length), int(max_symbols_per_frame)
        if beam_size < 1 or m < 1:
            raise ValueError(f"beam_stream: beam_size={beam_size} and max_symbols_per_frame={m} must be >= 1")
        if not 1 <= n <= engine.BEAM_STREAM_MAX:
            raise ValueError(f"beam_streams: n={n} outside [1, {engine.BEAM_STREAM_MAX}]")
        lstm = model._predictor_is_lstm()  # (rnnt_amd.LSTMPredictor: the host loop; a device stream with LSTM state is out of scope)
        if model._predictor_is_stateful() and not lstm:
            raise NotImplementedError("beam_stream needs a stateless predictor (forward(ids), e.g. ConvPredictor); "
                                      "stateful (LSTM) predictors are not supported")
        self.model, self.n = model, n
        self.beam_size, self.max_length, self.max_symbols_per_frame = beam_size, max_length, m
        self.nbest = [[([], 0.0)] for _ in range(n)]
        self.frames = [0] * n
        self.last_path = None
        dev = model.device
        # (with a context graph: the host loop — the device stream carries no node per slot yet)
        self._on_device = not lstm and context is None and dev.type == "cuda" and model._beam_device_ok(torch.zeros(1, 1, device=dev), beam_size, max_length)
        if self._on_device:
            self._sizes = model._decode_sizes()
            self._on_device = engine.beam_stream_supported(*self._sizes, max_length, beam_size, n)
        if self._on_device:
            self._tables = model._decode_tables()  # once per group, from the weights as they are now
            self._block = torch.zeros(engine.beam_stream_bytes(*self._sizes, max_length, beam_size, n), dtype=torch.uint8, device=dev)
            # scores | state | tokens in one buffer: ONE device-to-host copy reads a push's whole result
            self._cut = (8 * n * beam_size, 8 * n * beam_size + 4 * 32 * n)
            self._res = torch.zeros(self._cut[1] + 4 * n * beam_size * max_length, dtype=torch.uint8, device=dev)
            self._scores, self._state, self._tokens = self._views(self._res)
            engine.beam_stream_init(self._sizes, max_length, beam_size, model.joint.blank_idx, self._state, self._scores, self._block)
        else:
            self._loops = [HostBeamLoop(model, beam_size, max_length, m, context) for _ in range(n)]

    def _views(self, res):
        n, beam, a, b = self.n, self.beam_size, *self._cut
        return (res[:a].view(torch.float64).view(n, beam), res[a:b].view(torch.int32).view(n, 32),
                res[b:].view(torch.int32).view(n, beam, self.max_length))

    @property
    def tokens(self):
        return [list(nb[0][0]) for nb in self.nbest]

    @property
    def stable(self):
        return [_common_prefix([y for y, _ in nb]) for nb in self.nbest]

    def reset(self, i):
        """Stream i starts a new utterance (the others are untouched)."""
        i = range(self.n)[i]
        if self._on_device:
            from . import engine
            engine.beam_stream_init(self._sizes, self.max_length, self.beam_size, self.model.joint.blank_idx, self._state, self._scores,
                                    self._block, index=i)
        else:
            self._loops[i] = HostBeamLoop(self.model, self.beam_size, self.max_length, self.max_symbols_per_frame, self.context)
        self.nbest[i] = [([], 0.0)]
        self.frames[i] = 0

    @torch.no_grad()
    def push_encoded(self, chunks):
        """One push: `chunks[i]` is stream i's next chunk of encoder output (1, C, k_i), k_i >= 0, or None.  Returns the list of the
        streams' best token lists."""
        chunks = list(chunks)
        if len(chunks) != self.n:
            raise ValueError(f"BeamStreamGroup.push_encoded takes {self.n} chunks (None for a stream without new frames), got {len(chunks)}")
        audios = []
        for c in chunks:
            if c is not None and (c.dim() != 3 or c.shape[0] != 1):
                raise ValueError(f"a beam stream takes one chunk of encoder output (1, C, n), got {tuple(c.shape)}")
            audios.append(None if c is None or c.shape[2] == 0 else c.permute(0, 2, 1))  # (1, n, C), as rnnt/model.py:93
        if any(a is not None for a in audios):
            (self._push_device if self._on_device else self._push_host)(audios)
        return self.tokens

    def _push_host(self, audios):
        for i, a in enumerate(audios):
            if a is None:
                continue
            self._loops[i].run(a)
            self.nbest[i] = self._loops[i].nbest
            self.frames[i] = self._loops[i].frames
        self.last_path = "host"

    def _push_device(self, audios):
        from . import engine
        frames = [None if a is None else self.model._decode_frames(a) for a in audios]
        for f in frames:
            if f is not None and f.device != self._res.device:
                raise ValueError(f"beam stream: the stream lives on {self._res.device}, the chunk on {f.device}")
        engine.beam_stream_push(frames, *self.model._decode_bundle(), self.max_length, self.beam_size,
                                self.max_symbols_per_frame, self._tables, self._state, self._tokens, self._scores, self._block)
        scores, state, tokens = self._views(self._res.cpu())  # the push's one synchronisation
        sts, toks, scs = state.tolist(), tokens.tolist(), scores.tolist()
        for i, (f, st) in enumerate(zip(frames, sts)):
            if f is None:
                continue
            if not st[engine.BEAM_STREAM_AT_REST] or st[engine.BEAM_STREAM_FRAMES] != self.frames[i] + f.shape[0]:
                raise RuntimeError(f"rnnt_engine: beam stream {i} did not consume its push (frames={st[engine.BEAM_STREAM_FRAMES]}, "
                                   f"{st[5]} rounds)")
            self.frames[i] = st[engine.BEAM_STREAM_FRAMES]
            self.nbest[i] = self.model._nbest(st, toks[i], scs[i])
        self.last_path = "device"


class BeamStream:
    """One utterance beam-searched push by push (RNNTModel.beam_stream): a BeamStreamGroup of one, with the encoder's
    streaming state.  `push_encoded(audio_features)` takes a chunk of encoder output (1, C, n), n >= 0, `push(mel_chunk)` runs the encoder's
    streaming_forward on a (1, F, L) mel chunk first; both return the current best hypothesis's FULL token list (the best entry can
    change from push to push — `stable` is the part that cannot).  `nbest`, `tokens`, `stable`, `frames`, `last_path` as the group's, for
    the one stream; `reset()` starts a new utterance on the same block and tables."""

    def __init__(self, model, beam_size=4, max_length=200, max_symbols_per_frame=10, context=None):
        self.model = model
        self._group = BeamStreamGroup(model, 1, beam_size, max_length, max_symbols_per_frame, context)
        self._enc_state = None
        self._audio_state = None  # push_audio: the samples no frame has consumed yet (1, n), on the model's device
        self._pending = None      # push_audio: frames featurized but not yet taken by the encoder (1, F, L)

    nbest = property(lambda self: self._group.nbest[0])
    tokens = property(lambda self: self._group.tokens[0])
    stable = property(lambda self: self._group.stable[0])
    frames = property(lambda self: self._group.frames[0])
    last_path = property(lambda self: self._group.last_path)

    def reset(self):
        self._group.reset(0)
        self._enc_state = None
        self._audio_state = None
        self._pending = None

    @torch.no_grad()
    def push(self, mel_chunk):
        """Run the encoder's streaming_forward on `mel_chunk` (1, F, L) with the state it carries (streaming_init_state(1) on the first
        push, moved to the model's device), then push_encoded its output."""
        enc = self.model.encoder
        if not (callable(getattr(enc, "streaming_forward", None)) and callable(getattr(enc, "streaming_init_state", None))):
            raise TypeError(f"BeamStream.push needs an encoder with streaming_forward(x, state) and streaming_init_state(batch_size); "
                            f"{type(enc).__name__} lacks them (push_encoded takes encoder output directly)")
        if mel_chunk.dim() != 3 or mel_chunk.shape[0] != 1:
            raise ValueError(f"BeamStream.push takes one mel chunk (1, F, L), got {tuple(mel_chunk.shape)}")
        if self._enc_state is None:
            self._enc_state = _to_device(enc.streaming_init_state(1), self.model.device)
        out, self._enc_state = enc.streaming_forward(mel_chunk, self._enc_state)
        return self.push_encoded(out)

    @torch.no_grad()
    def push_audio(self, samples):
        """Featurize one chunk of samples — (time,) or (1, time), fp32 or int16, any length — with model.featurizer from the sample
        state the stream carries, then `push` the frames that are pending (held back and kept as GreedyStream.push_audio does)."""
        mel = _featurize_push(self, samples, "BeamStream.push_audio")
        if mel is None:
            return self.tokens
        best = self.push(mel)
        self._pending = None
        return best

    @torch.no_grad()
    def push_encoded(self, audio_features):
        """Search one chunk of encoder output (1, C, n), n >= 0, from where the stream stands.  Returns the best token list."""
        if audio_features.dim() != 3 or audio_features.shape[0] != 1:
            raise ValueError(f"BeamStream.push_encoded takes one chunk of encoder output (1, C, n), got {tuple(audio_features.shape)}")
        return self._group.push_encoded([audio_features])[0]
