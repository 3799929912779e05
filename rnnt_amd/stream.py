"""Streaming greedy decode: RNNTModel.greedy_stream() returns a GreedyStream that decodes chunk by chunk, carrying
the loop of the reference's greedy decode (rnnt/model.py:108-125) from one push of encoder frames to the next.  For every way of
cutting an utterance into pushes, empty ones included, the labels of the pushes concatenated equal RNNTModel.greedy_decode of all
frames at once with the same max_length, wherever the argmax is not a rounding-level tie.

HostGreedyLoop is greedy_decode's host loop made resumable; greedy_decode and the host path of GreedyStream both run it.
"""
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
    HostGreedyLoop.  The encoder's mode is the caller's business: the reference's BatchNorm encoder must be in eval() for its streaming
    output to equal its whole-utterance output."""

    def __init__(self, model, max_length=None, max_symbols_per_frame=10, persistent=None):
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
        dev = model.device
        self._on_device = (dev.type == "cuda" and not model._predictor_is_stateful()
                           and model._device_loop_ok(torch.zeros(1, 1, device=dev)))
        self._host = None
        self._tables = None
        if self._on_device:
            p, joint = model.predictor, model.joint
            S, E = p.embedding.weight.shape
            self._sizes = (S, E, p.linear.out_features, joint.joint_ln.in_features, joint.joint_ln.out_features, hasattr(joint, "text_ln"))
            if persistent is not False and engine.greedy_decode_persistent_supported(8, *self._sizes):
                self._tables = model._decode_tables()  # once per stream, from the weights as they are now
            self._buf = torch.empty(engine.STREAM_STATE_WORDS + 16, dtype=torch.int32, device=dev)  # state block | the push's labels
            engine.greedy_stream_init(self._buf[:engine.STREAM_STATE_WORDS], joint.blank_idx)
        else:
            self._host = HostGreedyLoop(model, self.max_length, self.max_symbols_per_frame, scan_frames=32)

    @property
    def done(self):
        return self._done

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
    def push_encoded(self, audio_features):
        """Decode one chunk of encoder output (1, C, n), n >= 0, from where the stream stands.  Returns the new labels (list of int)."""
        if audio_features.dim() != 3 or audio_features.shape[0] != 1:
            raise ValueError(f"GreedyStream.push_encoded takes one chunk of encoder output (1, C, n), got {tuple(audio_features.shape)}")
        if self._done:
            return []
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
        model, joint = self.model, self.model.joint
        frames = audio[0]
        if hasattr(joint, "audio_ln"):  # per frame: the same numbers chunk by chunk
            frames = joint.audio_ln(frames)
        frames = frames.float().contiguous()
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
        p, tl = model.predictor, getattr(joint, "text_ln", None)
        args = (frames, p._params(), (float(p.input_layer_norm.eps), float(p.output_layer_norm.eps)),
                tl.weight if tl is not None else None, tl.bias if tl is not None else None,
                joint.joint_ln.weight, joint.joint_ln.bias, joint.blank_idx, ml, m, self._tables)

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
