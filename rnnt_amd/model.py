"""RNNTModel container with the reference's interface (rnnt/model.py:7-139); `forward`
routes the joint + loss through the fused HIP engine.  Encoder and predictor are whatever
torch modules the caller supplies: the engine's own (rnnt_amd.ConvPredictor, rnnt_amd.LSTMPredictor,
rnnt_amd.AudioEncoder) or stock PyTorch-ROCm ones, stateless (forward(ids)) or stateful
(forward(ids, lengths, state=None)).
"""
import inspect
import warnings

import torch


class RNNTModel(torch.nn.Module):
    def __init__(self, predictor, encoder, joint):
        super().__init__()
        self.predictor = predictor
        self.encoder = encoder
        self.joint = joint
        # optional waveform front end (rnnt_amd.TFJSSpectrogram, ...): GreedyStream.push_audio / BeamStream.push_audio featurize with it;
        # forward, greedy_decode and beam_search take mel features and never look at it
        self.featurizer = None
        # torchaudio's host-side length checks (max(lengths) == T / U: they synchronise).  False skips
        # them — the kernels clamp every length into range — so that forward + backward enqueue
        # device work only and can be captured into a HIP graph.
        self.check_lengths = True
        # latency regularisers of the loss (rnnt_amd.joint_rnnt_loss's options of the same names): FastEmit's
        # lambda and the delay penalty's delta, both >= 0; 0 = the reference's plain loss
        self.fastemit_lambda = 0.0
        self.delay_penalty = 0.0
        # alignment-restricted loss: called as model(..., blank_idx, restrict_frames=frames), label u is emitted only
        # at encoder frames frames[n,u] - restrict_left .. frames[n,u] + restrict_right; ints >= 0
        self.restrict_left = 0
        self.restrict_right = 0
        self._restrict_frames = None  # the frames of the call in progress (__call__)
        # CTC auxiliary head: with a rnnt_amd.CTCHead as `ctc_head` and 0 < ctc_weight <= 1, `forward` returns
        # (1 - ctc_weight) * rnnt + ctc_weight * ctc from the one encoder output (CTC blank = blank_idx, the mean of the per-utterance
        # costs on both sides); None or 0: the transducer loss alone, exactly as without the attributes
        self.ctc_head = None
        self.ctc_weight = 0.0
        # the path the last greedy_decode / greedy_decode_many took: "persistent", "loop", "lstm_loop" (DESIGN.md §4p "Device decode")
        # or "host"; greedy_decode_many: "host" only if every utterance took the host loop
        self.last_decode_path = None
        # the path the last beam_search / beam_search_many took: "device" (ConvPredictor), "lstm_device" (LSTMPredictor,
        # §4h "LSTM") or "host"; beam_search_many: "host" only if every utterance took the host loop
        self.last_beam_path = None

    @property
    def device(self):
        return next(self.parameters()).device

    def __call__(self, *args, restrict_frames=None, **kwargs):
        """model(mel, mel_lens, ids, id_lens, blank_idx, restrict_frames=None): the reference's five arguments, and the optional
        reference alignment of the alignment-restricted loss (int32 [N,U] on the device, e.g. a teacher's `align(...)[1]`;
        DESIGN.md §4n).  `forward` keeps the reference's signature, which callers introspect and wrappers such as DDP pass
        through; the frames travel beside it for the duration of the call."""
        self._restrict_frames = restrict_frames
        try:
            return super().__call__(*args, **kwargs)
        finally:
            self._restrict_frames = None

    def forward(self, mel_features: torch.Tensor, mel_feature_lens: torch.Tensor,
                input_ids: torch.Tensor, input_id_lens: torch.Tensor,
                blank_idx: int) -> torch.Tensor:
        # predictor sees the targets with a leading blank (reference model.py:20-21); the loss
        # sees the un-prepended ids (model.py:36)
        start = torch.full((input_ids.shape[0], 1), blank_idx, dtype=input_ids.dtype,
                           device=self.device)
        decoder_features = self._predict(torch.cat([start, input_ids], dim=1), input_id_lens + 1)

        audio_features = self.encoder(mel_features).permute(0, 2, 1)  # (N,C,L) -> (N,L,C) view
        audio_feature_lens = self.encoder.calc_output_lens(mel_feature_lens)

        # reference model.py:32-41 — blank=-1, clamp=-1, reduction="mean" — as one engine call
        reg = {}
        if self.fastemit_lambda:
            reg["fastemit_lambda"] = self.fastemit_lambda
        if self.delay_penalty:
            reg["delay_penalty"] = self.delay_penalty
        if self._restrict_frames is not None:
            reg.update(restrict_frames=self._restrict_frames, restrict_left=self.restrict_left, restrict_right=self.restrict_right)
        loss = self.joint.fused_loss(audio_features, decoder_features,
                                     targets=input_ids.int(),
                                     logit_lengths=audio_feature_lens.int(),
                                     target_lengths=input_id_lens.int(),
                                     blank=-1, reduction="mean", check_lengths=self.check_lengths, **reg)
        w = float(self.ctc_weight)
        if self.ctc_head is None or w == 0.0:
            return loss
        # hybrid CTC / RNN-T: the CTC branch reads the same encoder output
        ctc = self.ctc_head.loss(audio_features, input_ids.int(), audio_feature_lens.int(), input_id_lens.int(),
                                 blank=blank_idx, reduction="mean", check_lengths=self.check_lengths)
        return (1.0 - w) * loss + w * ctc

    @torch.no_grad()
    def ctc_greedy_decode(self, mel_features: torch.Tensor, mel_feature_lens: torch.Tensor):
        """The CTC head's greedy decode of a whole batch: argmax per encoder frame, repeats and blanks dropped —
        no predictor, no per-token loop, one host synchronisation for the batch.  Returns a list of token lists; the blank is
        the joint's blank_idx."""
        if self.ctc_head is None:
            raise RuntimeError("ctc_greedy_decode needs a ctc_head (rnnt_amd.CTCHead)")
        audio_features = self.encoder(mel_features).permute(0, 2, 1)
        audio_feature_lens = self.encoder.calc_output_lens(mel_feature_lens)
        return self.ctc_head.greedy_decode(audio_features, audio_feature_lens.int(), blank=self.joint.blank_idx)

    def _predict(self, ids_with_start, lens_with_start):
        """The predictor's features for `forward` and `align`: a stateless predictor is called as predictor(ids); a stateful one
        (the LSTM's forward(input, lengths, state=None) -> (features, lengths, state)) with the lengths, from zero state."""
        if self._predictor_is_stateful():
            return self.predictor(ids_with_start, lens_with_start)[0]
        return self.predictor(ids_with_start)

    # ---- forced alignment
    @torch.no_grad()
    def align(self, mel_features: torch.Tensor, mel_feature_lens: torch.Tensor, input_ids: torch.Tensor,
              input_id_lens: torch.Tensor, blank_idx: int):
        """The best alignment of each transcript against its audio, inputs prepared exactly as `forward` prepares them.
        Returns (scores [N] float32: the best path's log-probability, frames [N,U] int32: the ENCODER frame at which each
        label is emitted, -1 past input_id_lens[n]).  Seconds: frame * the encoder's stride (calc_output_lens) * the
        featurizer's hop."""
        start = torch.full((input_ids.shape[0], 1), blank_idx, dtype=input_ids.dtype, device=self.device)
        decoder_features = self._predict(torch.cat([start, input_ids], dim=1), input_id_lens + 1)
        audio_features = self.encoder(mel_features).permute(0, 2, 1)
        audio_feature_lens = self.encoder.calc_output_lens(mel_feature_lens)
        return self.joint.align(audio_features, decoder_features, targets=input_ids.int(),
                                logit_lengths=audio_feature_lens.int(), target_lengths=input_id_lens.int(),
                                blank=-1, check_lengths=self.check_lengths)

    # ---- greedy decode (reference model.py:45-139); host loop, not on the engine's path
    def _predictor_is_stateful(self) -> bool:
        # forward(ids, lengths[, state]) (the reference's LSTMPredictor) against forward(ids) (its ConvPredictor); optional
        # extras with defaults — rnnt_amd.ConvPredictor's keep_masks test aid — do not make a predictor stateful
        params = inspect.signature(self.predictor.forward).parameters.values()
        required = [q for q in params if q.default is inspect.Parameter.empty
                    and q.kind in (inspect.Parameter.POSITIONAL_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD)]
        return len(required) >= 2

    def _predictor_is_lstm(self) -> bool:
        """The predictor is the engine's own LSTMPredictor (any backend, any dtype): the one stateful predictor the beam searches take."""
        from .lstm_predictor import LSTMPredictor
        return isinstance(self.predictor, LSTMPredictor)

    def _device_loop_ok(self, audio) -> bool:
        """The whole decode loop can run on the device: the engine's stateless ConvPredictor (rnnt_engine_greedy_decode) or its
        LSTMPredictor (rnnt_engine_greedy_decode_lstm; backend not "torch") in eval mode or at p = 0, fp32 HIP tensors, sizes the
        decode kernels cover."""
        from .predictor import ConvPredictor
        from .lstm_predictor import LSTMPredictor
        p = self.predictor
        if not (isinstance(p, (ConvPredictor, LSTMPredictor)) and audio.is_cuda and audio.dtype == torch.float32):
            return False
        if p.training and float(p.dropout.p) > 0.0:
            return False
        E, O = p.embedding.embedding_dim, p.linear.out_features
        H, V = self.joint.joint_ln.in_features, self.joint.joint_ln.out_features
        has_text = hasattr(self.joint, "text_ln")
        if isinstance(p, LSTMPredictor):
            if p.backend == "torch" or p._engine_refusal(audio, None) is not None or self.joint.joint_ln.weight.dtype != torch.float32:
                return False
            from . import engine
            return (has_text or O == H) and engine.greedy_decode_lstm_supported(1, *p._decode_sizes(), H, V, has_text)
        if E % 4 or O % 4 or E > 1024 or O > 1024 or H % 8 or V % 4:
            return False
        return has_text or O == H

    def _lstm_loop(self, frames_list, max_length, scan_frames):
        """The token lists of up to 32 utterances' frames ([T_u, H] each) decoded in lockstep by engine.greedy_decode_lstm with the
        model's live parameters; one host synchronisation."""
        from . import engine
        joint = self.joint
        tl = getattr(joint, "text_ln", None)
        out = engine.greedy_decode_lstm(frames_list, self.predictor._decode_bundle(), tl.weight if tl is not None else None,
                                        tl.bias if tl is not None else None, joint.joint_ln.weight, joint.joint_ln.bias, joint.blank_idx,
                                        max_length, max_per_frame=10,
                                        scan_frames=max(1, min(int(scan_frames) if scan_frames > 0 else 32, 128)))
        self.predictor.last_backend = "engine"
        self.last_decode_path = "lstm_loop"
        state, toks = out[:2]
        host = torch.cat((state, toks), dim=1).tolist()  # the batch's one synchronisation: [N][8 state words | tokens]
        return [row[engine.DECODE_LABELS:engine.DECODE_LABELS + row[engine.DECODE_NTOK]] for row in host]

    def _decode_tables(self):
        """The persistent decode's model tables (engine.greedy_decode_tables: conv2's pack, conv1 as tap tables, the folded text_ln) built
        from the parameters AS THEY ARE NOW, on the current stream.  Nothing is cached on the module: the engine's own optimizer
        (rnnt_amd.optim.AdamW) and replays of a captured training step update parameters through raw pointers, which no version counter
        sees, so a cache keyed on tensor identity went stale between the reference flow's evaluations (rnnt/train.py:165-201).  A build is
        ~0.13 ms; greedy_decode_many shares one build between all utterances of a call, greedy_decode lets the launch rebuild in place."""
        from . import engine
        return engine.greedy_decode_tables(*self._decode_bundle()[:4], self.joint.joint_ln.in_features)

    # ---- what the engine's decode entries are told about the model: greedy, beam and both kinds of stream share these
    def _decode_sizes(self):
        """(S, E, O, H, V, has_text), as the engine's *_supported queries take them."""
        p, joint = self.predictor, self.joint
        S, E = p.embedding.weight.shape
        return (S, E, p.linear.out_features, joint.joint_ln.in_features, joint.joint_ln.out_features, hasattr(joint, "text_ln"))

    def _decode_bundle(self):
        """The arguments every engine decode entry takes after the frames: the predictor's parameters, its two LayerNorm eps,
        joint.text_ln's weight and bias (or None, None), joint_ln's weight and bias, the blank."""
        p, joint = self.predictor, self.joint
        tl = getattr(joint, "text_ln", None)
        return (p._params(), (float(p.input_layer_norm.eps), float(p.output_layer_norm.eps)),
                tl.weight if tl is not None else None, tl.bias if tl is not None else None,
                joint.joint_ln.weight, joint.joint_ln.bias, joint.blank_idx)

    def _decode_frames(self, audio):
        """Encoder output (1, n, C), permuted as rnnt/model.py:93 -> the [n, H] fp32 frames the decode entries read: audio_ln applied
        (per frame: the same numbers chunk by chunk), contiguous.  audio_ln runs on the engine's fp32 GEMM (rnnt_engine_linear_fwd: one kernel,
        a row's sum does not depend on how many rows the call has).  torch.nn.Linear's library GEMM picks its kernel by the row count: at
        the reference's widths a stream's chunks and the whole utterance then differed in the last bits, and with them the scores of
        beam_stream and beam_search (1.5e-5 at -175.8 on decode_ref_widths_proj pushed frame by frame) that are promised equal."""
        frames, joint = audio[0], self.joint
        if hasattr(joint, "audio_ln"):
            ln = joint.audio_ln
            if (frames.is_cuda and frames.shape[0] > 0 and frames.dtype == ln.weight.dtype == torch.float32 and ln.bias is not None
                    and ln.in_features % 4 == 0 and ln.out_features % 4 == 0):
                from . import engine
                frames = engine.linear_fwd(frames, ln.weight, ln.bias, backend="fp32")
            else:
                frames = ln(frames)
        return frames.float().contiguous()

    @staticmethod
    def _nbest(st, toks, sc):
        """One search's n-best list from its state words, token rows and scores (engine.beam_decode's layout), best first."""
        return [(toks[j][1:1 + st[8 + j]], sc[j]) for j in range(st[2])]

    @torch.no_grad()
    def greedy_decode(self, mel_features: torch.Tensor, mel_feature_lens: torch.Tensor,
                      max_length: int = 200, scan_frames: int = 32, device_loop=None, persistent=None):
        """Greedy decode with the reference's control flow (rnnt/model.py:95-125): emit the argmax
        token until blank or 10 symbols per frame, then advance.  The joint + argmax of up to
        `scan_frames` consecutive frames run on the engine per call (JointNetwork.greedy_scan), so
        the host syncs once per emitted token / all-blank block instead of once per frame;
        scan_frames=0 keeps the per-frame single_forward loop."""
        assert mel_features.shape[0] == 1, "Greedy decoding only works with a batch size of 1"
        if max_length < 2:  # the reference's loop (rnnt/model.py:108) never runs: tokens = [blank] already has max_length entries
            return []
        stateful = self._predictor_is_stateful()
        audio = self.encoder(mel_features).permute(0, 2, 1)
        # device_loop (None: when possible): the WHOLE loop on the device — scan, argmax, the loop's bookkeeping and the
        # predictor's step per token (ConvPredictor or LSTMPredictor) as one fixed kernel sequence per iteration — and ONE host
        # synchronisation per utterance (the scan path below still synchronises once per emitted token).  An LSTM model takes
        # it by default because it beat the host loop at both timed lengths (2.5x at T = 1000, 2.2x at T = 100;
        # profiles/lstm_decode_bench.txt).
        if device_loop is None:
            device_loop = scan_frames > 0 and self._device_loop_ok(audio)
        if device_loop:
            from . import engine
            if not self._device_loop_ok(audio):
                raise RuntimeError("greedy_decode(device_loop=True) needs the engine's ConvPredictor or LSTMPredictor in eval mode on a HIP device")
            frames = self._decode_frames(audio)
            if stateful:
                if persistent:
                    raise RuntimeError("greedy_decode(persistent=True): there is no persistent decode kernel for the LSTMPredictor")
                return self._lstm_loop([frames], max_length, scan_frames)[0]
            args = (frames, *self._decode_bundle(), max_length)
            if persistent is None:  # one persistent launch per utterance where the engine takes the sizes
                persistent = engine.greedy_decode_persistent_supported(frames.shape[0], *self._decode_sizes())
            if persistent:
                state, toks = engine.greedy_decode_persistent(*args, max_per_frame=10)  # tables rebuilt inside the call, from the live weights
            else:
                state, toks = engine.greedy_decode_loop(*args, max_per_frame=10,
                                                        scan_frames=max(1, min(int(scan_frames) if scan_frames > 0 else 64, 128)))
            both = getattr(state, "_with_tokens", None)  # (the persistent launch: state and tokens in one buffer, one copy)
            host = both.tolist() if both is not None else None  # the utterance's one synchronisation
            st = host[:engine.DECODE_STATE_WORDS] if host is not None else state.tolist()
            code = st[engine.DECODE_CODE]
            if persistent and code != 0:
                # code < 10: the persistent loop gave up waiting for a hand-off (its workgroups were not all resident: a device shared
                # with another process or stream's long kernels).  code >= 10 (engine.DECODE_RANGE_CODES): an audio frame or a text
                # vector beyond +-30, where the loop's factored tanh is not exact.  Either way nothing it wrote is a decode — run the
                # kernel-per-layer loop, which needs no residency and takes tanh of the sum
                if code not in engine.DECODE_RANGE_CODES:
                    warnings.warn(f"rnnt_amd: the persistent greedy decode gave up at hand-off {code} (iteration {st[engine.DECODE_ITERATIONS]}); "
                                  "falling back to the kernel-per-layer loop", RuntimeWarning)
                state, toks = engine.greedy_decode_loop(*args, max_per_frame=10,
                                                        scan_frames=max(1, min(int(scan_frames) if scan_frames > 0 else 64, 128)))
                st, host = state.tolist(), None
            engine.check_decode_state(st)
            self.last_decode_path = "persistent" if host is not None else "loop"
            ntok = st[engine.DECODE_NTOK]
            return host[engine.DECODE_LABELS:engine.DECODE_LABELS + ntok] if host is not None else toks[1:1 + ntok].tolist()
        self.last_decode_path = "host"
        from .stream import HostGreedyLoop  # (one host loop, resumable: GreedyStream's host path runs it too)
        loop = HostGreedyLoop(self, max_length, max_symbols_per_frame=10, scan_frames=scan_frames)
        loop.run(audio)
        return loop.tokens[1:]

    def greedy_stream(self, max_length=None, max_symbols_per_frame=10, persistent=None, device_loop=None):
        """A GreedyStream (rnnt_amd/stream.py): greedy decoding push by push — `push(mel_chunk)` through the encoder's
        streaming_forward, or `push_encoded(audio_features)` — whose labels, concatenated, equal greedy_decode of all frames at once with
        the same max_length (None: unbounded).  The device paths and their choice follow greedy_decode; `persistent` forces one.
        `device_loop=None` keeps the choice every model had before LSTM streams could rest on the device: a ConvPredictor model takes its
        device paths, an LSTMPredictor model the HOST loop.  `device_loop=True` makes an LSTMPredictor stream a device group of one
        (greedy_streams; DESIGN.md §4p "Device stream") and raises where no device path applies; `device_loop=False` forces the host loop.
        Making the device the default of an LSTM stream is left to a follow-up."""
        from .stream import GreedyStream
        return GreedyStream(self, max_length=max_length, max_symbols_per_frame=max_symbols_per_frame, persistent=persistent,
                            device_loop=device_loop)

    def greedy_streams(self, n: int, max_length=None, max_symbols_per_frame=10, scan_frames=32, device_loop=None):
        """A GreedyStreamGroup (rnnt_amd/stream.py; DESIGN.md §4p "Device stream"): `n` (1 .. 32) independent greedy streams of this model
        — `push_encoded([chunk or None] * n)` returns each stream's new labels, `tokens[i]` equals greedy_decode of the frames stream i has
        been pushed so far, `reset(i)` starts a new utterance in slot i.  With an LSTMPredictor model the device decode loop takes, the
        streams rest on the device and a push advances all of them in lockstep with one host synchronisation (`device_loop`: None = where
        it applies and n >= 4, the sizes at which it beat n host loops at every timed shape, profiles/lstm_stream_bench.txt; True = or
        raise; False = n host loops); every other model runs n host loops."""
        from .stream import GreedyStreamGroup
        return GreedyStreamGroup(self, n, max_length=max_length, max_symbols_per_frame=max_symbols_per_frame, scan_frames=scan_frames,
                                 device_loop=device_loop)

    # greedy_decode_many's default batch with an LSTMPredictor: of 4, 8, 16 and 32 the only one within 10 % of the best time per utterance
    # at both timed lengths (2.0 ms at T = 1000, 0.56 ms at T = 100; profiles/lstm_decode_bench.txt)
    LSTM_DECODE_BATCH = 32

    @torch.no_grad()
    def greedy_decode_many(self, mels, max_length: int = 200, concurrency=None, batch=None):
        """Greedy decode of SEVERAL utterances (a list of (1, C, L) mel tensors): `greedy_decode` of each, but with up to `concurrency`
        utterances in flight on streams of their own — the persistent decode of one utterance keeps 16-128 of the device's compute units
        (rnnt_engine_greedy_decode_persistent: one workgroup per 16 vocabulary entries), so a 256-CU device runs four 1024-entry decodes
        side by side.  Nothing synchronises until every utterance is enqueued.  The reference decodes utterance by utterance
        (rnnt/model.py:131-139 called from train.py:170-201); this is that loop, returning the same token lists in the same order.
        `concurrency` defaults to as many decodes as are guaranteed to be resident together (compute units // workgroups per decode, at most
        8); more would risk none of them being complete on the device (each waits for all of its workgroups).
        With an rnnt_amd.LSTMPredictor the utterances the device loop takes (`_device_loop_ok`) advance `batch` (1 .. 32, default
        LSTM_DECODE_BATCH) at a time through ONE loop (rnnt_engine_greedy_decode_lstm: the utterances are the rows of every product's
        tile), one host synchronisation per batch; any other utterance, and every other stateful predictor, takes the host loop.
        `concurrency` is not used then.  Entry i of the result is greedy_decode(mels[i]) either way."""
        from . import engine
        if not mels:
            return []
        assert all(m.shape[0] == 1 for m in mels), "one utterance per entry"
        lens = [torch.tensor([m.shape[-1]], device=m.device) for m in mels]
        dev = mels[0].device
        if self._predictor_is_stateful():
            batch = self.LSTM_DECODE_BATCH if batch is None else int(batch)
            if not 1 <= batch <= engine.LSTM_DECODE_MAX:
                raise ValueError(f"greedy_decode_many: batch={batch} outside [1, {engine.LSTM_DECODE_MAX}]")
            out, path = [None] * len(mels), "host"
            audios = [self.encoder(m).permute(0, 2, 1) for m in mels]
            looped = [i for i, a in enumerate(audios) if max_length >= 2 and self._device_loop_ok(a)]
            for i in range(len(mels)):
                if i not in looped:
                    out[i] = self.greedy_decode(mels[i], lens[i], max_length=max_length, device_loop=False)
            for k in range(0, len(looped), batch):
                group = looped[k:k + batch]
                for i, toks in zip(group, self._lstm_loop([self._decode_frames(audios[i]) for i in group], max_length, 32)):
                    out[i] = toks
                path = "lstm_loop"
            self.last_decode_path = path
            return out
        ok = (max_length >= 2 and dev.type == "cuda" and not self._predictor_is_stateful()
              and self._device_loop_ok(torch.zeros(1, 1, device=dev)))
        if ok:
            ok = engine.greedy_decode_persistent_supported(8, *self._decode_sizes())
        if not ok:
            return [self.greedy_decode(m, l, max_length=max_length) for m, l in zip(mels, lens)]
        groups = min(max((self.joint.joint_ln.out_features + 15) // 16, 16), 128)
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        n_par = max(1, min(int(concurrency) if concurrency else 8, cus // groups, len(mels)))
        cur = torch.cuda.current_stream(dev)
        tables = self._decode_tables()  # one build per call, on `cur`; every side stream waits for `cur` before its first launch
        streams = [torch.cuda.Stream(device=dev) for _ in range(n_par)]
        pending = []
        for i, mel in enumerate(mels):
            st = streams[i % n_par]
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                frames = self._decode_frames(self.encoder(mel).permute(0, 2, 1))
                state, toks = engine.greedy_decode_persistent(frames, *self._decode_bundle(), max_length, max_per_frame=10, tables=tables)
            pending.append((state, mel))
        for st in streams:
            st.synchronize()
        out = []
        for (state, mel), l in zip(pending, lens):
            host = state._with_tokens.tolist()
            if host[engine.DECODE_CODE] != 0:  # this decode gave up waiting for a hand-off, or met an activation beyond +-30 (see greedy_decode): once more, alone
                out.append(self.greedy_decode(mel, l, max_length=max_length))
            else:
                out.append(host[engine.DECODE_LABELS:engine.DECODE_LABELS + host[engine.DECODE_NTOK]])
        self.last_decode_path = "persistent"
        return out

    # ---- beam search: frame-synchronous, <= max_symbols_per_frame labels per frame, hypotheses merged by sequence
    @torch.no_grad()
    def beam_search(self, mel_features: torch.Tensor, mel_feature_lens: torch.Tensor, beam_size: int = 4, max_length: int = 200,
                    max_symbols_per_frame: int = 10, return_nbest: bool = False, context=None, device_search=None):
        """Beam search over the whole encoder output (like greedy_decode, `mel_feature_lens` is not used).  Returns the best
        entry's token list, or with `return_nbest` the final beam as [(tokens, log-probability), ...] best first.  beam_size 1 is
        greedy_decode's result.  The search runs on the device (rnnt_engine_beam_decode: a fixed kernel sequence per round, one
        synchronisation per utterance) where greedy_decode's device loop does — engine ConvPredictor, eval mode, fp32 HIP tensors,
        sizes the kernels cover, beam_size <= 16 — else as a plain-torch host loop of the same search over any stateless
        `predictor(ids)` and `joint.single_forward` (CPU too).  With an rnnt_amd.LSTMPredictor (DESIGN.md §4h "LSTM") the search runs on
        the device under the same conditions and without a `context` (rnnt_engine_beam_decode_lstm: a hypothesis's LSTM state follows it
        as an index into a pool), else as the host loop with one predictor step per new hypothesis from its parent's cached state;
        `device_search` forces either (None: the device where it applies — it beat the host loop at every timed shape, 5.9x - 8.3x,
        profiles/beam_lstm_bench.txt).  Any other stateful predictor raises NotImplementedError.  `last_beam_path` names the path taken.
        `context` (a rnnt_amd.ContextGraph: phrases and a boost per matched token) biases the search towards the caller's phrases
        (DESIGN.md §4h "Context"): on the device where the plain search is (graphs of up to 65536 nodes; the n-best list is finalised
        and re-sorted on the host), else in the host loop.  The scores returned are FINALISED — the bonus of a match still unfinished at
        the end is taken back; banked phrases keep theirs.  With a graph beam_size 1 is no longer the greedy decode.  None, a graph
        without phrases and score 0 give exactly the plain search."""
        assert mel_features.shape[0] == 1, "Beam search only works with a batch size of 1"
        beam_size, max_length, m = int(beam_size), int(max_length), int(max_symbols_per_frame)
        if beam_size < 1 or m < 1:
            raise ValueError(f"beam_search: beam_size={beam_size} and max_symbols_per_frame={m} must be >= 1")
        lstm = self._predictor_is_lstm()
        if self._predictor_is_stateful() and not lstm:
            raise NotImplementedError("beam_search needs a stateless predictor (forward(ids), e.g. ConvPredictor); "
                                      "stateful (LSTM) predictors are not supported")
        g = self._beam_context(context)
        audio = self.encoder(mel_features).permute(0, 2, 1)
        if lstm:
            ok = g is None and self._beam_lstm_ok(audio, beam_size, max_length)
            if device_search and not ok:
                raise RuntimeError("beam_search(device_search=True) needs the engine's LSTMPredictor in eval mode on a HIP device, sizes the "
                                   "kernels cover, beam_size <= 16 and no context")
            if ok and device_search is not False:
                nbest = self._beam_search_lstm([self._decode_frames(audio)], beam_size, max_length, m)[0]
            else:
                nbest = self._beam_search_host(audio, beam_size, max_length, m, g)
        elif self._beam_device_ok(audio, beam_size, max_length, g):
            nbest = self._beam_search_device(audio, beam_size, max_length, m, g)
            self.last_beam_path = "device"
        else:
            nbest = self._beam_search_host(audio, beam_size, max_length, m, g)
        return nbest if return_nbest else list(nbest[0][0])

    def _beam_lstm_ok(self, audio, beam_size, max_length, n_utt=1) -> bool:
        """The LSTM model's beam search can run on the device: where its greedy loop can, beam_size <= 16, sizes the entry takes."""
        if not (1 <= beam_size <= 16 and max_length >= 2 and self._device_loop_ok(audio)):
            return False
        from . import engine
        H, V = self.joint.joint_ln.in_features, self.joint.joint_ln.out_features
        return engine.beam_decode_lstm_supported(n_utt, *self.predictor._decode_sizes(), H, V, hasattr(self.joint, "text_ln"), max_length,
                                                 beam_size)

    def _beam_search_lstm(self, frames_list, beam_size, max_length, m):
        """The n-best lists of up to 32 utterances' frames searched in lockstep by engine.beam_decode_lstm with the model's live
        parameters; one host synchronisation."""
        from . import engine
        joint = self.joint
        tl = getattr(joint, "text_ln", None)
        state, tokens, scores = engine.beam_decode_lstm(
            frames_list, self.predictor._decode_bundle(), tl.weight if tl is not None else None, tl.bias if tl is not None else None,
            joint.joint_ln.weight, joint.joint_ln.bias, joint.blank_idx, max_length, beam_size, max_per_frame=m)
        sts, toks, scs = state.tolist(), tokens.tolist(), scores.tolist()  # the batch's one synchronisation
        for u, st in enumerate(sts):
            if not st[3]:
                raise RuntimeError(f"rnnt_engine: the beam search of utterance {u} did not finish (t={st[0]}, {st[5]} rounds)")
        self.predictor.last_backend = "engine"
        self.last_beam_path = "lstm_device"
        return [self._nbest(st, toks[u], scs[u]) for u, st in enumerate(sts)]

    def _beam_context(self, context):
        """The ContextGraph a search runs with: checked against the vocabulary; None where it cannot change the search (no phrase, score 0)."""
        if context is None:
            return None
        from .context import ContextGraph
        if not isinstance(context, ContextGraph):
            raise TypeError(f"context must be a rnnt_amd.ContextGraph, got {type(context).__name__}")
        context.check(self.joint.joint_ln.out_features, self.joint.blank_idx)
        return context if context.active else None

    def _beam_device_ok(self, audio, beam_size, max_length, context=None) -> bool:
        if not (1 <= beam_size <= 16 and max_length >= 2 and self._device_loop_ok(audio)):
            return False
        from . import engine
        if context is not None and context.n_nodes > engine.BEAM_CONTEXT_MAX_NODES:
            return False
        return engine.beam_decode_supported(*self._decode_sizes(), max_length, beam_size)

    def _beam_search_device(self, audio, beam_size, max_length, m, context=None):
        from . import engine
        frames = self._decode_frames(audio)
        state, tokens, scores = engine.beam_decode(
            frames, *self._decode_bundle(), max_length, beam_size, max_per_frame=m,
            context=context.device_tables(frames.device) if context is not None else None)
        st, toks, sc = state.tolist(), tokens.tolist(), scores.tolist()  # the utterance's one synchronisation
        if not st[3]:
            raise RuntimeError(f"rnnt_engine: the beam search did not finish (t={st[0]}, {st[5]} rounds)")
        nbest = self._nbest(st, toks, sc)
        return context.finalise(nbest) if context is not None else nbest  # (the device's scores are internal)

    BEAM_BATCH = 32  # beam_search_many's default batch: the best of N = 1 .. 32 in profiles/beam_batch_bench.txt, the only one within 10 % of it
    # beam_search_many's default batch with an LSTMPredictor: of 4, 8, 16 and 32 the only one within 10 % of the best time per utterance at
    # both timed lengths and beams (19.0 / 23.3 ms at T = 1000, 2.2 / 3.0 ms at T = 100, beams 4 / 8; profiles/beam_lstm_bench.txt)
    BEAM_LSTM_BATCH = 32

    @torch.no_grad()
    def beam_search_many(self, mels, beam_size: int = 4, max_length: int = 200, max_symbols_per_frame: int = 10,
                         return_nbest: bool = False, batch=None, context=None):
        """Beam search of SEVERAL utterances (a list of (1, C, L) mel tensors, as greedy_decode_many takes): a list in input order whose
        entry i is exactly what `beam_search(mels[i], ...)` returns — the same token lists, the same float64 scores.  Up to `batch`
        utterances (at most 64) advance in lockstep through ONE sequence of rounds on the device (rnnt_engine_beam_decode_batch: the
        round's kernels carry the utterance as a grid dimension, so its launch boundaries are paid once per batch, not once per
        utterance); longer lists run as consecutive batches, the last one possibly partial, with one host synchronisation per batch.
        `batch` defaults to BEAM_BATCH = 32: of N = 1 .. 32 measured at the reference's widths (profiles/beam_batch_bench.txt) the time per
        utterance was still falling at 32 (7 - 21 ms against 106 - 336 ms one by one), so 32 is the smallest N within 10 % of the best.
        Where beam_search would take its host loop (CPU, other stateless predictors, beam_size > 16, sizes the kernels do not cover)
        this is a loop over beam_search.  `context` as beam_search's: ONE ContextGraph biases every utterance
        (rnnt_engine_beam_decode_batch_ctx).
        With an rnnt_amd.LSTMPredictor the utterances beam_search would search on the device advance `batch` (1 .. 32, default
        BEAM_LSTM_BATCH) at a time through rnnt_engine_beam_decode_lstm (DESIGN.md §4h "LSTM"), every other one — all of them with a
        `context` — takes the host loop; any other stateful predictor raises NotImplementedError."""
        beam_size, max_length, m = int(beam_size), int(max_length), int(max_symbols_per_frame)
        if beam_size < 1 or m < 1:
            raise ValueError(f"beam_search_many: beam_size={beam_size} and max_symbols_per_frame={m} must be >= 1")
        lstm = self._predictor_is_lstm()
        if self._predictor_is_stateful() and not lstm:
            raise NotImplementedError("beam_search_many needs a stateless predictor (forward(ids), e.g. ConvPredictor); "
                                      "stateful (LSTM) predictors are not supported")
        mels = list(mels)
        if not mels:
            return []
        assert all(mel.shape[0] == 1 for mel in mels), "one utterance per entry"
        from . import engine
        if lstm:
            batch = self.BEAM_LSTM_BATCH if batch is None else int(batch)
            if not 1 <= batch <= engine.BEAM_LSTM_MAX:
                raise ValueError(f"beam_search_many: batch={batch} outside [1, {engine.BEAM_LSTM_MAX}]")
            g = self._beam_context(context)
            out, path = [None] * len(mels), "host"
            audios = [self.encoder(mel).permute(0, 2, 1) for mel in mels]
            searched = [i for i, a in enumerate(audios) if g is None and self._beam_lstm_ok(a, beam_size, max_length)]
            for i, a in enumerate(audios):
                if i not in searched:
                    out[i] = self._beam_search_host(a, beam_size, max_length, m, g)
            for k in range(0, len(searched), batch):
                group = searched[k:k + batch]
                if not self._beam_lstm_ok(audios[group[0]], beam_size, max_length, len(group)):
                    raise RuntimeError(f"rnnt_engine: the LSTM beam search refuses {len(group)} utterances of sizes the single search takes")
                for i, nbest in zip(group, self._beam_search_lstm([self._decode_frames(audios[i]) for i in group], beam_size, max_length, m)):
                    out[i] = nbest
                path = "lstm_device"
            self.last_beam_path = path
            return out if return_nbest else [list(nbest[0][0]) for nbest in out]
        batch = self.BEAM_BATCH if batch is None else int(batch)
        if not 1 <= batch <= engine.BEAM_BATCH_MAX:
            raise ValueError(f"beam_search_many: batch={batch} outside [1, {engine.BEAM_BATCH_MAX}]")
        g = self._beam_context(context)
        out = [None] * len(mels)
        tables = None
        for i in range(0, len(mels), batch):
            audios = [self.encoder(mel).permute(0, 2, 1) for mel in mels[i:i + batch]]
            # the utterances of the slice that beam_search would decode on the device advance together; any other takes its host loop
            on_device = [self._beam_device_ok(a, beam_size, max_length, g) for a in audios]
            batched = [u for u, ok in enumerate(on_device) if ok]
            if batched and not self._beam_batch_ok(len(batched), beam_size, max_length):
                raise RuntimeError(f"rnnt_engine: the batched beam search refuses {len(batched)} utterances of sizes the single search takes")
            for u, a in enumerate(audios):
                if not on_device[u]:
                    out[i + u] = self._beam_search_host(a, beam_size, max_length, m, g)
            if not batched:
                continue
            if tables is None:
                tables = self._decode_tables()  # one build per call, shared by every batch and utterance
            frames = [self._decode_frames(audios[u]) for u in batched]
            state, tokens, scores = engine.beam_decode_batch(
                frames, *self._decode_bundle(), max_length, beam_size, max_per_frame=m,
                tables=tables, context=g.device_tables(frames[0].device) if g is not None else None)
            sts, toks, scs = state.tolist(), tokens.tolist(), scores.tolist()  # the batch's one synchronisation
            for k, (u, st) in enumerate(zip(batched, sts)):
                if not st[3]:
                    raise RuntimeError(f"rnnt_engine: the beam search of utterance {i + u} did not finish (t={st[0]}, {st[5]} rounds)")
                nbest = self._nbest(st, toks[k], scs[k])
                out[i + u] = g.finalise(nbest) if g is not None else nbest
            self.last_beam_path = "device"
        return out if return_nbest else [list(nbest[0][0]) for nbest in out]

    def beam_stream(self, beam_size: int = 4, max_length: int = 200, max_symbols_per_frame: int = 10, context=None):
        """A BeamStream (rnnt_amd/stream.py): beam search push by push — `push(mel_chunk)` through the encoder's
        streaming_forward, or `push_encoded(audio_features)` — whose n-best list after frames 0 .. k-1, however they were chunked, is
        `beam_search` of those k frames (`nbest`, `tokens`), with the `stable` prefix no later push can change.  On the device where
        beam_search is (the search's state rests in a block the stream owns), else a resumable host loop.  With a `context`
        (ContextGraph, as beam_search's) the stream runs the resumable host loop — the device stream with a context graph is not built
        yet; `nbest`, `tokens` and `stable` are finalised views of the carried internal beam, so any chunking still equals
        `beam_search(..., context=context)` of the same frames.  An rnnt_amd.LSTMPredictor model runs the resumable host loop too (a
        device stream with LSTM state is out of scope, DESIGN.md §4h "LSTM"); any other stateful predictor raises NotImplementedError."""
        from .stream import BeamStream
        return BeamStream(self, beam_size=beam_size, max_length=max_length, max_symbols_per_frame=max_symbols_per_frame,
                          context=self._beam_context(context))

    def beam_streams(self, n: int, beam_size: int = 4, max_length: int = 200, max_symbols_per_frame: int = 10, context=None):
        """A BeamStreamGroup of `n` (1 .. 64) independent beam streams sharing one block and ONE launch sequence per push
        (`push_encoded(chunks)`, a list of n chunks or None); stream i's results are exactly a lone beam_stream's.  `context` as
        beam_stream's: one graph for every stream, on the host loop."""
        from .stream import BeamStreamGroup
        return BeamStreamGroup(self, n, beam_size=beam_size, max_length=max_length, max_symbols_per_frame=max_symbols_per_frame,
                               context=self._beam_context(context))

    def _beam_batch_ok(self, n_utt, beam_size, max_length) -> bool:
        from . import engine
        return engine.beam_decode_batch_supported(*self._decode_sizes(), max_length, beam_size, n_utt)

    def _beam_search_host(self, audio, beam_size, max_length, m, context=None):
        """The search of DESIGN.md §4h as a host loop: the predictor on the whole history of each new hypothesis (cached by
        sequence; an LSTMPredictor: one step from the parent's cached state), single_forward batched over the round's active
        hypotheses, scores as Python floats (double)."""
        from .stream import HostBeamLoop  # (one host loop, resumable frame by frame: BeamStream's host path runs it too)
        loop = HostBeamLoop(self, beam_size, max_length, m, context)
        loop.run(audio)
        self.last_beam_path = "host"
        return loop.nbest
