"""LSTMPredictor with the constructor, attribute names and state-dict keys of the reference
(rnnt/predictor.py:93-186) whose forward, backward and stateful decode step run on the HIP engine
(C ABI rnnt_engine_lstm_predictor_fwd / _bwd).

    predictor:
      _target_: rnnt_amd.LSTMPredictor                 # was rnnt.predictor.LSTMPredictor
      num_symbols: ..., output_dim: 1024, symbol_embedding_dim: 512, num_lstm_layers: 3, lstm_hidden_dim: 512,
      lstm_layer_norm: true, lstm_layer_norm_epsilon: 1e-3, lstm_dropout: 0.3

What the network computes (B rows, U tokens, L layers, hidden width Hd):
  x = input_layer_norm(embedding(ids));  per layer, per token t, with (h, c) starting at the layer's state (zeros without one):
      gates = g_norm(x2g(x_t) + p2g(h))          all 4 Hd gates of a row normalised together; chunks: input, forget, cell, output
      c = c_norm(sigmoid(forget) * c + sigmoid(input) * tanh(cell))     the NORMALISED cell is the one that continues
      h = sigmoid(output) * tanh(c)
  x = dropout(h) after every layer (the state keeps h before dropout);  out = output_layer_norm(linear(x)).
Without layer norm both norms are the identity and x2g has a bias; p2g never has one.  `lengths` is returned as given and masks
nothing: every row runs all U steps.

`backend`: "auto" | "torch" | "engine", as on rnnt_amd.AudioEncoder.  The torch path is this file's plain torch modules (CPU,
float64, autograd: the oracle of the engine path); the engine path needs fp32 HIP tensors and sizes the kernels cover; "engine"
raises with the reason where it does not apply; `last_backend` names the path of the last call.  Dropout masks are drawn with
torch's generator as keep bytes [L][B, U, Hd] on either path.
"""
import ctypes

import torch

from . import engine

MAX_HIDDEN, MAX_EMBED, MAX_LAYERS = 1024, 2048, 8  # rnnt_amd/csrc/lstm.hip


class _LayerParams(ctypes.Structure):  # include/rnnt_engine.h: rnnt_lstm_layer_params
    _fields_ = [(n, ctypes.c_void_p) for n in ("x2g_w", "x2g_b", "p2g_w", "g_norm_w", "g_norm_b", "c_norm_w", "c_norm_b")]


class _Params(ctypes.Structure):  # include/rnnt_engine.h: rnnt_lstm_predictor_params
    _fields_ = [(n, ctypes.c_void_p) for n in ("embedding", "ln_in_w", "ln_in_b", "linear_w", "linear_b", "ln_out_w", "ln_out_b")] + [
        ("layers", ctypes.POINTER(_LayerParams))]


def _per_layer(layer_norm):
    return 6 if layer_norm else 3


def _struct(tensors, L, layer_norm):
    """(struct, the layer array it points to) for the flat parameter order of LSTMPredictor._params()."""
    ptr = [t.data_ptr() for t in tensors]
    n = _per_layer(layer_norm)
    arr = (_LayerParams * L)()
    for l in range(L):
        q = ptr[7 + n * l: 7 + n * (l + 1)]
        if layer_norm:
            arr[l] = _LayerParams(q[0], None, q[1], q[2], q[3], q[4], q[5])
        else:
            arr[l] = _LayerParams(q[0], q[1], q[2], None, None, None, None)
    return _Params(*ptr[:7], ctypes.cast(arr, ctypes.POINTER(_LayerParams))), arr


class _LSTMPredictorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, state_in, keep, p, cfg, *params):
        L, Hd, layer_norm, eps = cfg
        dev = engine._require_cuda(ids, state_in, keep, *params)
        engine._require_dtype(torch.float32, state_in=state_in, **{f"param{i}": t for i, t in enumerate(params)})
        engine._require_dtype(torch.int64, ids=ids)
        engine._require_dtype(torch.uint8, keep=keep)
        engine._require_contiguous(state_in=state_in, keep=keep)
        ids = ids.contiguous()
        params = tuple(t.contiguous() for t in params)
        B, U1 = ids.shape
        S, E = params[0].shape
        O = params[3].shape[0]
        dims = (B, U1, S, E, Hd, O, L, int(layer_norm))
        train = any(ctx.needs_input_grad)  # a call nothing is differentiated through keeps nothing for a backward
        lib = engine.lib()
        with torch.cuda.device(dev):
            n = ctypes.c_size_t(0)
            saved = None
            if train:
                engine._check(lib.rnnt_engine_lstm_predictor_saved_bytes(*dims, ctypes.byref(n)))
                saved = torch.empty(int(n.value), dtype=torch.uint8, device=dev)
            engine._check(lib.rnnt_engine_lstm_predictor_workspace_bytes(*dims, 0, ctypes.byref(n)))
            ws = engine.workspace(dev, int(n.value))
            out = torch.empty((B, U1, O), dtype=torch.float32, device=dev)
            state_out = torch.empty((L, 2, B, Hd), dtype=torch.float32, device=dev)
            st, _arr = _struct(params, L, layer_norm)
            engine._check(lib.rnnt_engine_lstm_predictor_fwd(
                engine._p(ids), *dims, ctypes.byref(st), engine._p(state_in), engine._p(keep), ctypes.c_float(p),
                ctypes.c_float(eps[0]), ctypes.c_float(eps[1]), ctypes.c_float(eps[2]), engine._p(out), engine._p(state_out),
                engine._p(saved), ctypes.c_size_t(saved.numel() if train else 0), engine._p(ws), ctypes.c_size_t(ws.numel()),
                engine._stream(dev)))
        if train:
            ctx.save_for_backward(ids, keep, saved, *params)
        ctx.p, ctx.cfg, ctx.dims = p, cfg, dims
        ctx.mark_non_differentiable(state_out)
        return out, state_out

    @staticmethod
    def backward(ctx, grad_out, _grad_state):
        ids, keep, saved, *params = ctx.saved_tensors
        L, Hd, layer_norm, eps = ctx.cfg
        dev = ids.device
        grad_out = grad_out.contiguous().float()
        lib = engine.lib()
        with torch.cuda.device(dev):
            n = ctypes.c_size_t(0)
            engine._check(lib.rnnt_engine_lstm_predictor_workspace_bytes(*ctx.dims, 1, ctypes.byref(n)))
            ws = engine.workspace(dev, int(n.value))
            grads = [torch.empty_like(t) for t in params]
            sp, _a = _struct(params, L, layer_norm)
            sg, _b = _struct(grads, L, layer_norm)
            engine._check(lib.rnnt_engine_lstm_predictor_bwd(
                engine._p(ids), *ctx.dims, ctypes.byref(sp), engine._p(keep), ctypes.c_float(ctx.p), ctypes.c_float(eps[0]),
                ctypes.c_float(eps[1]), ctypes.c_float(eps[2]), engine._p(grad_out), ctypes.byref(sg), engine._p(saved),
                ctypes.c_size_t(saved.numel()), engine._p(ws), ctypes.c_size_t(ws.numel()), engine._stream(dev)))
        return (None, None, None, None, None, *grads)


class _LSTMLayer(torch.nn.Module):
    """One layer's parameters under the reference's names (x2g, p2g, c_norm, g_norm) and its plain-torch recurrence."""

    def __init__(self, input_dim, hidden_dim, layer_norm=False, layer_norm_epsilon=1e-5):
        super().__init__()
        self.x2g = torch.nn.Linear(input_dim, 4 * hidden_dim, bias=not layer_norm)
        self.p2g = torch.nn.Linear(hidden_dim, 4 * hidden_dim, bias=False)
        self.c_norm = torch.nn.LayerNorm(hidden_dim, eps=layer_norm_epsilon) if layer_norm else torch.nn.Identity()
        self.g_norm = torch.nn.LayerNorm(4 * hidden_dim, eps=layer_norm_epsilon) if layer_norm else torch.nn.Identity()
        self.hidden_dim = hidden_dim

    def forward(self, x, state=None):
        """x [B, U, in] -> (h of every step [B, U, Hd], [h, c] after the last step)."""
        if state is None:
            h = x.new_zeros(x.shape[0], self.hidden_dim)
            c = x.new_zeros(x.shape[0], self.hidden_dim)
        else:
            h, c = state
        from_input = self.x2g(x)
        steps = []
        for t in range(x.shape[1]):
            i, f, g, o = self.g_norm(from_input[:, t] + self.p2g(h)).chunk(4, dim=1)
            c = self.c_norm(torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g))
            h = torch.sigmoid(o) * torch.tanh(c)
            steps.append(h)
        return torch.stack(steps, dim=1), [h, c]


class LSTMPredictor(torch.nn.Module):
    backend = "auto"  # "auto" | "torch" | "engine"

    def __init__(self, num_symbols: int, output_dim: int, symbol_embedding_dim: int, num_lstm_layers: int,
                 lstm_hidden_dim: int, lstm_layer_norm: bool = False, lstm_layer_norm_epsilon: float = 1e-5,
                 lstm_dropout: float = 0.0) -> None:
        super().__init__()
        self.embedding = torch.nn.Embedding(num_symbols, symbol_embedding_dim)
        self.input_layer_norm = torch.nn.LayerNorm(symbol_embedding_dim)
        self.lstm_layers = torch.nn.ModuleList([
            _LSTMLayer(lstm_hidden_dim if l else symbol_embedding_dim, lstm_hidden_dim, layer_norm=lstm_layer_norm,
                       layer_norm_epsilon=lstm_layer_norm_epsilon) for l in range(num_lstm_layers)])
        self.dropout = torch.nn.Dropout(p=lstm_dropout)
        self.linear = torch.nn.Linear(lstm_hidden_dim, output_dim)
        self.output_layer_norm = torch.nn.LayerNorm(output_dim)
        self.lstm_dropout = lstm_dropout
        self.lstm_layer_norm = bool(lstm_layer_norm)
        self.lstm_layer_norm_epsilon = float(lstm_layer_norm_epsilon)
        self.last_backend = None  # "engine" | "torch": the path of the last call

    def _params(self):
        """Flat order of rnnt_lstm_predictor_params: the seven outer tensors, then each layer's."""
        out = [self.embedding.weight, self.input_layer_norm.weight, self.input_layer_norm.bias, self.linear.weight, self.linear.bias,
               self.output_layer_norm.weight, self.output_layer_norm.bias]
        for layer in self.lstm_layers:
            if self.lstm_layer_norm:
                out += [layer.x2g.weight, layer.p2g.weight, layer.g_norm.weight, layer.g_norm.bias, layer.c_norm.weight,
                        layer.c_norm.bias]
            else:
                out += [layer.x2g.weight, layer.x2g.bias, layer.p2g.weight]
        return tuple(out)

    def _decode_sizes(self):
        """(S, E, Hd, O, L, layer_norm), as engine.greedy_decode_lstm_supported takes them."""
        S, E = self.embedding.weight.shape
        return (S, E, self.lstm_layers[0].hidden_dim, self.linear.out_features, len(self.lstm_layers), self.lstm_layer_norm)

    def _decode_bundle(self):
        """What engine.greedy_decode_lstm is told about the predictor: the LIVE parameter tensors (nothing is cached on the module:
        optimizers and replayed graphs write through raw pointers), (L, Hd, layer_norm) and the three eps."""
        return (self._params(), (len(self.lstm_layers), self.lstm_layers[0].hidden_dim, self.lstm_layer_norm),
                (float(self.input_layer_norm.eps), self.lstm_layer_norm_epsilon, float(self.output_layer_norm.eps)))

    def _engine_refusal(self, input, state):
        """Why the engine path does not apply to this call, or None."""
        L, Hd = len(self.lstm_layers), self.lstm_layers[0].hidden_dim
        E, O = self.embedding.embedding_dim, self.linear.out_features
        tensors = list(self._params()) + ([t for pair in state for t in pair] if state is not None else [])
        if not input.is_cuda or any(not t.is_cuda for t in tensors):
            return "tensors that are not on a HIP device"
        if any(t.dtype != torch.float32 for t in tensors):
            return "parameters or state that are not float32"
        if E % 4 or Hd % 4 or O % 4 or Hd > MAX_HIDDEN or E > MAX_EMBED or L > MAX_LAYERS:
            return (f"sizes the kernels do not cover (E % 4, Hd % 4, O % 4 == 0, Hd <= {MAX_HIDDEN}, E <= {MAX_EMBED}, "
                    f"L <= {MAX_LAYERS}; E={E} Hd={Hd} O={O} L={L})")
        if state is not None and torch.is_grad_enabled() and any(t.requires_grad for pair in state for t in pair):
            return "a state that requires grad (the engine has no gradient through the state)"
        return None

    @staticmethod
    def _pack_state(state, B, Hd):
        """The state as ONE [L, 2, B, Hd] tensor: a view (no copy) where the list is the engine's own state_out handed back."""
        L, first = len(state), state[0][0]
        step = B * Hd
        if all(t.shape == (B, Hd) and t.is_contiguous() and t.data_ptr() == first.data_ptr() + 4 * step * (2 * l + k)
               for l, pair in enumerate(state) for k, t in enumerate(pair)):
            try:
                return first.as_strided((L, 2, B, Hd), (2 * step, step, Hd, 1), first.storage_offset())
            except RuntimeError:  # the tensors are neighbours by chance, not one allocation
                pass
        return torch.stack([torch.stack([h, c]) for h, c in state]).contiguous()

    def _keep(self, input, keep_masks):
        """(dropout p of this call, keep bytes [L, B, U, Hd] or None)."""
        p = float(self.dropout.p) if self.training else 0.0
        if p <= 0.0:
            return 0.0, None
        L, Hd = len(self.lstm_layers), self.lstm_layers[0].hidden_dim
        if keep_masks is not None:
            keep = torch.stack([k.to(torch.uint8) for k in keep_masks]) if not torch.is_tensor(keep_masks) else keep_masks.to(torch.uint8)
            return p, keep.to(input.device).contiguous()
        return p, (torch.rand((L, *input.shape, Hd), device=input.device) >= p).to(torch.uint8)

    def forward(self, input, lengths, state=None, keep_masks=None):
        """input [B, U] int64 symbol ids, lengths [B] (returned as given; nothing is masked), state: None or a list of L
        [h, c] pairs of shape (B, Hd) -> (features [B, U, output_dim], lengths, state after the last step).
        `keep_masks` (test aid): explicit keep bytes [L][B, U, Hd] instead of drawing them; ignored in eval mode or at p = 0."""
        if self.backend not in ("auto", "torch", "engine"):
            raise ValueError(f"LSTMPredictor.backend {self.backend!r}: 'auto', 'torch' or 'engine'")
        if state is not None and len(state) != len(self.lstm_layers):
            raise ValueError(f"LSTMPredictor: state has {len(state)} layers, the network {len(self.lstm_layers)}")
        why = None if self.backend == "torch" else self._engine_refusal(input, state)
        if self.backend == "engine" and why is not None:
            raise RuntimeError(f"LSTMPredictor(backend='engine'): the engine path does not apply: {why}")
        p, keep = self._keep(input, keep_masks)
        L, Hd = len(self.lstm_layers), self.lstm_layers[0].hidden_dim
        # "auto": the engine wherever it applies — it was faster at every timed shape (profiles/lstm_predictor_bench.txt), no threshold
        if self.backend == "torch" or why is not None:
            self.last_backend = "torch"
            x = self.input_layer_norm(self.embedding(input))
            state_out = []
            for l, layer in enumerate(self.lstm_layers):
                x, s = layer(x, None if state is None else state[l])
                if keep is not None:
                    x = x * keep[l].to(x.dtype) / (1.0 - p)
                state_out.append(s)
            return self.output_layer_norm(self.linear(x)), lengths, state_out
        self.last_backend = "engine"
        packed = None if state is None else self._pack_state(state, input.shape[0], Hd)
        eps = (float(self.input_layer_norm.eps), self.lstm_layer_norm_epsilon, float(self.output_layer_norm.eps))
        out, st = _LSTMPredictorFn.apply(input, packed, keep, p, (L, Hd, self.lstm_layer_norm, eps), *self._params())
        return out, lengths, [[st[l, 0], st[l, 1]] for l in range(L)]
