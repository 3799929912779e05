"""rnnt_amd — MI355X (gfx950) native RNN-T joint + transducer-loss engine.

Host-side mirror of the jakepoz/rnnt API for this path (rnnt.joint.JointNetwork,
rnnt.model.RNNTModel) over hand-written HIP kernels reached through a C ABI
(include/rnnt_engine.h -> rnnt_amd/csrc/librnnt_engine.so, bound with ctypes).
"""
from . import engine, optim  # noqa: F401
from .functional import joint_rnnt_loss, rnnt_loss, joint_logits, linear, rnnt_align, joint_rnnt_align  # noqa: F401
from .functional import ctc_loss, ctc_greedy_decode  # noqa: F401
from .ctc import CTCHead  # noqa: F401
from .joint import JointNetwork  # noqa: F401
from .predictor import ConvPredictor  # noqa: F401
from .lstm_predictor import LSTMPredictor  # noqa: F401
from .encoder import AudioEncoder, JasperBlock  # noqa: F401
from .featurizer import NormalizedMelSpectrogram, TFJSOldPiecewiseSpectrogram, TFJSSpectrogram  # noqa: F401
from .model import RNNTModel  # noqa: F401
from .stream import BeamStream, BeamStreamGroup, GreedyStream  # noqa: F401
from .context import ContextGraph  # noqa: F401

__all__ = ["engine", "optim", "joint_rnnt_loss", "rnnt_loss", "joint_logits", "rnnt_align", "joint_rnnt_align", "ctc_loss", "ctc_greedy_decode", "CTCHead", "JointNetwork", "RNNTModel", "ConvPredictor", "LSTMPredictor", "AudioEncoder", "JasperBlock", "TFJSSpectrogram", "TFJSOldPiecewiseSpectrogram", "NormalizedMelSpectrogram", "GreedyStream", "BeamStream", "BeamStreamGroup", "ContextGraph"]
