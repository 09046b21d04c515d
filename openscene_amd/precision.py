"""The arithmetic of the convolutions of an INFERENCE pass: "bf16x6" (default), "bf16x3" or "bf16x1".

Every convolution splits its fp32 operands into bf16 pieces and multiplies them on the bf16 matrix units (csrc/split.h):

    name     pieces   products h_i(a) h_j(b) kept          error per output element, in units of sum |a||b|
    bf16x6   3        31 22 13 21 12 11                     2e-6                 (fp32-class; what training needs)
    bf16x3   2        21 12 11                              2^-15 + 2e-6
    bf16x1   1        11  (plain bf16 operands)             2^-7  + 2e-6

The reference rounds the network's output to fp16 (2^-11) before anything reads it (run/evaluate.py:290-292), so an inference pass
can trade the last bits for time.  The mode applies to a forward pass in evaluation mode that records no autograd graph -- through the
network executor and through the module-by-module path alike, bitwise the same either way -- on the tile-list, register-gather,
weight-stationary and 1x1 kernels.  It is IGNORED (the pass stays bf16x6) in training mode and whenever a backward pass can follow;
the 3-channel stem and the first-generation kernel are always exact.

    with openscene_amd.conv_precision("bf16x3"):
        feats = model(x)                       # model.eval(), under torch.no_grad()
    openscene_amd.set_conv_precision("bf16x1")  # process-wide default; OSN_INFER_PRECISION sets the initial one
"""
import os
import threading

MODES = {"bf16x6": 3, "bf16x3": 2, "bf16x1": 1}
ENV = "OSN_INFER_PRECISION"


def _check(name):
    if name not in MODES:
        raise ValueError("unknown convolution precision %r (one of %s)" % (name, ", ".join(MODES)))
    return name


def _initial(environ):
    """The process default a given environment asks for."""
    return _check(environ.get(ENV) or "bf16x6")


_default = _initial(os.environ)
_tls = threading.local()


def set_conv_precision(name):
    """Set the process-wide default mode; -> the previous default.  A `conv_precision` context of the calling thread still wins."""
    global _default
    prev, _default = _default, _check(name)
    return prev


def get_conv_precision():
    """The mode in force for the calling thread: its innermost `conv_precision` context, else the process default."""
    stack = getattr(_tls, "stack", None)
    return stack[-1] if stack else _default


class conv_precision:
    """Context manager: the mode of the inference passes the calling thread runs inside it.  Nests; the mode outside is back in
    force on exit, also when the body raises.  The name is checked when the object is made."""

    def __init__(self, name):
        self.name = _check(name)

    def __enter__(self):
        if getattr(_tls, "stack", None) is None:
            _tls.stack = []
        _tls.stack.append(self.name)
        return self

    def __exit__(self, *exc):
        _tls.stack.pop()
        return False


def inference_pieces(training, grad):
    """Operand pieces (3, 2, 1) of a forward pass: the mode in force when the pass runs in evaluation mode (`training` false) and
    records no graph (`grad` false), else 3."""
    return 3 if (training or grad) else MODES[get_conv_precision()]
