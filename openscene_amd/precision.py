"""The arithmetic of the convolutions: "bf16x6" (default), "bf16x3" or "bf16x1" -- one knob for INFERENCE passes, a second,
independent one for TRAINING passes.

Every convolution splits its fp32 operands into bf16 pieces and multiplies them on the bf16 matrix units (csrc/split.h):

    name     pieces   products h_i(a) h_j(b) kept          error per output element, in units of sum |a||b|
    bf16x6   3        31 22 13 21 12 11                     2e-6                 (fp32-class; what training needs)
    bf16x3   2        21 12 11                              2^-15 + 2e-6
    bf16x1   1        11  (plain bf16 operands)             2^-7  + 2e-6

The reference rounds the network's output to fp16 (2^-11) before anything reads it (run/evaluate.py:290-292), so an inference pass
can trade the last bits for time.  The mode applies to a forward pass in evaluation mode that records no autograd graph -- through the
network executor and through the module-by-module path alike, bitwise the same either way -- on the tile-list, register-gather,
weight-stationary and 1x1 kernels.  It is IGNORED in training mode and whenever a backward pass can follow (those passes have the
training knob below, bf16x6 by default); the 3-channel stem and the first-generation kernel are always exact.

    with openscene_amd.conv_precision("bf16x3"):
        feats = model(x)                       # model.eval(), under torch.no_grad()
    openscene_amd.set_conv_precision("bf16x1")  # process-wide default; OSN_INFER_PRECISION sets the initial one

TRAINING has its own knob, `train_precision` / `set_train_precision` / OSN_TRAIN_PRECISION, with the same names.  It applies to every
pass `conv_precision` does not: training mode, or a pass that records an autograd graph -- forward launches, their input-gradient
launches (the same kernels on the input-gradient weight image) and the pair-array weight gradient (csrc/wgrad_tl.hip, where both the
gathered activations and the gathered output gradients are split).  The backward of a forward pass runs in the mode the FORWARD ran in,
wherever backward() is called.  Always exact, as in inference: the stem (forward and weight gradient) and the first-generation kernels,
which include the 96 -> 768 head's weight gradient; batch norm, loss and optimizer are fp32, and so are parameters, gradients and the
weight gradient's partial sums.  bf16 pieces keep fp32's exponent range: no loss scaling.  bf16x3 (2^-15 per element) is far tighter
than the mixed precision networks are usually trained in, bf16x1 (2^-7) is of that class; convergence on real data was not measured.

    with openscene_amd.train_precision("bf16x3"):
        loss = criterion(model(x), target)     # model.train()
    loss.backward()                            # in bf16x3: the forward's mode

The two knobs do not see each other: a training pass ignores `conv_precision`, an evaluation-mode pass under no_grad ignores
`train_precision`.
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


# ---- the training knob: the same machinery, a default, an environment variable and a context stack of its own
TRAIN_ENV = "OSN_TRAIN_PRECISION"


def _initial_train(environ):
    """The process default of the training mode a given environment asks for."""
    return _check(environ.get(TRAIN_ENV) or "bf16x6")


_train_default = _initial_train(os.environ)


def set_train_precision(name):
    """Set the process-wide default training mode; -> the previous default.  A `train_precision` context of the calling thread still wins."""
    global _train_default
    prev, _train_default = _train_default, _check(name)
    return prev


def get_train_precision():
    """The training mode in force for the calling thread: its innermost `train_precision` context, else the process default."""
    stack = getattr(_tls, "train_stack", None)
    return stack[-1] if stack else _train_default


class train_precision:
    """Context manager: the mode of the training passes (forward and the backward that belongs to it) the calling thread STARTS inside
    it.  Nests; the mode outside is back in force on exit, also when the body raises.  The name is checked when the object is made."""

    def __init__(self, name):
        self.name = _check(name)

    def __enter__(self):
        if getattr(_tls, "train_stack", None) is None:
            _tls.train_stack = []
        _tls.train_stack.append(self.name)
        return self

    def __exit__(self, *exc):
        _tls.train_stack.pop()
        return False


def pass_pieces(training, grad):
    """Operand pieces (3, 2, 1) of a forward pass and of its backward pass: the inference mode when the pass runs in evaluation mode and
    records no graph, else the training mode."""
    return MODES[get_train_precision()] if (training or grad) else MODES[get_conv_precision()]


def inference_pieces(training, grad):
    """Operand pieces (3, 2, 1) of a forward pass: the mode in force when the pass runs in evaluation mode (`training` false) and
    records no graph (`grad` false), else 3."""
    return 3 if (training or grad) else MODES[get_conv_precision()]
