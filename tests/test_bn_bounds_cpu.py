"""What gives tests/test_gpu_bn_bounds.py its teeth, checked without a GPU: on every shape and input kind the GPU module uses (up to
8193 rows here), the numpy emulation of the batch-norm kernels' arithmetic (bn_bounds.emulate) meets every limit of bn_bounds with
a worst ratio <= 0.5, the margin the limits have over correct arithmetic; the same emulation with ONE defect (bn_bounds.MUTANTS)
breaks a limit; and the reference alone leaves at most 5 % of a case's columns out of the backward checks.

The one quantity not held to 0.5 is gres with k > 1 gradient sources: its limit k u sum|g_i| is the rigorous worst case of the fp32
sum ((k - 1) u sum|g_i|) plus one u, not a doubled first-order count, so the emulation may reach (k - 1) / k of it and is held to that.

What the tensor-max check of test_gpu_dense.py (max |err| / max |ref| at 2e-5 / 5e-5 / 1e-5) makes of each mutant, measured on the
"scales" inputs of MUTANT_CASES with a residual, ReLU and three gradient sources:
    a  fp32 column sums                        passes it at (16, 4), (63, 12), (65, 20); breaks var / mean / y / gx here
    b  variance against the fp32 mean          passes it at (16, 4), (63, 12), (65, 20); breaks var / rv / y / gx here
    c  biased running_var                      passes it at (8193, 20);                  breaks rv here
    f  1 / (n - 1) in gx                       passes it from 512 rows on;               breaks gx here
    d  last n % 16 rows dropped, e  last 4 columns with column 0's sums, g  64 rows dropped from the backward sums:
       the tensor-max check catches them at every shape where they act -- y is normalised, so a column with wrong statistics is wrong
       at the tensor's own scale -- but test_gpu_dense.py runs no width with c % 8 == 4 and no row count at a block edge, so (e) in
       the half-filled workgroup and (g) at 65 / 129 row blocks were never looked at.  Here each breaks mean, gbeta or ggamma.
"""
import functools

import numpy as np
import pytest

import bn_bounds as bb

MARGIN = 0.5
MUTANT_CASES = [("scales", 63, 12), ("scales", 65, 20), ("scales", 513, 68), ("scales", 8193, 20), ("offset", 65, 20), ("offset", 4161, 68)]
PASS_THE_TENSOR_MAX_CHECK = ("a", "b", "c", "f")      # on at least one "scales" case of MUTANT_CASES, while breaking a limit there
CASES = [(k, n, c) for k in bb.GPU_KINDS for (n, c) in bb.CPU_SHAPES]


def _runs(cs):
    """(label, arguments) of every launch the GPU module makes for a case."""
    for config in bb.CONFIGS:
        for nsrc in ((1, 2, 3) if config == "res" else (3,)):
            yield "%s %d sources" % (config, nsrc), bb.config_args(cs, config, nsrc), nsrc


@pytest.mark.parametrize("kind,n,c", CASES, ids=["%s-%dx%d" % k for k in CASES])
def test_the_emulation_meets_every_limit_with_margin(kind, n, c):
    cs = bb.case(kind, n, c)
    for label, args, nsrc in _runs(cs):
        r = bb.reference(**args)
        L = bb.limits(r)
        assert L.excluded.mean() <= bb.EXCLUDED_CAP, "%s %dx%d %s: %d of %d columns excluded" % (kind, n, c, label, L.excluded.sum(), c)
        got = bb.emulate(**args)
        for name, ratio in bb.within(got, r, L, "%s %dx%d %s" % (kind, n, c, label)).items():
            cap = (nsrc - 1.0) / nsrc if (name == "gres" and nsrc > 2) else MARGIN
            assert ratio <= cap, "%s %dx%d %s: %s at %.3f of its limit: the derivation misses a term" % (kind, n, c, label, name, ratio)
        if args["relu"] and n >= 64:                             # the ReLU is open in a part of the elements, closed in another
            assert 0.02 < float((got["y"] > 0).mean()) < 0.98


LARGE = [(k, n, c) for k in bb.GPU_KINDS for (n, c) in bb.SHAPES if n > 8193]


@pytest.mark.parametrize("kind,n,c", LARGE, ids=["%s-%dx%d" % k for k in LARGE])
def test_the_reference_excludes_few_columns_at_the_large_shapes(kind, n, c):
    cs = bb.case(kind, n, c)
    for config in ("res", "mask", "eval"):
        L = bb.limits(bb.reference(**dict(bb.config_args(cs, config, 0))))
        assert L.excluded.mean() <= bb.EXCLUDED_CAP, "%s %dx%d %s: %d of %d columns excluded" % (kind, n, c, config, L.excluded.sum(), c)


@functools.lru_cache(maxsize=None)
def _mutant_reference(kind, n, c):
    args = bb.config_args(bb.case(kind, n, c), "res", 3)
    r = bb.reference(**args)
    return args, r, bb.limits(r)


@pytest.mark.parametrize("mutant", bb.MUTANTS)
def test_each_mutant_breaks_a_limit(mutant):
    broke, slipped = [], []
    for key in MUTANT_CASES:
        args, r, L = _mutant_reference(*key)
        got = bb.emulate(mutant=mutant, **args)
        bad = sorted(k for k, v in bb.ratios(got, r, L).items() if v[1])
        print("mutant %s %s: beyond the limit: %s; tensor-max check %s" % (mutant, key, bad, "passes" if bb.tensor_max_check(got, r) else "fails"))
        if bad:
            broke.append(key)
            if key[0] == "scales" and bb.tensor_max_check(got, r):
                slipped.append(key)
    assert broke, "mutant %s stays inside every limit on every case" % mutant
    # the gap on record: these defects pass the tensor-max check of test_gpu_dense.py on inputs where they break a limit here
    assert bool(slipped) == (mutant in PASS_THE_TENSOR_MAX_CHECK), "mutant %s: tensor-max check passes it on %s" % (mutant, slipped)


def test_the_correct_emulation_passes_the_tensor_max_check():
    """(so that a mutant failing it above is the mutant's doing)"""
    for key in MUTANT_CASES:
        if key[0] == "scales":                                   # (on "offset" a rounding of the mean, 2^-24 * 4096, is beyond 2e-5 of max |y|)
            args, r, L = _mutant_reference(*key)
            assert bb.tensor_max_check(bb.emulate(**args), r), key


def test_input_kinds_are_what_their_names_say():
    g = np.random.default_rng(0)
    x, gs = bb.columns("scales", 4096, 36, g)
    assert float(x[:, 0].min()) == float(x[:, 0].max()) == 3.25
    sd, mu = x[:, 1:].astype(np.float64).std(0), np.abs(x[:, 1:].astype(np.float64).mean(0))
    assert sd.max() / sd.min() > 1e3 and (mu / sd).max() > 10 and 1e-3 * 0.9 <= gs.min() and gs.max() <= 1e3 * 1.1
    x, _ = bb.columns("offset", 4096, 36, g)
    m = x.astype(np.float64).mean(0)
    assert abs(m[12] - 4096) < 0.1 and abs(m[13] - 1) < 0.1 and abs(x[:, 12].astype(np.float64).std() - 1) < 0.05
    cs = bb.case("scales", 513, 20)
    assert float(cs.x[:, 0].min()) == float(cs.x[:, 0].max()) == 3.25 and not cs.x.flags.writeable
    assert np.shares_memory(cs.gys[0], cs.wide) and cs.gys[0].shape == (513, 20)
