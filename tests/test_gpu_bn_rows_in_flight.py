"""The batch-norm kernels with several rows in flight and column-keeping apply walks (csrc/bn.hip) against the kernels they replace,
which osn_bn_set_flat_kernels(1) runs in the same process: the flat apply kernels and column sums with one row in flight.

Every case = one (n, c); every variant of it runs three times -- new kernels, earlier kernels, new kernels again -- and ALL outputs of
the three runs are compared bit for bit (forward: y, the whole matrix that holds the second store, mean, var, the running buffers;
backward: gx, gres, ggamma, gbeta).
  rows    1, 15, 16, 17      fewer rows than the column sums' 16 row lanes, and one more
          207, 208, 209      208 = 13 x 16 = a level-0 block of the column sums: a ragged last round for every R, one row either side
          4097               the first size past the one-launch forward (the three-launch path with one 64-row block too many)
          70001              several strides of the apply walk (c >= 32), 137-row blocks: 8 full rounds + a ragged one for R = 2, 4
  widths  4, 32 (c4 = 8), 96 (c4 = 24: the stride's period is 3 workgroups), 100 (c4 = 25), 192, 260 (c4 = 65) and 772 (c4 = 193).
          The plan helper says which apply kernels run: 260 keeps its columns at every size; 772 does from 207 rows on and takes the
          flat kernels at 1 .. 17 rows (no grid within 127 workgroups of the wanted one is a multiple of 193) -- asserted below.
  forward variants   residual x ReLU x second store (ld2 = c + 16, column offset 4), training mode and evaluation mode, and the
                     evaluation-mode apply IN PLACE on x
  backward variants  (ReLU, training) x 1 .. 3 gradient sources, each a column window of a wider matrix (row strides c + 24, c + 8,
                     c + 4), x: no gres with the mask from y / the mask recomputed from x (y null) / gres in a buffer of its own (the
                     reduction stores it) / gres written in place over a contiguous source 0 (the aliased flow)
Float64: where the reference of tests/bn_bounds.py (long-double column sums) takes well under a second -- n x c <= 450 000, which holds
for every width up to 209 rows, for 4097 rows at c <= 100 and for 70001 x 4 -- one configuration of bb.CONFIGS per shape (rotating with
the shape, as the source count does) is also held to the limits of bn_bounds.limits().  Both sets of kernels take their per-element
expressions from one definition each (csrc/epilogue.h), so at the larger shapes the bitwise comparison covers the walks and the loop
structure -- rows in flight, ragged rounds, kept columns -- against the earlier ones; the expressions themselves are held by
tests/test_gpu_bn_bounds.py (the same limits) and tests/test_gpu_bn_backward_gres.py (gres bitwise against torch).
Every case also prints  BITS <n>x<c> <sha256>  over every tensor it compares, in the order produced (_feed): two builds of the library
are compared by running this file once with each and comparing the lines.
"""
import hashlib

import numpy as np
import pytest
import torch

import bn_bounds as bb

pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 207, 208, 209, 4097, 70001)
CS = (4, 32, 96, 100, 192, 260, 772)
SHAPES = [(n, c) for n in NS for c in CS]
MODES = [(True, True), (True, False), (False, True), (False, False)]          # (relu, training)
F64_MAX = 450000
FWD_NAMES = ("y", "second", "mean", "var", "rm", "rv")
BWD_NAMES = ("gx", "gres", "ggamma", "gbeta")


def dev():
    return torch.device("cuda", 0)


def _ops():
    from openscene_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(names, a, b, label):
    assert len(a) == len(b)
    for name, u, v in zip(names, a, b):
        assert (u is None) == (v is None), "%s: %s" % (label, name)
        if u is not None:
            assert torch.equal(_bits(u), _bits(v)), "%s: %s differs" % (label, name)


def _feed(digest, *outs):
    """Every tensor of `outs` into the case's digest: its shape and two 64-bit sums of its 32-bit words, taken on the device (the largest
    case compares some 60 GB: minutes of hashing on the host).  The sums wrap, under the odd weights 2 i + 1 and 2 i^2 + 1 of word i: a
    changed word changes both, whatever the change."""
    for t in outs:
        if t is None:
            continue
        w = _bits(t).reshape(-1).to(torch.int64)
        i = torch.arange(w.numel(), dtype=torch.int64, device=w.device)
        sums = torch.stack([(w * (2 * i + 1)).sum(), (w * (2 * i * i + 1)).sum()])
        digest.update(repr(tuple(t.shape)).encode() + sums.cpu().numpy().tobytes())


def _three_runs(ops, names, fn, label, digest):
    """fn() with the new kernels, with the earlier ones, with the new ones again: every output bitwise the same.  -> the first."""
    new = fn()
    assert ops.bn_set_flat_kernels(True) is False
    try:
        old = fn()
    finally:
        assert ops.bn_set_flat_kernels(False) is True
    again = fn()
    _feed(digest, *new, *old, *again)
    _same(names, new, old, label + ": new kernels against the earlier ones")
    _same(names, new, again, label + ": second call")
    return new


def _numpy_inputs(n, c, config):
    """Inputs on the host (float64-checked shapes), with the pre-activations of `config` moved away from zero as bn_bounds.case does."""
    g = np.random.default_rng(bb._seed("rows in flight", n, c))
    f = np.float32
    x = (g.standard_normal((n, c)) * 2.5 + 0.7).astype(f)
    d = dict(x=x, gamma=g.uniform(0.5, 1.5, c).astype(f), beta=(g.uniform(0.1, 0.5, c) * g.choice([-1.0, 1.0], c)).astype(f),
             res=g.standard_normal((n, c)).astype(f), res_eval=g.standard_normal((n, c)).astype(f),
             w0=g.standard_normal((n, c + 24)).astype(f), w1=(3.0 * g.standard_normal((n, c + 8))).astype(f),
             w2=(0.25 * g.standard_normal((n, c + 4))).astype(f))
    d["rm"] = (x.mean(0) * (1 + 0.1 * g.standard_normal(c))).astype(f)
    d["rv"] = ((x.var(0) + 0.5) * g.uniform(0.5, 2.0, c)).astype(f)
    cs = _case(d, n, c)

    def move_x(r, L, bad):
        step = np.maximum(16 * L.y / np.abs(r.ga * r.is_), 4 * np.spacing(np.abs(x)).astype(np.float64))
        x[bad] = (x.astype(np.float64) + np.where(r.pre >= 0, 1.0, -1.0) * np.sign(r.ga) * step)[bad].astype(f)

    def move_res(which):
        def move(r, L, bad):
            which[bad] = (which.astype(np.float64) + np.where(r.pre >= 0, 1.0, -1.0) * 16 * L.y)[bad].astype(f)
        return move

    if config == "mask":
        bb._push_away(bb.config_args(cs, "mask"), move_x, keep_constant=True)
    elif config in ("res", "eval"):
        bb._push_away(bb.config_args(cs, config), move_res(d["res"] if config == "res" else d["res_eval"]))
    return d


def _case(d, n, c):
    gys = (d["w0"][:, 8:8 + c], d["w1"][:, 4:4 + c], d["w2"][:, :c])
    return bb.Case("plain", n, c, d["x"], d["gamma"], d["beta"], d["res"], d["res_eval"], d["w0"], gys, d["rm"], d["rv"])


def _device_inputs(n, c):
    g = torch.Generator(device=dev())
    g.manual_seed(bb._seed("rows in flight", n, c))

    def rn(*shape):
        return torch.randn(*shape, generator=g, device=dev())
    d = dict(x=rn(n, c) * 2.5 + 0.7, gamma=torch.rand(c, generator=g, device=dev()) + 0.5, beta=rn(c) * 0.3, res=rn(n, c), res_eval=rn(n, c),
             w0=rn(n, c + 24), w1=3.0 * rn(n, c + 8), w2=0.25 * rn(n, c + 4))
    d["rm"] = d["x"].mean(0) * 1.05
    d["rv"] = d["x"].var(0, unbiased=False) * 1.3 + 0.5
    return d


@pytest.mark.parametrize("n,c", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_new_kernels_give_the_bits_of_the_earlier_ones(n, c):
    ops = _ops()
    index = SHAPES.index((n, c))
    digest = hashlib.sha256()
    config, nsrc64 = bb.CONFIGS[index % 4], 1 + index % 3
    host = _numpy_inputs(n, c, config) if n * c <= F64_MAX else None
    T = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev()) for k, v in host.items()} if host else _device_inputs(n, c)
    x, gamma, beta, res, res_eval, rm, rv = (T[k] for k in ("x", "gamma", "beta", "res", "res_eval", "rm", "rv"))
    srcs = [T["w0"][:, 8:8 + c], T["w1"][:, 4:4 + c], T["w2"][:, :c]]
    assert all(s.stride(0) > c for s in srcs)

    # ---- which apply kernels run, from the plan helper
    grid, flat = ops.bn_apply_plan(n * (c // 4), c // 4)
    assert flat or (grid * 256) % (c // 4) == 0
    if c == 260:
        assert not flat, "c = 260 keeps its columns at every size"
    if c == 772:
        assert flat == (n <= 17), "c = 772 takes the flat kernels exactly below 207 rows"
    if c in (4, 32, 96, 192):
        assert not flat
    print("PLAN %dx%d grid %d %s" % (n, c, grid, "flat" if flat else "columns kept"))

    def second():
        return torch.full((n, c + 16), 7.0, device=dev())

    # ---- forward
    for r in (None, res):
        for relu in (False, True):
            for two in (False, True):
                label = "%dx%d forward, residual %d relu %d second store %d" % (n, c, r is not None, relu, two)

                def train():
                    a, b = rm.clone(), rv.clone()
                    if two:
                        w = second()
                        y, mean, var = ops.bn_forward_train(x, gamma, beta, bb.EPS, r, relu, a, b, bb.MOMENTUM, y2=w[:, 4:4 + c])
                        assert torch.equal(_bits(w[:, 4:4 + c]), _bits(y)), label + ": the second store is not y"
                        return y, w, mean, var, a, b
                    y, mean, var = ops.bn_forward_train(x, gamma, beta, bb.EPS, r, relu, a, b, bb.MOMENTUM)
                    return y, None, mean, var, a, b

                def evaluate():
                    w = second() if two else None
                    y = ops.bn_apply(x, rm, rv, gamma, beta, bb.EPS, r if r is None else res_eval, relu, y2=w[:, 4:4 + c] if two else None)
                    return y, w
                _three_runs(ops, FWD_NAMES, train, label + ", training", digest)
                ev = _three_runs(ops, FWD_NAMES[:2], evaluate, label + ", evaluation", digest)
                if two:
                    assert torch.equal(_bits(ev[1][:, 4:4 + c]), _bits(ev[0])) and bool((ev[1][:, :4] == 7.0).all()) and bool((ev[1][:, 4 + c:] == 7.0).all())
                if not two:                       # y in place on x: the bits of the call with a y of its own
                    xin = x.clone()
                    out = ops.bn_apply(xin, rm, rv, gamma, beta, bb.EPS, r if r is None else res_eval, relu, out=xin)
                    assert out.data_ptr() == xin.data_ptr()
                    _feed(digest, out)
                    _same(("y",), (ev[0],), (out,), label + ", evaluation in place on x")

    # ---- backward
    y_of, stats_of = {}, {}
    for relu, training in MODES:
        if training:
            y_of[relu, training], m, v = ops.bn_forward_train(x, gamma, beta, bb.EPS, res, relu, rm.clone(), rv.clone(), bb.MOMENTUM)
            stats_of[relu, training] = (m, v)
        else:
            y_of[relu, training], stats_of[relu, training] = ops.bn_apply(x, rm, rv, gamma, beta, bb.EPS, res_eval, relu), (rm, rv)
    for relu, training in MODES:
        y, (mean, var) = y_of[relu, training], stats_of[relu, training]
        for k in (1, 2, 3):
            label = "%dx%d backward, relu %d training %d, %d sources" % (n, c, relu, training, k)
            plain = _three_runs(ops, BWD_NAMES, lambda: ops.bn_backward_multi(x, y, srcs[:k], mean, var, gamma, bb.EPS, relu, training, False),
                                label + ", no gres", digest)
            own = _three_runs(ops, BWD_NAMES, lambda: ops.bn_backward_multi(x, y, srcs[:k], mean, var, gamma, bb.EPS, relu, training, True),
                              label + ", gres stored by the reduction", digest)
            _same(("gx", "ggamma", "gbeta"), (plain[0],) + plain[2:], (own[0],) + own[2:], label + ": with gres against without")
            g0 = srcs[0].contiguous()

            def aliased():
                inplace = g0.clone()
                out = ops.bn_backward_multi(x, y, [inplace] + srcs[1:k], mean, var, gamma, bb.EPS, relu, training, True, gres_out=inplace)
                assert out[1].data_ptr() == inplace.data_ptr()
                return out
            _same(BWD_NAMES, own, _three_runs(ops, BWD_NAMES, aliased, label + ", gres over source 0", digest),
                  label + ": aliased against a gres of its own")
            if relu:
                # the mask recomputed from x (no residual: y = relu(bn(x)) is what the kernels rebuild, bit for bit)
                yx = ops.bn_forward_train(x, gamma, beta, bb.EPS, None, True, rm.clone(), rv.clone(), bb.MOMENTUM)[0] if training else \
                    ops.bn_apply(x, rm, rv, gamma, beta, bb.EPS, None, True)
                from_x = _three_runs(ops, BWD_NAMES, lambda: ops.bn_backward_multi(x, None, srcs[:k], mean, var, gamma, bb.EPS, True, training, False,
                                                                                   beta=beta), label + ", mask from x", digest)
                from_y = ops.bn_backward_multi(x, yx, srcs[:k], mean, var, gamma, bb.EPS, True, training, False)
                _feed(digest, yx, *from_y)
                _same(BWD_NAMES, from_x, from_y, label + ": mask from x against mask from y")

    print("BITS %dx%d %s" % (n, c, digest.hexdigest()))

    # ---- one configuration against float64 (bn_bounds)
    if host is None:
        return
    args = bb.config_args(_case(host, n, c), config, nsrc64)
    ref = bb.reference(**args)
    L = bb.limits(ref)
    label = "%dx%d %s, %d sources against float64" % (n, c, config, nsrc64)
    assert L.excluded.mean() <= bb.EXCLUDED_CAP, "%s: %d of %d columns excluded" % (label, L.excluded.sum(), c)
    relu, training, r = config != "plain", config != "eval", {"plain": None, "res": res, "mask": None, "eval": res_eval}[config]
    got = {}
    if training:
        a, b = rm.clone(), rv.clone()
        y, mean, var = ops.bn_forward_train(x, gamma, beta, bb.EPS, r, relu, a, b, bb.MOMENTUM)
        got.update(mean=mean, var=var, rm=a, rv=b)
    else:
        y, mean, var = ops.bn_apply(x, rm, rv, gamma, beta, bb.EPS, r, relu), rm, rv
    out = ops.bn_backward_multi(x, None if config == "mask" else y, srcs[:nsrc64], mean, var, gamma, bb.EPS, relu, training, r is not None,
                                beta=beta if config == "mask" else None)
    got.update(y=y, **dict(zip(BWD_NAMES, out)))
    flat_ratios = bb.within({k: v.cpu().numpy() for k, v in got.items() if v is not None}, ref, L, label)
    print("RATIO %s %s" % (label, "  ".join("%s %.3f" % kv for kv in sorted(flat_ratios.items()))))
