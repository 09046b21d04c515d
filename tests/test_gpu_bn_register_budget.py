"""The backward column sums whose operands are compile-time choices (csrc/bn.hip: one kernel per ReLU mask -- none, from x, from y --
each with a row loop for one gradient source and one for up to three; the sums that store gres keep run-time operands) and the
weight-stationary reduction that keeps nine of its K quads in flight (csrc/spconv_ws.hip) -- the kernels sized to the registers the
weight gradients leave on a SIMD.

Batch norm: osn_bn_backward against the same call under osn_bn_set_flat_kernels(1) (the one-row loop of the earlier rounds, every
operand a run-time choice), bit for bit in gx, gres, ggamma and gbeta.
  rows     1, 15, 16, 17, 31, 32, 33, 209: fewer rows than the 16 row lanes, 16 R and 16 R + 1 for R = 1 and 2 rows in flight (the
           sums without a gres store keep one, those with it two), one below 32, and 209 = several rounds and a ragged one
  widths   4, 60, 64, 68, 96: less than one 64-column group, exactly one, one quad more (a second, nearly empty group), the level-0 width
  sources  1 (contiguous, and as a column window), 2 and 3 (source 0 contiguous, the others column windows with ld > c)
  masks    ReLU off / ReLU with y / ReLU with the mask from x (y null, beta given)
  gres     none / stored by the reduction into a buffer of its own / written over source 0 (the overlap that disables the store)
  values   one NaN and one -0.0 in source 0: a NaN stays a NaN in its column's sums and in gx, under every mask
Reduction: osn_spconv_fwd_ws on hand-made tables whose per-offset products are exact in float32 (small integers times a power of two
per offset), so the only rounding is the sum over the offsets -- compared bit for bit with a float32 running sum in ascending k formed
with numpy.  K = 27 and 8, 1 / 63 / 257 rows, 4 / 96 / 128 columns; rows with no, one and all K neighbours.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-5
NS = (1, 15, 16, 17, 31, 32, 33, 209)
CS = (4, 60, 64, 68, 96)
BWD_NAMES = ("gx", "gres", "ggamma", "gbeta")


def dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, label):
    for name, u, v in zip(BWD_NAMES, a, b):
        assert (u is None) == (v is None), "%s: %s" % (label, name)
        if u is not None:
            assert torch.equal(_bits(u), _bits(v)), "%s: %s differs from the one-row kernels'" % (label, name)


def _both(ops, fn, label):
    """fn() with the product kernels and under osn_bn_set_flat_kernels(1): the same bits.  -> the product's outputs"""
    new = fn()
    assert ops.bn_set_flat_kernels(True) is False
    try:
        old = fn()
    finally:
        assert ops.bn_set_flat_kernels(False) is True
    _same(new, old, label)
    return new


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_backward_sums_give_the_bits_of_the_one_row_kernels(n, c):
    from openscene_amd import ops
    g = torch.Generator(device=dev())
    g.manual_seed(1000 * n + c)

    def rn(*shape):
        return torch.randn(*shape, generator=g, device=dev())
    x = rn(n, c) * 2.5 + 0.7
    gamma, beta, res = torch.rand(c, generator=g, device=dev()) + 0.5, rn(c) * 0.3, rn(n, c)
    rm, rv = torch.zeros(c, device=dev()), torch.ones(c, device=dev())
    w0, w1, w2 = rn(n, c), 3.0 * rn(n, c + 8), 0.25 * rn(n, c + 4)
    w0[0, 1 % c] = float("nan")
    w0[n // 2, 2 % c] = -0.0
    wide0 = torch.zeros(n, c + 24, device=dev())
    wide0[:, 8:8 + c] = w0
    srcs = [w0, w1[:, 4:4 + c], w2[:, :c]]
    source_sets = [("1 source", [w0]), ("1 source, a column window", [wide0[:, 8:8 + c]]), ("2 sources", srcs[:2]), ("3 sources", srcs)]
    assert n == 1 or (wide0[:, 8:8 + c].stride(0) > c and all(s.stride(0) > c for s in srcs[1:]))
    y_res, mean, var = ops.bn_forward_train(x, gamma, beta, EPS, res, True, rm.clone(), rv.clone(), 0.1)
    y_plain = ops.bn_forward_train(x, gamma, beta, EPS, None, True, rm.clone(), rv.clone(), 0.1)[0]
    nan_col = 1 % c

    for what, ss in source_sets:
        for training in (True, False):
            label = "%dx%d, %s, training %d" % (n, c, what, training)
            outs = {}
            # ReLU off: no gres / gres of its own
            outs["off"] = _both(ops, lambda: ops.bn_backward_multi(x, y_res, ss, mean, var, gamma, EPS, False, training, False), label + ", relu off")
            outs["off gres"] = _both(ops, lambda: ops.bn_backward_multi(x, y_res, ss, mean, var, gamma, EPS, False, training, True),
                                     label + ", relu off, gres stored")
            # ReLU with y: no gres / gres of its own / gres over source 0
            outs["y"] = _both(ops, lambda: ops.bn_backward_multi(x, y_res, ss, mean, var, gamma, EPS, True, training, False), label + ", mask from y")
            outs["y gres"] = _both(ops, lambda: ops.bn_backward_multi(x, y_res, ss, mean, var, gamma, EPS, True, training, True),
                                   label + ", mask from y, gres stored")
            for relu in (False, True):
                def aliased():
                    inplace = ss[0].contiguous().clone()
                    out = ops.bn_backward_multi(x, y_res, [inplace] + ss[1:], mean, var, gamma, EPS, relu, training, True, gres_out=inplace)
                    assert out[1].data_ptr() == inplace.data_ptr()
                    return out
                _same(outs["y gres" if relu else "off gres"], _both(ops, aliased, label + ", relu %d, gres over source 0" % relu),
                      label + ", relu %d: gres over source 0 against a gres of its own" % relu)
            # ReLU with the mask from x (no residual): the bits of the mask from y = relu(bn(x))
            outs["x"] = _both(ops, lambda: ops.bn_backward_multi(x, None, ss, mean, var, gamma, EPS, True, training, False, beta=beta),
                              label + ", mask from x")
            _same(outs["x"], ops.bn_backward_multi(x, y_plain, ss, mean, var, gamma, EPS, True, training, False), label + ": mask from x against y")
            # with a gres store or without: the same gx and sums
            _same((outs["y"][0], None) + outs["y"][2:], (outs["y gres"][0], None) + outs["y gres"][2:], label + ": with gres against without")
            # the NaN of source 0 stays in its column's sums wherever its row is not masked off, and in gres where gres is formed
            for key, out in outs.items():
                kept = key.startswith("off") or bool(((y_res if key.startswith("y") else y_plain)[0, nan_col] > 0).item())
                assert bool(torch.isnan(out[3][nan_col]).item()) == kept, "%s, %s: gbeta[%d]" % (label, key, nan_col)
                if out[1] is not None:
                    assert bool(torch.isnan(out[1][0, nan_col]).item()) == kept, "%s, %s: gres" % (label, key)
                others = torch.ones(c, dtype=torch.bool, device=dev())
                others[nan_col] = False
                assert not bool(torch.isnan(out[3][others]).any().item()), "%s, %s: a NaN outside its column" % (label, key)


def _ws_case(K, n_dst, cout, only_one=False):
    """A hand-made map (n_in = n_dst, a permutation per offset with about half its entries kept; row 0 no neighbour, row 1 one, row 2
    all K when there are that many rows; one row: all K, or one) and operands whose per-offset products are exact in float32."""
    rng = np.random.default_rng(100 * K + 7 * n_dst + cout)
    cin = 8
    nbr = np.stack([rng.permutation(n_dst) for _ in range(K)]).astype(np.int32)
    nbr[rng.random((K, n_dst)) < 0.5] = -1
    if n_dst == 1:
        nbr[:] = 0
        if only_one:
            nbr[:] = -1
            nbr[K // 2] = 0
    else:
        nbr[:, 0] = -1
        nbr[:, 1] = -1
        nbr[K // 3, 1] = 5
        nbr[:, 2] = np.arange(K) % n_dst
    feats = rng.integers(-15, 16, (n_dst, cin)).astype(np.float32)
    w = rng.integers(-7, 8, (K, cin, cout)).astype(np.float32) * np.exp2(rng.integers(-6, 25, (K, 1, 1))).astype(np.float32)
    return nbr, feats, w


def _ws_reference(nbr, feats, w):
    K, n_dst = nbr.shape
    out = np.zeros((n_dst, w.shape[2]), dtype=np.float32)
    for k in range(K):
        on = nbr[k] >= 0
        p64 = feats[nbr[k][on]].astype(np.float64) @ w[k].astype(np.float64)
        p = p64.astype(np.float32)
        assert np.array_equal(p.astype(np.float64), p64), "the products of one offset must be exact in float32"
        out[on] = out[on] + p                                 # float32 running sum, ascending k
    return out


@pytest.mark.parametrize("cout", (4, 96, 128))
@pytest.mark.parametrize("n_dst", (1, 63, 257))
@pytest.mark.parametrize("K", (27, 8))
def test_ws_reduction_is_the_float32_running_sum_in_ascending_k(K, n_dst, cout):
    from openscene_amd import ops
    for only_one in ((False, True) if n_dst == 1 else (False,)):
        nbr, feats, w = _ws_case(K, n_dst, cout, only_one)
        counts = (nbr >= 0).sum(0)
        assert n_dst == 1 or (counts[0] == 0 and counts[1] == 1 and counts[2] == K)
        ref = _ws_reference(nbr, feats, w)
        # the sum over the offsets does round, and not as the descending sum does: the order is what is tested
        if n_dst > 1:
            back = _ws_reference(nbr[::-1], feats, w[::-1])
            assert not np.array_equal(ref, back)
        nbr_d = torch.from_numpy(nbr).to(dev())
        tl = ops.tile_lists(nbr_d)
        wf, _ = ops.weight_prep_tl(torch.from_numpy(w).to(dev()), want_dgrad=False)
        out = ops.spconv_fwd_ws(torch.from_numpy(feats).to(dev()), wf, tl, nbr_d, n_dst, K, cout)
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.int32), ref.view(np.int32)), "K %d, %d rows, %d columns: %d elements differ" % (
            K, n_dst, cout, int((got.view(np.int32) != ref.view(np.int32)).sum()))
