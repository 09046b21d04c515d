"""The open-vocabulary query kernels (csrc/query.hip) against the contract of tests/query_bounds.py, through ops.cosine_query,
ops.query_ensemble, the two vote entry points and ops.rows_argmax: every fp16 score inside the fp16 rounding of the float64 score
+- 2e-6 of its abs-sum, on six operand kinds; every label equal to torch.max of the kernel's own scores, on rows that mix NaN, +-inf,
signed zeros and exact ties with ordinary scores, and equal to the float64 argmax wherever that is decided.
test_query_bounds_cpu.py shows that these shapes and operands tell a subtly wrong kernel from a right one.

Shapes: query_kernel<CT> at both ends of every CT instance and with two and three column groups, one row / a second workgroup of
one row / a ragged third, feature widths below one 64-chunk, with a ragged 8 and at the CLIP width; query_wide_kernel<D, NCW> in its
six instances at both ends of every NCW, at the 4096-point switch (4095 points: the same shape on query_kernel, bit-identical) and
with more tiles than compute units, the last tile holding one point.

Worst c' / c per kernel family (the smallest constant that would admit the score, over 2e-6; 0 = the rounding of the float64 score
itself), measured on an MI355X (every case prints its figure):
    family                     unit    row_scales  wide_elements  coherent  cancellation  half_ties
    query_kernel               0.03    0.02        0.06           0.17      0.01          0.02
    query_wide_kernel          0.02    0.01        0.06           0.25      0.00          0.02
    ensemble (both kernels)    0.02 (its own operands)
The 4095-point launch of query_kernel and the 4096-point launch of query_wide_kernel agree bit for bit on every kind.
"""
import numpy as np
import pytest
import torch

import query_bounds as qb

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def bits_equal(a, b):
    """fp16 tensors equal bit for bit; a NaN matches a NaN (payloads are not part of the contract)."""
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a.view(torch.int16)[~na], b.view(torch.int16)[~nb])


def check_labels(labels, scores, ref=None, rows=None):
    labels = labels.cpu()
    assert labels.dtype == torch.int64 and torch.equal(labels, qb.torch_max_labels(scores))
    if ref is not None:                                     # the float64 argmax wherever it is decided
        w, dec = qb.decided(ref)
        if rows is not None:
            w, dec = w[rows], dec[rows]
        assert np.array_equal(labels.numpy()[dec], w[dec])


def check_query(kind, n, n_rows, d, c, no_gather=True):
    """One operand kind through cosine_query (with the gather, labels only, without the gather where n == n_rows) and through
    cosine_query_vote from a zero vote matrix.  -> (worst ratio, the gathered scores)."""
    from openscene_amd import ops
    x, t = qb.operands(kind, n_rows, d, c)
    ref = qb.reference(kind, n_rows, d, c)
    xg, tg = x.to(dev()), t.to(dev())
    rows = qb.gather_index(n, x.shape[0])
    g = rows.to(dev())
    label = "%s n=%d d=%d c=%d" % (kind, n, d, c)
    scores, labels = ops.cosine_query(xg, tg, g)
    ratio = qb.within(scores, ref, rows.numpy(), label)
    check_labels(labels, scores, ref, rows.numpy())
    none, labels2 = ops.cosine_query(xg, tg, g, want_scores=False)
    assert none is None and torch.equal(labels2, labels), label + ": labels-only call"
    votes = torch.zeros((n, c), dtype=torch.float16, device=dev())
    labels3 = ops.cosine_query_vote(xg, tg, votes, g, want_labels=True)
    assert torch.equal(labels3, labels), label + ": vote labels"
    assert bits_equal(votes, scores.cpu() + torch.zeros((n, c), dtype=torch.float16)), label + ": votes from zero"    # (-0 + 0 = +0)
    if no_gather and n == x.shape[0]:
        s0, l0 = ops.cosine_query(xg, tg)
        ratio = max(ratio, qb.within(s0, ref, None, label + " no gather"))
        check_labels(l0, s0, ref)
        assert bits_equal(s0[g], scores), label + ": gathered and direct rows differ"
    return ratio, scores


NARROW = sorted(set([(n, d, c) for n in (1, 129, 300) for d in (8, 72, 520, 768) for c in (33, 161)]
                    + [(129, 72, c) for c in (1, 32, 33, 64, 65, 96, 97, 160, 161, 321)]))


@pytest.mark.parametrize("n,d,c", NARROW)
def test_query_kernel(n, d, c):
    worst = {kind: check_query(kind, n, n, d, c)[0] for kind in qb.KINDS}
    print("QB query_kernel n=%d d=%d c=%d %s" % (n, d, c, " ".join("%s=%.3f" % kv for kv in worst.items())))


WIDE = [(d, c) for d in (512, 768) for c in (65, 96, 97, 128, 129, 160)]
WIDE_ROWS = 4096


def wide_kinds(d, c):
    return qb.KINDS if (d, c) in ((768, 160), (512, 65)) else ("unit", "coherent", "cancellation")


@pytest.mark.parametrize("d,c", WIDE)
def test_query_wide_kernel_at_the_switch(d, c):
    """4096 points: the fewest query_wide_kernel takes; with and without the gather."""
    worst = {kind: check_query(kind, WIDE_ROWS, WIDE_ROWS, d, c)[0] for kind in wide_kinds(d, c)}
    print("QB query_wide_kernel n=%d d=%d c=%d %s" % (WIDE_ROWS, d, c, " ".join("%s=%.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("d,c", WIDE)
def test_query_wide_kernel_wraps_onto_a_ragged_tile(d, c):
    """32 * CUs + 33 points gathered from the 4096 feature rows: more tiles than persistent workgroups, so some run a second tile
    (the other LDS buffer), and the last tile holds one point."""
    n = 32 * torch.cuda.get_device_properties(dev()).multi_processor_count + 33
    worst = {kind: check_query(kind, n, WIDE_ROWS, d, c)[0] for kind in wide_kinds(d, c)}
    print("QB query_wide_kernel n=%d d=%d c=%d %s" % (n, d, c, " ".join("%s=%.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("kind", qb.KINDS)
def test_both_kernels_give_the_same_bits_across_the_switch(kind):
    """4095 points take query_kernel, 4096 query_wide_kernel (c = 160, d = 768): the header promises the same accumulation order,
    so rows 0 .. 4094 are bit-identical; the narrow launch obeys the contract on its own."""
    from openscene_amd import ops
    d, c = 768, 160
    x, t = qb.operands(kind, WIDE_ROWS, d, c)
    ref = qb.reference(kind, WIDE_ROWS, d, c)
    xg, tg = x.to(dev()), t.to(dev())
    s_wide, l_wide = ops.cosine_query(xg, tg)
    s_narrow, l_narrow = ops.cosine_query(xg[:WIDE_ROWS - 1], tg)
    rows = np.arange(WIDE_ROWS - 1)
    ratio = qb.within(s_narrow, ref, rows, "%s n=4095 d=768 c=160" % kind)
    check_labels(l_narrow, s_narrow, ref, rows)
    print("QB query_kernel n=4095 d=768 c=160 %s=%.3f" % (kind, ratio))
    assert bits_equal(s_narrow, s_wide[:WIDE_ROWS - 1]) and torch.equal(l_narrow, l_wide[:WIDE_ROWS - 1])


@pytest.mark.parametrize("n,n_vox,d,c", qb.ENSEMBLE_SHAPES)
def test_query_ensemble(n, n_vox, d, c):
    """row_norm_kernel, the rowdiv / rowmax paths, ensemble_select_kernel and the X1 / g1 offsets: the selection equals the float64
    reference's wherever the two best normalised scores have disjoint intervals; every row's scores obey the score contract of the
    source the kernel says it selected (a decided row: the reference's source; an undecided one: one of the two)."""
    from openscene_amd import ops
    ens = qb.ensemble_case(n, n_vox, d, c)
    xd, xf, t, gd, gf = (a.to(dev()) for a in (ens.xd, ens.xf, ens.text, ens.gd, ens.gf))
    scores, labels, sel = ops.query_ensemble(xd, xf, t, gd, gf)
    sel_np = sel.cpu().numpy()
    wrong = int((sel_np != ens.sel)[ens.decided].sum())
    assert wrong == 0, "%d decided points took the other source" % wrong
    ratio = 0.0
    for src, ref in ((False, ens.ref_d), (True, ens.ref_f)):
        m = sel_np == src
        if m.any():
            ratio = max(ratio, qb.worst_ratio(scores.cpu().numpy()[m], qb.Ref(*(a[m] for a in ref)))[0])
    n_bad = int(qb.ensemble_scores_outside(scores, sel, ens).sum())
    print("QB ensemble n=%d d=%d c=%d ratio=%.3f outside=%d" % (n, d, c, ratio, n_bad))
    assert n_bad == 0, "%d scores outside the selected source's interval, worst ratio %.2f" % (n_bad, ratio)
    check_labels(labels, scores)
    assert not scores[0].cpu().float().abs().any() and not torch.signbit(scores[0].float()).any() and int(labels[0]) == 0 and not bool(sel[0])
    none, labels2, sel2 = ops.query_ensemble(xd, xf, t, gd, gf, want_scores=False)
    assert none is None and torch.equal(labels2, labels) and torch.equal(sel2, sel)
    votes = torch.zeros((n, c), dtype=torch.float16, device=dev())
    labels3, sel3 = ops.query_ensemble_vote(xd, xf, t, votes, gd, gf, want_labels=True)
    assert torch.equal(labels3, labels) and torch.equal(sel3, sel)
    assert bits_equal(votes, scores.cpu() + torch.zeros((n, c), dtype=torch.float16))


@pytest.mark.parametrize("n,c", [(16, 1), (40, 3), (40, 64), (40, 97), (300, 161)])
def test_rows_argmax_label_rule(n, c):
    """ops.rows_argmax on fp32 scores = scores.argmax(1) on the CPU: NaN among finite scores (also in a column >= 64, which a lane
    meets on its second trip), +inf twice, all -inf, signed zeros, ties; on a column slice of a wider matrix, with and without the
    gather."""
    from openscene_amd import ops
    s = qb.rows_argmax_scores(n, c)
    wide = torch.full((n, c + 3), float("inf"))
    wide[:, :c] = s
    sg = wide.to(dev())[:, :c]
    want = s.argmax(1)
    assert torch.equal(ops.rows_argmax(sg).cpu(), want)
    g = torch.Generator().manual_seed(n + c)
    idx = torch.randint(0, n, (2 * n + 1,), generator=g)
    idx[:n] = torch.arange(n)
    assert torch.equal(ops.rows_argmax(sg, idx.to(dev())).cpu(), want[idx])
