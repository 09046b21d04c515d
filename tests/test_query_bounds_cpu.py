"""What gives tests/test_gpu_query_bounds.py its teeth, checked without a GPU (the contract: tests/query_bounds.py).

Scores: the CPU emulation of the query kernels -- fp16 operands, exact products, fp32 accumulation in ascending k, one fp16
rounding -- meets the score interval on every operand kind; six subtly wrong variants of it each put scores outside the interval on
the operand kind named in CAUGHT_BY.  Labels: on the planted rows "a NaN never wins" and "the raw fp16 bit order" both differ from
torch.max, the numpy restatement of the rule does not.  The conditions on the INPUTS that the GPU module relies on are asserted here
with the reference alone: at most 5 % of the rows are undecided against float64 for "unit" and "row_scales"; in the ensemble both
sources win for 15 - 85 % of the points and at most 5 % are undecided; query_bounds.DELTA is four times the measured error of the
fp32 quotient x / (||x|| + 1e-5), in both summation orders."""
import numpy as np
import pytest
import torch

import query_bounds as qb

SHAPES = [(129, 72, 33), (300, 520, 161), (300, 768, 160)]          # (feature rows, d, c)


def emulate(x, t, drop=None, operands="fp16", acc="fp32", x_round="rne", out_round="rne"):
    """fp16 scores [n, c] of fp32 features x against fp16 text t: the kernels' arithmetic on the CPU, or a broken variant of it.
    drop: a range of k left out; operands "bf16": both operands rounded to bf16 first; acc "fp16": the accumulator rounded to fp16
    after every step; x_round / out_round "trunc": the conversion of x / of the result to fp16 by truncation."""
    xf, tf = x.float(), t.float()
    if operands == "bf16":
        xf, tf = xf.bfloat16().float(), tf.bfloat16().float()
    xh = to_fp16(xf.double().numpy(), x_round).astype(np.float64)
    th = tf.double().numpy()
    acc_t = np.float32 if acc == "fp32" else np.float16
    a = np.zeros((x.shape[0], t.shape[0]), dtype=acc_t)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(x.shape[1]):
            if drop is not None and k in drop:
                continue
            a = (a.astype(np.float64) + xh[:, k, None] * th[None, :, k]).astype(acc_t)      # (an fp16 x fp16 product is exact)
        return to_fp16(a.astype(np.float64), out_round)


def to_fp16(a, mode):
    """float64 -> fp16, round to nearest even or truncated towards zero (overflow past 65504: inf either way)."""
    h = qb.fp16_rne(a)
    if mode == "rne":
        return h
    assert mode == "trunc"
    with np.errstate(invalid="ignore"):
        away = np.isfinite(h) & (np.abs(h.astype(np.float64)) > np.abs(a))
    return np.where(away, np.nextafter(h, np.float16(0)), h)


@pytest.mark.parametrize("n,d,c", SHAPES)
@pytest.mark.parametrize("kind", qb.KINDS)
def test_fp32_chain_meets_the_score_contract(kind, n, d, c):
    x, t = qb.operands(kind, n, d, c)
    ref = qb.reference(kind, n, d, c)
    qb.within(emulate(x, t), ref, label="chain %s %s" % (kind, (n, d, c)))
    # the planted rows give what the module docstring says
    s = qb.fp16_rne(ref.S).astype(np.float64)
    P = qb.PLANTED
    assert np.isnan(s[P["nan"]]).all() and np.isnan(s[P["nan_among"], 2]) and np.isnan(s[P["nan_among"]]).sum() == 1
    assert s[P["nan_among"], 0] == -np.inf and s[P["nan_among"], 1] == np.inf
    assert s[P["inf_two"], 0] == -np.inf and (s[P["inf_two"], 1:] == np.inf).all()
    assert (s[P["all_neg_inf"]] == -np.inf).all()
    assert (s[P["signed_zeros"]] == 0).all() and np.signbit(s[P["signed_zeros"], ::2]).all() and not np.signbit(s[P["signed_zeros"], 1::2]).any()
    assert (s[P["zero"]] == 0).all() and not np.signbit(s[P["zero"]]).any()
    assert (s[:, 3] == s[:, 1])[~np.isnan(s[:, 1])].all()
    if d >= 520:
        assert (s[P["pos3000"], 0] == np.inf).all() and (s[P["neg3000"], 0] == -np.inf).all()


# broken variant -> (emulate arguments, the operand kind that catches it, the shape)
CAUGHT_BY = {
    "ragged_tail_dropped": (dict(drop=range(64, 72)), "unit", (129, 72, 33)),
    "k_step_dropped": (dict(drop=range(16, 32)), "unit", (300, 768, 160)),
    "operands_through_bf16": (dict(operands="bf16"), "half_ties", (300, 768, 160)),
    "fp16_accumulation": (dict(acc="fp16"), "coherent", (300, 768, 160)),
    "x_truncated": (dict(x_round="trunc"), "half_ties", (300, 520, 161)),
    "result_truncated": (dict(out_round="trunc"), "cancellation", (300, 520, 161)),
}


@pytest.mark.parametrize("name", sorted(CAUGHT_BY))
def test_broken_emulation_is_caught(name):
    args, kind, (n, d, c) = CAUGHT_BY[name]
    x, t = qb.operands(kind, n, d, c)
    ratio, n_bad = qb.worst_ratio(emulate(x, t, **args), qb.reference(kind, n, d, c))
    print("%s on %s: %d outside, worst ratio %.2f" % (name, kind, n_bad, ratio))
    assert n_bad >= 1 and ratio > 1


def test_label_rules_on_the_planted_rows():
    n, d, c = 129, 72, 33
    ref = qb.reference("unit", n, d, c)
    scores = torch.from_numpy(qb.fp16_rne(ref.S))
    want = qb.torch_max_labels(scores)
    assert torch.equal(want, torch.max(scores.float(), 1)[1])                  # (the fp16 and the fp32 path of torch agree)
    assert torch.equal(qb.rule_labels(scores, "torch_max"), want)
    P = qb.PLANTED
    assert int(want[P["nan_among"]]) == 2 and int(want[P["inf_two"]]) == 1 and int(want[P["all_neg_inf"]]) == 0
    assert int(want[P["signed_zeros"]]) == 0 and int(want[P["zero"]]) == 0 and not want[P["nan"]].any()
    planted = slice(0, qb.N_PLANTED)
    assert not torch.equal(qb.rule_labels(scores, "nan_never_wins")[planted], want[planted])
    assert not torch.equal(qb.rule_labels(scores, "raw_bits")[planted], want[planted])
    # a negative NaN, which the raw bit order puts below -inf
    neg = scores.clone()
    neg[P["nan_among"], 2] = torch.tensor(np.array([0xFE00], dtype=np.uint16).view(np.float16))[0]
    assert int(qb.torch_max_labels(neg)[P["nan_among"]]) == 2 and int(qb.rule_labels(neg, "raw_bits")[P["nan_among"]]) != 2
    # the rows handed to ops.rows_argmax
    s = qb.rows_argmax_scores(40, 97)
    assert torch.equal(qb.rule_labels(s, "torch_max"), s.argmax(1)) and torch.equal(s.argmax(1), torch.max(s, 1)[1])
    assert not torch.equal(qb.rule_labels(s, "nan_never_wins"), s.argmax(1))


@pytest.mark.parametrize("n,d,c", SHAPES)
@pytest.mark.parametrize("kind", ["unit", "row_scales"])
def test_few_rows_are_undecided_against_float64(kind, n, d, c):
    ref = qb.reference(kind, n, d, c)
    w, dec = qb.decided(ref)
    share = 1.0 - dec[qb.N_PLANTED:].mean()
    print("%s %s: %.1f %% of the ordinary rows undecided" % (kind, (n, d, c), 100 * share))
    assert 1.0 - dec.mean() <= 0.05 + qb.N_PLANTED / dec.shape[0] and share <= 0.05
    # the emulation's labels obey both label clauses
    x, t = qb.operands(kind, n, d, c)
    got = qb.torch_max_labels(torch.from_numpy(emulate(x, t)))
    assert np.array_equal(got.numpy()[dec], w[dec])


@pytest.mark.parametrize("n,n_vox,d,c", qb.ENSEMBLE_SHAPES)
def test_ensemble_inputs_and_delta(n, n_vox, d, c):
    ens = qb.ensemble_case(n, n_vox, d, c)
    share = ens.sel.mean()
    print("fusion wins %.1f %%, undecided %.1f %%" % (100 * share, 100 * (1 - ens.decided.mean())))
    assert 0.15 <= share <= 0.85 and 1 - ens.decided.mean() <= 0.05
    assert not ens.sel[0] and not torch.equal(ens.gd, ens.gf)
    worst = 0.0
    for x in (ens.xd, ens.xf):
        for order in ("ascending", "lanes"):
            e = qb.quotient_error(x.numpy(), order)
            print("d = %d %s: quotient error %.3e" % (d, order, e))
            worst = max(worst, e)
    assert 4 * worst <= qb.DELTA
    # the reference's own normalised fp16 features lie inside the element interval, and its scores inside the score interval
    tn = ens.text.double().numpy()
    for f in (ens.xd[ens.gd], ens.xf[ens.gf]):
        r = qb.normalised_interval(f.numpy(), tn)
        q32 = (f / (f.norm(dim=-1, keepdim=True) + 1e-5)).half()
        got = (q32.float() @ ens.text.float().t()).half()
        assert not qb.outside(got, r).any()
