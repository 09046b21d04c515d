"""The matching contract on the CPU (tests/match_reference.py): the checker the GPU test applies to csrc/match.hip is first
shown to accept a correct evaluation -- an fp32 chain in ascending d -- on every case, and to catch each of six wrong
"kernels"; the share of undecided rows is held at or below 5 % on every bound case, so that "idx equals the reference's on
decided rows" is a condition on almost every row; the planted scenes give the label-transfer accuracy the GPU test must meet."""
import pytest
import torch

import gram_reference as gr
import match_reference as mr


def test_the_constant_is_the_projects_forward_bound():
    import conv_bounds
    assert mr.C == conv_bounds.FWD_C == 2e-6


@pytest.mark.parametrize("d", mr.DIMS_FP16)
def test_an_fp32_chain_meets_the_conditions_and_few_rows_are_undecided(d):
    for m in mr.MS:
        xq, xe = mr.rows_case(d, m)
        a16, b16 = mr.operands_cpu(xq), mr.operands_cpu(xe)
        s, a = mr.scores(mr.operands_f64(a16), mr.operands_f64(b16))
        idx, score, count = mr.match_chain(a16, b16, mr.K)
        worst, undecided = mr.check(idx, score, count, s, a, mr.K, label="d=%d M=%d" % (d, m))
        print("d=%d M=%d: worst err / limit %.3f, undecided rows %.4f" % (d, m, worst, undecided))
        assert undecided <= mr.UNDECIDED_MAX


@pytest.mark.parametrize("d", (16, 528))
def test_the_fp8_dims_hold_the_same(d):
    xq, xe = mr.rows_case(d, 700)
    a16, b16 = mr.operands_cpu(xq), mr.operands_cpu(xe)
    s, a = mr.scores(mr.operands_f64(a16), mr.operands_f64(b16))
    _, undecided = mr.check(*mr.match_chain(a16, b16, mr.K), s, a, mr.K)
    assert undecided <= mr.UNDECIDED_MAX


def _case_with_ties(d=520, m=700):
    xq, xe = mr.rows_case(d, m)
    xe = xe.clone()
    xe[5::7] = xe[3::7][:xe[5::7].shape[0]]                  # duplicated exemplars: exact ties in every row
    return xq, xe


@pytest.mark.parametrize("wrong", mr.WRONG)
def test_each_wrong_kernel_is_caught(wrong):
    xq, xe = _case_with_ties()
    a16, b16 = mr.operands_cpu(xq), mr.operands_cpu(xe)
    s, a = mr.scores(mr.operands_f64(a16), mr.operands_f64(b16))
    mr.check(*mr.match_chain(a16, b16, mr.K), s, a, mr.K)                       # the right one passes on the very same inputs
    with pytest.raises(AssertionError):
        mr.check(*mr.match_chain(a16, b16, mr.K, wrong=wrong, raw_b=xe), s, a, mr.K)


def test_ties_and_positions_are_caught_exactly_on_integers():
    xa, xb = mr.integer_case(24, 129)
    for k in (1, 8):
        idx, score, count = mr.match_chain(xa.half(), xb.half(), k)
        mr.check_exact(idx, score, count, xa, xb, k)
        for wrong in ("ties_to_higher", "off_by_one"):
            with pytest.raises(AssertionError):
                mr.check_exact(*mr.match_chain(xa.half(), xb.half(), k, wrong=wrong), xa, xb, k)


def test_fewer_exemplars_than_k_pad_the_lists():
    xq, xe = mr.rows_case(24, 9)
    a16, b16 = mr.operands_cpu(xq), mr.operands_cpu(xe[:5])
    idx, score, count = mr.match_chain(a16, b16, 8)
    s, a = mr.scores(mr.operands_f64(a16), mr.operands_f64(b16))
    mr.check(idx, score, count, s, a, 8)
    assert bool((count == 5).all()) and bool((idx[:, 5:] == -1).all())


def test_label_transfer_on_the_planted_scenes_reaches_the_accuracy_the_device_must_meet():
    p = gr.planted()
    b = mr.operands_f64(mr.operands_cpu(p["feats"][0]))
    for scene in (1, 2):
        a = mr.operands_f64(mr.operands_cpu(p["feats"][scene]))
        labels, sure = mr.planted_reference(a, b, p["cls"][0])
        accuracy = float((labels == p["cls"][scene]).double().mean())
        print("scene %d: accuracy %.4f, decided rows %.4f" % (scene, accuracy, float(sure.double().mean())))
        assert accuracy >= mr.PLANT_ACCURACY


def test_vote_takes_the_most_similar_holder_on_a_tie():
    labels = torch.tensor([4, 7, 7, 4, -1, 9])
    idx = torch.tensor([[0, 1, 2, 3], [5, 4, -1, -1], [4, -1, -1, -1], [1, 0, 3, 2]], dtype=torch.int32)
    count = torch.tensor([4, 2, 1, 4], dtype=torch.int32)
    assert mr.vote(labels, idx, count).tolist() == [4, 9, -1, 7]
