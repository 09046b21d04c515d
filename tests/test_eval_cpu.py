"""Host side of the open-vocabulary evaluation (no GPU): metrics.evaluate_confusion against the reference's own
util/metric.py:evaluate (tests/golden/eval_metric.npz, made by make_golden_eval.py), argument validation, the rounding
contract of the vote, and the slot bookkeeping of OpenVocabEvaluator."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from openscene_amd import metrics

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metric.npz")
TAGS = ("scannet", "scannet_nofeat", "matterport21", "matterport160", "nuscenes", "all_nofeat")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def host_confusion(pred, gt, c):
    """(c + 1) x c [pred, gt]: util/metric.py:confusion_matrix plus the row of no-feature (256) points; gt 255 ignored."""
    pred = np.asarray(pred, dtype=np.int64).copy()
    gt = np.asarray(gt, dtype=np.int64)
    keep = gt != 255
    pred[pred == 256] = c
    return np.bincount(pred[keep] * c + gt[keep], minlength=(c + 1) * c).reshape(c + 1, c).astype(np.int64)


def case(gold, tag):
    names = [str(x) for x in gold["labels_" + str(gold[tag + "_names"])]]
    return names, str(gold[tag + "_dataset"]), gold[tag + "_pred"].astype(np.int64), gold[tag + "_gt"].astype(np.int64)


def run(conf, names, dataset, n_points):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = metrics.evaluate_confusion(conf, names, dataset, stdout=True, n_points=n_points)
    return res, buf.getvalue()


@pytest.mark.parametrize("tag", [t for t in TAGS if t != "all_nofeat"])
def test_evaluate_confusion_matches_reference(gold, tag):
    names, dataset, pred, gt = case(gold, tag)
    res, text = run(host_confusion(pred, gt, len(names)), names, dataset, gt.size)
    assert type(res.mean_iou) is np.float64 and res.mean_iou == gold[tag + "_mean_iou"]
    assert res.mean_acc == gold[tag + "_mean_acc"]
    assert res[0] == res.mean_iou
    keys = [str(k) for k in gold[tag + "_class_names"]]
    assert list(res.class_ious) == keys and list(res.class_accs) == keys
    for k, iou, tp, den, acc in zip(keys, gold[tag + "_iou"], gold[tag + "_tp"], gold[tag + "_denom"], gold[tag + "_acc"]):
        assert res.class_ious[k] == (iou, tp, den)
        assert res.class_accs[k] == acc
    assert text == str(gold[tag + "_stdout"])


def test_plain_matrix_of_segmentation_meter(gold):
    # run/eval_mink.py: SegmentationMeter.matrix() is C x C (no no-feature row); same numbers when no point lacks a feature
    names, dataset, pred, gt = case(gold, "scannet")
    conf = host_confusion(pred, gt, len(names))
    assert not conf[-1].any()
    a = metrics.evaluate_confusion(conf, names, dataset)
    b = metrics.evaluate_confusion(conf[:-1].copy(), names, dataset)
    assert a.mean_iou == b.mean_iou == gold["scannet_mean_iou"] and a.class_ious == b.class_ious
    assert metrics.evaluate_confusion(torch.from_numpy(conf[:-1].copy()), names, dataset).mean_iou == a.mean_iou


def test_nuscenes_mapper_replay(gold):
    mapper = gold["mapping_nuscenes_details"]
    assert np.array_equal(mapper[gold["nuscenes_pred_premap"].astype(np.int64)], gold["nuscenes_pred"])


def test_all_no_feature_class_fails_like_reference(gold):
    names, dataset, pred, gt = case(gold, "all_nofeat")
    want = str(gold["all_nofeat_error"])
    buf = io.StringIO()
    with pytest.raises(TypeError) as ei, contextlib.redirect_stdout(buf):
        metrics.evaluate_confusion(host_confusion(pred, gt, len(names)), names, dataset, stdout=True, n_points=gt.size)
    assert "TypeError: %s" % ei.value == want
    assert buf.getvalue() == str(gold["all_nofeat_stdout"])


def test_default_point_count_is_matrix_sum(gold):
    names, dataset, pred, gt = case(gold, "nuscenes")
    _, text = run(host_confusion(pred, gt, len(names)), names, dataset, None)
    assert text.splitlines()[0] == "evaluating %d points..." % int((gt != 255).sum())


def test_vote_rounding_contract(gold):
    # store = pred + store on CPU half tensors == fp32 add of the two halves, rounded once (round to nearest even)
    scores = gold["votes_scores"].view(np.float16)
    store = np.zeros_like(scores[0])
    for r in range(scores.shape[0]):
        with np.errstate(over="ignore"):
            store = (store.astype(np.float32) + scores[r].astype(np.float32)).astype(np.float16)
        ref = gold["votes_store"][r]
        got = store.view(np.uint16)
        nan = np.isnan(store)
        assert np.array_equal(nan, np.isnan(ref.view(np.float16)))
        assert np.array_equal(got[~nan], ref[~nan])
        # the argmax rule of store.float().max(1)[1]: first NaN, else the first of equal maxima
        f = store.astype(np.float32)
        want = np.where(nan.any(1), nan.argmax(1), np.nanargmax(np.where(nan, -np.inf, f), 1))
        assert np.array_equal(want, gold["votes_logit"][r])
    assert np.isinf(store).any() and np.isnan(store).any()


def test_evaluate_confusion_arguments():
    names = ["a", "b", "c"]
    ok = np.zeros((4, 3), dtype=np.int64)
    ok[0, 0] = 1
    with pytest.raises(ValueError):
        metrics.evaluate_confusion(np.zeros((5, 3), dtype=np.int64), names, "scannet_3d")
    with pytest.raises(ValueError):
        metrics.evaluate_confusion(np.zeros((4, 4), dtype=np.int64), names, "scannet_3d")
    with pytest.raises(ValueError):
        metrics.evaluate_confusion(ok.astype(np.float64), names, "scannet_3d")
    with pytest.raises(ValueError):
        metrics.evaluate_confusion(-ok, names, "scannet_3d")
    with pytest.raises(TypeError):
        metrics.evaluate_confusion(ok, "abc", "scannet_3d")
    with pytest.raises(TypeError):
        metrics.evaluate_confusion(ok, names, None)
    res = metrics.evaluate_confusion(ok, names, "scannet_3d")
    assert res.mean_iou == 1.0 / 3 and res.class_ious == {"a": (1.0, 1, 1)}
    empty = metrics.evaluate_confusion(np.zeros((4, 3), dtype=np.int64), names, "scannet_3d")
    assert empty.mean_iou == 0 and empty.class_ious == {}


def test_evaluator_arguments():
    names = ["c%d" % i for i in range(16)]
    with pytest.raises(ValueError):
        metrics.OpenVocabEvaluator(0, names, "scannet_3d", 1, device="cpu")
    with pytest.raises(ValueError):
        metrics.OpenVocabEvaluator(16, names, "scannet_3d", 0, device="cpu")
    with pytest.raises(TypeError):
        metrics.OpenVocabEvaluator(16, [], "scannet_3d", 1, device="cpu")
    with pytest.raises(ValueError):              # 43 labels for 16 classes without a mapper
        metrics.OpenVocabEvaluator(43, names, "nuscenes_3d", 5, device="cpu")
    ev = metrics.OpenVocabEvaluator(43, names, "nuscenes_3d", 5, mapper=list(range(16)) * 3, device="cpu")
    assert ev.mapper.dtype == torch.int64 and ev.mapper.numel() == 48
    assert tuple(ev.confusion.shape) == (17, 16)


def test_evaluator_slot_bookkeeping():
    # the vote itself is torch's add_ here (add_scores), so the bookkeeping runs on the CPU; counting needs the GPU
    ev = metrics.OpenVocabEvaluator(4, ["a", "b", "c", "d"], "scannet_3d", 3, device="cpu")
    sizes = (5, 0, 7, 3)
    with pytest.raises(RuntimeError):
        ev.add_scores(torch.zeros(5, 4, dtype=torch.float16), torch.zeros(5, dtype=torch.int64))
    ev.begin_repeat()
    preds = [torch.randn(n, 4).half() for n in sizes]
    for p, n in zip(preds, sizes):
        ev.add_scores(p, torch.zeros(n, dtype=torch.int64))
    assert ev.slots == [(0, 5), (5, 0), (5, 7), (12, 3)]
    with pytest.raises(ValueError):
        ev.add_scores(torch.zeros(2, 3, dtype=torch.float16), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        ev.add_scores(torch.zeros(2, 4, dtype=torch.float16), torch.zeros(3, dtype=torch.int64))
    # what end_repeat does before it counts: the first repeat's scenes become one matrix
    ev._chunks, chunks = None, ev._chunks
    ev.votes = torch.cat([c[0] for c in chunks])
    ev.labels = torch.cat([c[1] for c in chunks])
    ev._scene = -1
    assert torch.equal(ev.votes, torch.cat(preds) + 0.0)
    ev.begin_repeat()
    ev.add_scores(preds[0], torch.ones(5, dtype=torch.int64))
    assert torch.equal(ev.votes[:5], preds[0] + preds[0])
    assert torch.equal(ev.labels[:5], torch.ones(5, dtype=torch.int64))
    with pytest.raises(ValueError):              # slot 1 holds 0 points
        ev.add_scores(preds[2], torch.zeros(7, dtype=torch.int64))
    ev.add_scores(preds[1], torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError):              # a repeat that ends early
        ev.end_repeat()
    for p, n in zip(preds[2:], sizes[2:]):
        ev.add_scores(p, torch.zeros(n, dtype=torch.int64))
    with pytest.raises(ValueError):              # a fifth scene
        ev.add_scores(preds[3], torch.zeros(3, dtype=torch.int64))
    ev._scene = -1
    ev.begin_repeat()
    with pytest.raises(RuntimeError):            # test_repeats = 3
        ev.begin_repeat()


def test_evaluator_mask_required_with_mark_no_feature():
    ev = metrics.OpenVocabEvaluator(4, ["a", "b", "c", "d"], "scannet_3d", 2, mark_no_feature=True, device="cpu")
    ev.begin_repeat()
    with pytest.raises(ValueError):
        ev.add_scores(torch.zeros(3, 4, dtype=torch.float16), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        ev.add_scores(torch.zeros(3, 4, dtype=torch.float16), torch.zeros(3, dtype=torch.int64), mask=torch.ones(2, dtype=torch.bool))
    ev.add_scores(torch.zeros(3, 4, dtype=torch.float16), torch.zeros(3, dtype=torch.int64), mask=torch.ones(3, dtype=torch.bool))
    assert ev.slots == [(0, 3)]
