"""Generate tests/golden/eval_metric.npz by running the REFERENCE's own util/metric.py:evaluate (and the `store = pred +
store` test-repeat vote of run/evaluate.py:397-424 on CPU fp16 tensors).

Run in the authoring container only (needs /root/reference):
    python tests/golden/make_golden_eval.py           # write the fixture
    python tests/golden/make_golden_eval.py --check   # re-run the reference and compare with the fixture
evaluate returns only the mean IoU; its class_ious / class_accs / mean_acc are read from its frame when it returns (the
reference's own values, not a re-computation).  The fixture also keeps the class name lists of
dataset/label_constants.py that the cases use, so the tests need nothing from the reference.
"""
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, "/root/reference")

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "eval_metric.npz")


def reference():
    from util import metric                       # noqa: E402  (the reference's module, imported as it is)
    from dataset import label_constants as L
    return metric, L


def run_evaluate(metric, pred, gt, dataset):
    """-> (mean_iou, mean_acc, class_ious, class_accs, stdout, error): evaluate(stdout=True) on copies of the arrays."""
    captured = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code is metric.evaluate.__code__:
            captured.update({k: frame.f_locals.get(k) for k in ("class_ious", "class_accs", "mean_acc")})
    buf = io.StringIO()
    err = ""
    mean_iou = None
    sys.setprofile(prof)
    try:
        with contextlib.redirect_stdout(buf):
            mean_iou = metric.evaluate(pred.copy(), gt.copy(), stdout=True, dataset=dataset)
    except Exception as e:                        # the reference's failure on an all-no-feature class
        err = "%s: %s" % (type(e).__name__, e)
    finally:
        sys.setprofile(None)
    return mean_iou, captured.get("mean_acc"), captured.get("class_ious"), captured.get("class_accs"), buf.getvalue(), err


def cases(L):
    """(tag, dataset, class-name list key, pred ids (after mapper / no-feature), gt ids, pre-mapper ids or None)."""
    rng = np.random.default_rng(2024)
    out = []

    def noisy(gt, c, p_right):
        pred = np.where(rng.random(gt.size) < p_right, gt, rng.integers(0, c, gt.size))
        pred[gt == 255] = rng.integers(0, c, int((gt == 255).sum()))
        return pred.astype(np.int64)

    # ScanNet-20: classes 3, 11 absent from the gt (one of them still predicted), gt 255 sprinkled
    n = 4000
    gt = rng.integers(0, 20, n)
    gt[np.isin(gt, (3, 11))] = 0
    gt[rng.random(n) < 0.07] = 255
    out.append(("scannet", "scannet_3d", "SCANNET_LABELS_20", noisy(gt, 20, 0.6), gt.astype(np.int64), None))
    # ScanNet with no-feature points (fusion + mark_no_feature_to_unknown: pred 256)
    pred = noisy(gt, 20, 0.6)
    pred[rng.random(n) < 0.15] = 256
    out.append(("scannet_nofeat", "scannet_3d", "SCANNET_LABELS_20", pred, gt.astype(np.int64), None))
    # Matterport-21 (accuracy-only table), with no-feature points and an absent class
    gt = rng.integers(0, 21, 3000)
    gt[gt == 7] = 1
    gt[rng.random(3000) < 0.05] = 255
    pred = noisy(gt, 21, 0.5)
    pred[rng.random(3000) < 0.1] = 256
    out.append(("matterport21", "matterport_3d", "MATTERPORT_LABELS_21", pred, gt.astype(np.int64), None))
    # Matterport-160: many absent classes
    gt = rng.integers(0, 160, 5000)
    gt[(gt % 7) == 3] = 255
    out.append(("matterport160", "matterport_3d_160", "MATTERPORT_LABELS_160", noisy(gt, 160, 0.4), gt.astype(np.int64), None))
    # nuScenes: 43 detailed labels -> 16 through MAPPING_NUSCENES_DETAILS (label_mask: only gt != 255 points are kept)
    mapper = np.asarray(L.MAPPING_NUSCENES_DETAILS, dtype=np.int64)
    gt = rng.integers(0, 16, 3500)
    p43 = rng.integers(0, 43, 3500)
    right = rng.random(3500) < 0.55
    inv = {int(v): k for k, v in enumerate(mapper)}
    p43[right] = [inv[int(g)] for g in gt[right]]
    out.append(("nuscenes", "nuscenes_3d", "NUSCENES_LABELS_16", mapper[p43], gt.astype(np.int64), p43.astype(np.int64)))
    # a class whose gt points all lack a feature: get_iou returns a bare nan and evaluate fails on indexing it
    gt = rng.integers(0, 20, 1500)
    pred = noisy(gt, 20, 0.6)
    pred[pred == 5] = 4
    pred[gt == 5] = 256
    out.append(("all_nofeat", "scannet_3d", "SCANNET_LABELS_20", pred, gt.astype(np.int64), None))
    return out


def repeat_scores(rng, n=600, c=20, reps=5):
    """fp16 score matrices of five repeats built for the vote's corner cases: exact ties, -0.0, sums that saturate to
    +-inf, NaN, and values whose fp16 sum needs rounding."""
    import torch
    out = []
    for r in range(reps):
        s = (rng.standard_normal((n, c)) * 0.3).astype(np.float16)
        s[0:40, 3] = s[0:40, 7] = s[0:40, 1]                          # ties inside a repeat
        s[40:60, :] = -0.0                                             # -0.0 (+ 0.0 start: +0.0)
        s[60:70, 2] = np.float16(40000.0)                              # 40000 * 2 saturates to inf
        s[70:80, 4] = np.float16(-40000.0)
        s[80:85, 5] = np.float16(np.nan) if r in (1, 3) else np.float16(0.5)
        s[85:90, 6] = np.float16(60000.0) if r == 0 else np.float16(-60000.0)   # inf + (-inf) = NaN later
        s[90:100, :] = np.float16(2048.0) if r == 0 else np.float16(1.0)        # 2048 + 1 -> 2048 (RNE)
        s[100:110, 8] = np.float16(0.1) * (r + 1)                      # rounding of the sum
        s[100:110, 9] = np.float16(0.1) * (r + 1)
        out.append(torch.from_numpy(s))
    return out


def generate():
    import torch
    metric, L = reference()
    rec = {}
    names_used = set()
    for tag, dataset, names, pred, gt, p43 in cases(L):
        mean_iou, mean_acc, class_ious, class_accs, text, err = run_evaluate(metric, pred, gt, dataset)
        names_used.add(names)
        rec[tag + "_dataset"] = np.asarray(dataset)
        rec[tag + "_names"] = np.asarray(names)
        rec[tag + "_pred"] = pred.astype(np.int16)
        rec[tag + "_gt"] = gt.astype(np.int16)
        if p43 is not None:
            rec[tag + "_pred_premap"] = p43.astype(np.int16)
        rec[tag + "_stdout"] = np.asarray(text)
        rec[tag + "_error"] = np.asarray(err)
        if not err:
            rec[tag + "_mean_iou"] = np.float64(mean_iou)
            rec[tag + "_mean_acc"] = np.float64(mean_acc)
            keys = list(class_ious)
            rec[tag + "_class_names"] = np.asarray(keys)
            rec[tag + "_iou"] = np.asarray([class_ious[k][0] for k in keys], dtype=np.float64)
            rec[tag + "_tp"] = np.asarray([class_ious[k][1] for k in keys], dtype=np.int64)
            rec[tag + "_denom"] = np.asarray([class_ious[k][2] for k in keys], dtype=np.int64)
            rec[tag + "_acc"] = np.asarray([class_accs[k] for k in keys], dtype=np.float64)
    for names in sorted(names_used):
        rec["labels_" + names] = np.asarray(getattr(L, names))
    rec["mapping_nuscenes_details"] = np.asarray(L.MAPPING_NUSCENES_DETAILS, dtype=np.int64)
    # five-repeat vote on CPU fp16 tensors: store = pred + store; store.float().max(1)[1]; evaluate
    rng = np.random.default_rng(77)
    scores = repeat_scores(rng)
    n = scores[0].shape[0]
    gt = rng.integers(0, 20, n)
    gt[rng.random(n) < 0.05] = 255
    rec["votes_scores"] = np.stack([s.numpy() for s in scores]).view(np.uint16)
    rec["votes_gt"] = gt.astype(np.int16)
    store = 0.0
    stores, logits, mious, texts = [], [], [], []
    for s in scores:
        store = s + store
        store_logit = store.float().max(1)[1]
        m, _, _, _, text, err = run_evaluate(metric, store_logit.numpy(), gt.astype(np.int64), "scannet_3d")
        assert not err, err
        stores.append(store.numpy().view(np.uint16).copy())
        logits.append(store_logit.numpy().astype(np.int16))
        mious.append(m)
        texts.append(text)
    rec["votes_store"] = np.stack(stores)
    rec["votes_logit"] = np.stack(logits)
    rec["votes_mean_iou"] = np.asarray(mious, dtype=np.float64)
    rec["votes_stdout"] = np.asarray(texts)
    return rec


def main():
    rec = generate()
    if "--check" in sys.argv:
        old = np.load(OUT)
        bad = [k for k in rec if k not in old.files or not np.array_equal(old[k], rec[k], equal_nan=rec[k].dtype.kind == "f")]
        bad += [k for k in old.files if k not in rec]
        if bad:
            print("MISMATCH:", bad)
            sys.exit(1)
        print("ok: %s matches the reference (%d arrays)" % (os.path.basename(OUT), len(rec)))
        return
    np.savez_compressed(OUT, **rec)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
