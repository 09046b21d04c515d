"""Segmentation metrics of the supervised baseline on the device.

The reference computes them per iteration with intersectionAndUnionGPU (util/util.py:132-145: three host copies and a CPU
histc, run/train_mink.py:285-297 / 370-379) and at evaluation with a numpy confusion matrix (util/metric.py:9-25).
``SegmentationMeter`` keeps ONE int64 confusion matrix on the device, ``confusion[pred, label]``; every vector of the
reference is a sum over it:

    intersection = diag,   output = row sums,   target = column sums,   union = output + target - intersection

``update`` (or ``segmentation_loss(..., meter=meter)``, which counts inside the loss's own pass) never synchronises the host;
reading a result copies the matrix to the host once."""
import numpy as np
import torch

from . import ops


class SegmentationMeter:
    def __init__(self, num_classes, ignore_index=255, device=None):
        if not 1 <= int(num_classes) <= 256:
            raise ValueError("num_classes=%r: the kernels take 1 to 256 classes" % (num_classes,))
        self.num_classes = int(num_classes)
        self.ignore_index = int(ignore_index)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.confusion = torch.zeros((self.num_classes, self.num_classes), dtype=torch.int64, device=dev)

    def reset(self):
        self.confusion.zero_()

    def update(self, logits, labels, rows=None, validate=False):
        """Count (argmax of logits[rows], label) over the labelled rows (rows: ``inds_reverse``, None = every row)."""
        ops.seg_loss_fwd(logits, labels, self.ignore_index, rows=rows, want_loss=False, confusion=self.confusion, validate=validate)

    def matrix(self):
        """The confusion matrix on the host (int64 [pred, label]): util/metric.py's confusion_matrix summed over the updates."""
        return self.confusion.cpu().numpy()

    @staticmethod
    def _vectors(conf):
        inter = np.diag(conf).copy()
        output = conf.sum(axis=1)
        target = conf.sum(axis=0)
        return inter, output + target - inter, target

    def intersection_union_target(self):
        """(intersection, union, target), int64 [C] each: the sums over every update of intersectionAndUnionGPU's vectors."""
        return self._vectors(self.matrix())

    def iou(self):
        inter, union, _ = self.intersection_union_target()
        return inter / (union + 1e-10)

    def miou(self):
        return float(np.mean(self.iou()))

    def macc(self):
        inter, _, target = self.intersection_union_target()
        return float(np.mean(inter / (target + 1e-10)))

    def allacc(self):
        inter, _, target = self.intersection_union_target()
        return float(sum(inter) / (sum(target) + 1e-10))

    def summary(self):
        """{'miou', 'macc', 'allacc', 'iou'} from one host copy (run/train_mink.py:337-341, 385-389)."""
        inter, union, target = self._vectors(self.matrix())
        iou = inter / (union + 1e-10)
        return {"miou": float(np.mean(iou)), "macc": float(np.mean(inter / (target + 1e-10))),
                "allacc": float(sum(inter) / (sum(target) + 1e-10)), "iou": iou}


# ------------------------------------------------------------------------------------- open-vocabulary evaluation
NO_FEATURE_ID = 256      # util/metric.py: a point without a fused 2-D feature (mark_no_feature_to_unknown)


class EvalResult(tuple):
    """(mean_iou, mean_acc, class_ious, class_accs) of util/metric.py:evaluate.  mean_iou is what evaluate returns;
    class_ious[name] = (iou, tp, tp + fp + fn) and class_accs[name] = tp / #gt for every class present in the gt."""
    __slots__ = ()

    def __new__(cls, mean_iou, mean_acc, class_ious, class_accs):
        return tuple.__new__(cls, (mean_iou, mean_acc, class_ious, class_accs))

    mean_iou = property(lambda self: self[0])
    mean_acc = property(lambda self: self[1])
    class_ious = property(lambda self: self[2])
    class_accs = property(lambda self: self[3])


def _get_iou(label_id, confusion):
    # util/metric.py:get_iou, the same numpy types and the same bare nan when nothing is counted
    tp = np.longlong(confusion[label_id, label_id])
    fp = np.longlong(confusion[label_id, :].sum()) - tp
    fn = np.longlong(confusion[:, label_id].sum()) - tp
    denom = (tp + fp + fn)
    if denom == 0:
        return float('nan')
    return float(tp) / denom, tp, denom


def evaluate_confusion(conf, class_labels, dataset, stdout=False, n_points=None):
    """util/metric.py:evaluate from a confusion matrix [pred, gt] instead of the per-point arrays.

    conf: (C + 1) x C (row C = the no-feature points of each gt class, eval_confusion / OpenVocabEvaluator) or C x C
    (SegmentationMeter.matrix()); numpy or a tensor.  class_labels: the C names the caller's dataset.label_constants
    gives evaluate for `dataset` (SCANNET_LABELS_20, MATTERPORT_LABELS_21/40/80/160, NUSCENES_LABELS_16); `dataset` only
    picks the printed form ('matterport' in it: accuracy only).  n_points: the count of the 'evaluating N points...'
    line (gt_ids.size, ignored points included); default: the points the matrix counts.
    Returns EvalResult(mean_iou, mean_acc, class_ious, class_accs) with evaluate's values and types: the means are
    summed in class order and divided by C (absent classes add nothing); class accuracy is tp over every gt point of the
    class, no-feature points included, while IoU leaves the no-feature points out.  A class whose gt points all lack a
    feature fails as in the reference (get_iou returns a bare nan, and indexing it raises TypeError)."""
    if not isinstance(dataset, str):
        raise TypeError("dataset must be the dataset name string, got %r" % (dataset,))
    if isinstance(class_labels, str) or len(class_labels) < 1 or not all(isinstance(x, str) for x in class_labels):
        raise TypeError("class_labels must be a non-empty sequence of class names")
    if hasattr(conf, "detach"):
        conf = conf.detach().cpu().numpy()
    conf = np.asarray(conf)
    n_classes = len(class_labels)
    if conf.ndim != 2 or conf.shape not in ((n_classes + 1, n_classes), (n_classes, n_classes)):
        raise ValueError("conf is %s: expected (%d, %d) or (%d, %d) for %d classes"
                         % (conf.shape, n_classes + 1, n_classes, n_classes, n_classes, n_classes))
    if conf.dtype.kind not in "iu" or (conf.size and conf.min() < 0):
        raise ValueError("conf must hold non-negative integer counts")
    gt_count = conf.sum(axis=0).astype(np.int64)                     # (gt_ids == i).sum(): no-feature points included
    confusion = conf[:n_classes, :n_classes].astype(np.ulonglong)     # metric.confusion_matrix
    if stdout:
        print('evaluating', int(conf.sum()) if n_points is None else int(n_points), 'points...')
    class_ious = {}
    class_accs = {}
    mean_iou = 0
    mean_acc = 0
    for i in range(n_classes):
        label_name = class_labels[i]
        if gt_count[i] == 0:
            continue
        class_ious[label_name] = _get_iou(i, confusion)
        class_accs[label_name] = class_ious[label_name][1] / gt_count[i]
        mean_iou += class_ious[label_name][0]
        mean_acc += class_accs[label_name]
    mean_iou /= n_classes
    mean_acc /= n_classes
    if stdout:
        print('classes          IoU')
        print('----------------------------')
        for i in range(n_classes):
            label_name = class_labels[i]
            try:
                if 'matterport' in dataset:
                    print('{0:<14s}: {1:>5.3f}'.format(label_name, class_accs[label_name]))
                else:
                    print('{0:<14s}: {1:>5.3f}   ({2:>6d}/{3:<6d})'.format(
                        label_name, class_ious[label_name][0], class_ious[label_name][1], class_ious[label_name][2]))
            except (KeyError, TypeError, IndexError, ValueError):
                print(label_name + ' error!')
                continue
        print('Mean IoU', mean_iou)
        print('Mean Acc', mean_acc)
    return EvalResult(mean_iou, mean_acc, class_ious, class_accs)


class OpenVocabEvaluator:
    """The evaluation loop of run/evaluate.py:262-424 on the device: per scene the fused query (+ test-repeat vote), per
    repeat one confusion pass and util/metric.py:evaluate's numbers.

        ev = OpenVocabEvaluator(len(text_features), class_labels, labelset_name, args.test_repeats, mapper, mark_no_feature)
        for rep_i in range(args.test_repeats):
            ev.begin_repeat()
            for ... in loader:          ev.add_distill(predictions, text_features, inds_reverse, label)   (or add_fusion,
                                        add_ensemble, add_scores)
            result = ev.end_repeat(stdout=True)

    test_repeats == 1: each scene's labels are counted at once (no vote matrix).  test_repeats > 1: one dataset-wide fp16
    vote matrix [N_pts, num_labels] (`store`); scene k of every repeat adds to slot k, whose size the first repeat fixes.
    Votes are rounded as torch's CPU `pred + store` on half tensors (fp32 add, one rounding), the prediction is
    `store.float().max(1)[1]` (first NaN, else the lowest of equal maxima), then `mapper[...]` (nuScenes 43 -> 16), then 256
    where the point has no fused feature (mark_no_feature).  gt 255 is ignored, so nuScenes' label_mask needs no
    compaction; the printed point count is still the reference's."""

    def __init__(self, num_labels, class_labels, dataset, test_repeats, mapper=None, mark_no_feature=False, device=None):
        if int(num_labels) < 1:
            raise ValueError("num_labels=%r: need at least one label" % (num_labels,))
        if int(test_repeats) < 1:
            raise ValueError("test_repeats=%r: need at least one repeat" % (test_repeats,))
        if not isinstance(dataset, str):
            raise TypeError("dataset must be the dataset name string, got %r" % (dataset,))
        if isinstance(class_labels, str) or not 1 <= len(class_labels) <= 254 or not all(isinstance(x, str) for x in class_labels):
            raise TypeError("class_labels must be a sequence of 1 to 254 class names")
        self.num_labels = int(num_labels)
        self.class_labels = list(class_labels)
        self.n_classes = len(self.class_labels)
        self.dataset = dataset
        self.test_repeats = int(test_repeats)
        self.mark_no_feature = bool(mark_no_feature)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if mapper is not None:
            mapper = torch.as_tensor(mapper, dtype=torch.int64).reshape(-1)
            if mapper.numel() < 1:
                raise ValueError("mapper is empty")
            mapper = mapper.to(self.device)
        elif self.num_labels > self.n_classes:
            raise ValueError("%d labels for %d classes need a mapper" % (self.num_labels, self.n_classes))
        self.mapper = mapper
        self.slots = []              # (first row, points) of scene k, fixed by the first repeat (test_repeats > 1)
        self.repeat = -1
        self._scene = 0
        self._chunks = None          # first repeat: per-scene (votes, labels, has_feature) until end_repeat joins them
        self.votes = self.labels = self.has_feature = None
        self._n_points = 0
        self.confusion = torch.zeros((self.n_classes + 1, self.n_classes), dtype=torch.int64, device=self.device)
        self._err = torch.zeros(1, dtype=torch.int32, device=self.device)

    # ------------------------------------------------------------------------------------------------ bookkeeping
    def begin_repeat(self):
        if self.repeat + 1 >= self.test_repeats:
            raise RuntimeError("all %d repeats are done" % self.test_repeats)
        self.repeat += 1
        self._scene = 0
        self._n_points = 0
        self._err.zero_()
        if self.test_repeats == 1 or self.repeat == 0:
            self.confusion.zero_()
        if self.test_repeats > 1 and self.repeat == 0:
            self._chunks = []

    def _slot(self, n, labels, mask):
        """-> (vote rows of this scene or None, labels, has_feature or None) on the device; advances the scene counter."""
        if self.repeat < 0 or self._scene < 0:
            raise RuntimeError("call begin_repeat() first")
        labels = torch.as_tensor(labels).to(self.device, torch.int64).reshape(-1)
        if labels.shape[0] != n:
            raise ValueError("scene %d: %d labels for %d points" % (self._scene, labels.shape[0], n))
        hf = None
        if self.mark_no_feature:
            if mask is None:
                raise ValueError("mark_no_feature needs the per-point mask of fused features")
            hf = mask.to(self.device).reshape(-1).bool()
            if hf.shape[0] != n:
                raise ValueError("scene %d: mask has %d entries for %d points" % (self._scene, hf.shape[0], n))
        k = self._scene
        if self.test_repeats == 1:
            self._scene += 1
            self._n_points += n
            return None, labels, hf
        if self.repeat == 0:
            start = self.slots[-1][0] + self.slots[-1][1] if self.slots else 0
            self.slots.append((start, n))
            v = torch.zeros((n, self.num_labels), dtype=torch.float16, device=self.device)   # `store = pred + 0.0`
            self._chunks.append((v, labels, hf))
            self._scene += 1
            self._n_points += n
            return v, labels, hf
        if k >= len(self.slots):
            raise ValueError("repeat %d brings more scenes than the first repeat (%d)" % (self.repeat, len(self.slots)))
        start, size = self.slots[k]
        if size != n:
            raise ValueError("scene %d has %d points in repeat %d but %d in the first" % (k, n, self.repeat, size))
        self._scene += 1
        self._n_points += n
        self.labels[start:start + n].copy_(labels)
        if hf is not None:
            self.has_feature[start:start + n].copy_(hf)
        return self.votes[start:start + n], labels, hf

    def _count(self, labels, hf, ids=None, votes=None):
        ops.eval_confusion(labels, self.confusion, self._err, votes=votes, ids=ids, mapper=self.mapper, has_feature=hf)

    @staticmethod
    def _mask_rows(mask, inds_reverse):
        if mask is None or inds_reverse is None:
            return mask
        return mask.to(inds_reverse.device)[inds_reverse]

    # ------------------------------------------------------------------------------------------------ one scene
    def add_distill(self, predictions, text_features, inds_reverse, labels, mask=None):
        """run/evaluate.py:288-292: predictions[inds_reverse].half() @ text.t() (predictions per voxel)."""
        n = inds_reverse.shape[0] if inds_reverse is not None else predictions.shape[0]
        votes, labels, hf = self._slot(n, labels, self._mask_rows(mask, inds_reverse))
        if votes is None:
            _, ids = ops.cosine_query(predictions, text_features, inds_reverse, want_scores=False)
            self._count(labels, hf, ids=ids)
        else:
            ops.cosine_query_vote(predictions, text_features, votes, inds_reverse)

    def add_fusion(self, feat_3d, text_features, inds_reverse, labels, mask=None):
        """run/evaluate.py:293-300: feat_3d[inds_reverse].half() @ text.t(); with mark_no_feature the points whose
        mask[inds_reverse] is False count as no-feature (256)."""
        self.add_distill(feat_3d, text_features, inds_reverse, labels, mask)

    def add_ensemble(self, predictions, feat_3d, text_features, inds_reverse, labels, mask=None):
        """run/evaluate.py:302-324: per point the source with the larger normalised best score, then its fp16 scores."""
        n = inds_reverse.shape[0] if inds_reverse is not None else predictions.shape[0]
        votes, labels, hf = self._slot(n, labels, self._mask_rows(mask, inds_reverse))
        if votes is None:
            _, ids, _ = ops.query_ensemble(predictions, feat_3d, text_features, inds_reverse, inds_reverse, want_scores=False)
            self._count(labels, hf, ids=ids)
        else:
            ops.query_ensemble_vote(predictions, feat_3d, text_features, votes, inds_reverse, inds_reverse)

    def add_scores(self, pred, labels, mask=None):
        """One scene's fp16 score matrix [n, num_labels] from anywhere else (mask: per point, already gathered)."""
        if pred.dtype != torch.float16 or pred.dim() != 2 or pred.shape[1] != self.num_labels:
            raise ValueError("pred must be a float16 [n, %d] score matrix" % self.num_labels)
        pred = pred.to(self.device)
        votes, labels, hf = self._slot(pred.shape[0], labels, mask)
        if votes is None:
            self._count(labels, hf, votes=pred)          # torch.max(pred, 1)[1] inside the confusion pass
        else:
            votes.add_(pred)                             # fp32 add, one rounding: the CPU half add's result

    # ------------------------------------------------------------------------------------------------ results
    def end_repeat(self, stdout=False):
        """util/metric.py:evaluate of this repeat (test_repeats == 1) or of the votes so far -> EvalResult."""
        if self.repeat < 0 or self._scene < 0:
            raise RuntimeError("call begin_repeat() first")
        if self.test_repeats > 1:
            if self.repeat == 0:
                self.votes = torch.cat([c[0] for c in self._chunks]) if self._chunks else \
                    torch.zeros((0, self.num_labels), dtype=torch.float16, device=self.device)
                self.labels = torch.cat([c[1] for c in self._chunks]) if self._chunks else \
                    torch.zeros(0, dtype=torch.int64, device=self.device)
                if self.mark_no_feature:
                    self.has_feature = torch.cat([c[2] for c in self._chunks]) if self._chunks else \
                        torch.zeros(0, dtype=torch.bool, device=self.device)
                self._chunks = None
            elif self._scene != len(self.slots):
                raise ValueError("repeat %d brought %d scenes, the first brought %d" % (self.repeat, self._scene, len(self.slots)))
            self.confusion.zero_()
            self._count(self.labels, self.has_feature, votes=self.votes)
        ops.eval_check(self._err)
        self._scene = -1
        conf = self.confusion.cpu().numpy()
        n_points = int(conf.sum()) if 'nuscenes' in self.dataset else self._n_points
        return evaluate_confusion(conf, self.class_labels, self.dataset, stdout=stdout, n_points=n_points)
