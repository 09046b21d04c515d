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
