"""Stand-alone cost of the supervised-baseline head (csrc/seg.hip) and optimizer (osn_sgd_step) against what the reference
runs (run/train_mink.py:147-148,160,279-290).  HIP events around many back-to-back iterations after a warm-up.

    python tools/micro_seg.py [iters]

Prints one JSON object per line:
  kind=loss   per (n, c): our forward (loss + pred + confusion in one launch pair), backward, metric-only update, against
              F.cross_entropy forward / backward and `.max(1)[1]` + intersectionAndUnionGPU (util/util.py:132-145, restated
              here with its three host copies and CPU histc); bytes each of our passes must move and the rate that implies
  kind=optim  FlatSGD.step() against torch.optim.SGD(momentum=0.9, weight_decay=1e-4).step() on MinkUNet18A(3, 20)
  kind=step   one full supervised step on S100k (maps, forward, loss, backward, SGD, metrics), both ways"""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import ops, synthetic as syn                       # noqa: E402
from openscene_amd.losses import segmentation_loss                    # noqa: E402
from openscene_amd.metrics import SegmentationMeter                   # noqa: E402
from openscene_amd.mink_unet import mink_unet                         # noqa: E402
from openscene_amd.optim import FlatSGD                               # noqa: E402
from openscene_amd.sparse import SparseTensor                         # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device("cuda", 0)


def timed(f, iters=ITERS, warmup=10):
    """us per call: device events around `iters` calls (calls that wait on the host are timed with their waits)."""
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def intersection_and_union_gpu(output, target, K, ignore_index=255):
    """util/util.py:132-145 as the reference runs it (three device -> host copies, CPU histc, three copies back)."""
    output = output.view(-1).clone()
    target = target.view(-1)
    output[target == ignore_index] = ignore_index
    intersection = output[output == target]
    a_i = torch.histc(intersection.float().cpu(), bins=K, min=0, max=K - 1)
    a_o = torch.histc(output.float().cpu(), bins=K, min=0, max=K - 1)
    a_t = torch.histc(target.float().cpu(), bins=K, min=0, max=K - 1)
    return a_i.cuda(), (a_o + a_t - a_i).cuda(), a_t.cuda()


def emit(d):
    print(json.dumps(d), flush=True)


def loss_rows():
    for name, n, c in (("S100k/ScanNet", 100999, 20), ("nuScenes", 236000, 16), ("Matterport", 150000, 21),
                       ("Matterport-160", 150000, 160)):
        g = torch.Generator(device=dev).manual_seed(n + c)
        x = torch.randn(n, c, device=dev, generator=g) * 3
        y = torch.randint(0, c, (n,), device=dev, generator=g)
        y[torch.rand(n, device=dev, generator=g) < 0.15] = 255
        xg = x.clone().requires_grad_()
        meter = SegmentationMeter(c, device=dev)
        gl = torch.ones((), device=dev)
        state = {}

        def ours_fwd():
            state["l"], state["p"], state["s"] = ops.seg_loss_fwd(x, y, 255, want_pred=True, confusion=meter.confusion)

        ours_fwd()

        def ours_bwd():
            ops.seg_loss_bwd(x, y, state["s"], 255, gl)

        def ours_meter():
            meter.update(x, y)

        def ours_step():                  # autograd node: forward + backward, metrics in the forward's pass
            loss = segmentation_loss(xg, y, meter=meter)
            loss.backward()

        def torch_fwd():
            F.cross_entropy(x, y, ignore_index=255)

        def torch_step():
            loss = F.cross_entropy(xg, y, ignore_index=255)
            loss.backward()

        def torch_metric():
            pred = x.max(1)[1]
            intersection_and_union_gpu(pred, y, c, 255)

        def torch_step_and_metric():
            loss = F.cross_entropy(xg, y, ignore_index=255)
            loss.backward()
            pred = x.detach().max(1)[1]
            i, u, t = intersection_and_union_gpu(pred, y, c, 255)
            i.cpu(), u.cpu(), t.cpu()                    # run/train_mink.py:288-289

        t = dict(kind="loss", shape=name, n=n, c=c,
                 ours_fwd_us=timed(ours_fwd), ours_bwd_us=timed(ours_bwd), ours_meter_update_us=timed(ours_meter),
                 ours_fwd_bwd_metrics_us=timed(ours_step),
                 torch_fwd_us=timed(torch_fwd), torch_fwd_bwd_us=timed(torch_step),
                 torch_metrics_us=timed(torch_metric, iters=max(ITERS // 4, 10)),
                 torch_fwd_bwd_metrics_us=timed(torch_step_and_metric, iters=max(ITERS // 4, 10)))
        fwd_bytes = n * c * 4 + n * 8 + n * 8            # logits + labels + pred
        bwd_bytes = 2 * n * c * 4 + n * 8                # logits + gradient + labels
        t["fwd_bytes"], t["bwd_bytes"] = fwd_bytes, bwd_bytes
        t["ours_fwd_GBps"] = fwd_bytes / t["ours_fwd_us"] / 1e3
        t["ours_bwd_GBps"] = bwd_bytes / t["ours_bwd_us"] / 1e3
        emit(t)


def optim_row():
    torch.manual_seed(0)
    models = [mink_unet(3, 20, 3, "MinkUNet18A").to(dev) for _ in range(2)]
    opts = [FlatSGD(models[0], lr=0.01, momentum=0.9, weight_decay=1e-4),
            torch.optim.SGD(models[1].parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)]
    n_params = sum(p.numel() for p in models[1].parameters())
    # our gradients as the network executor hands them out (slices of one flat buffer in the optimizer's layout: read in place)
    flat_grad = torch.randn(opts[0].total, device=dev) * 1e-3
    for p, o in zip(opts[0]._params, opts[0].offsets):
        p.grad = flat_grad[o:o + p.numel()].view_as(p)
    assert opts[0]._flat_grads()[1]
    for p in models[1].parameters():
        p.grad = torch.randn_like(p) * 1e-3
    flat = timed(opts[0].step)
    ref = timed(opts[1].step)
    emit(dict(kind="optim", model="MinkUNet18A(3, 20)", n_tensors=len(list(models[1].parameters())), n_params=n_params,
              ours_flat_sgd_us=flat, torch_sgd_us=ref, bytes=20 * n_params, ours_GBps=20 * n_params / flat / 1e3))


def step_row():
    vox = syn.shuffled(syn.grid_voxels(syn.room_points(0), 0.02), 0)
    coords = torch.from_numpy(syn.batch_coords([vox])).to(dev)
    n = coords.shape[0]
    labels = ((vox[:, 0].astype(np.int64) // 20) * 3 + vox[:, 1] // 20 + vox[:, 2] // 15) % 20
    labels[np.random.default_rng(0).random(n) < 0.15] = 255
    label = torch.from_numpy(labels).to(dev)
    feats = torch.rand(n, 3, device=dev)
    out = {}
    for way in ("ours", "torch"):
        torch.manual_seed(1)
        model = mink_unet(3, 20, 3, "MinkUNet18A").to(dev).train()
        if way == "ours":
            opt = FlatSGD(model, lr=0.01, momentum=0.9, weight_decay=1e-4)
            meter = SegmentationMeter(20, device=dev)

            def step():
                o = model(SparseTensor(feats, coords))
                loss = segmentation_loss(o, label, meter=meter)
                opt.zero_grad()
                loss.backward()
                opt.step()
        else:
            opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
            crit = torch.nn.CrossEntropyLoss(ignore_index=255)

            def step():
                o = model(SparseTensor(feats, coords))
                loss = crit(o, label)
                opt.zero_grad()
                loss.backward()
                opt.step()
                pred = o.detach().max(1)[1]
                i, u, t = intersection_and_union_gpu(pred, label, 20, 255)
                i.cpu(), u.cpu(), t.cpu()
        iters = max(ITERS // 10, 10)
        out[way + "_step_ms"] = timed(step, iters=iters, warmup=5) / 1e3
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        out[way + "_step_wall_ms"] = (time.perf_counter() - t0) * 1e3 / iters
    emit(dict(kind="step", scene="S100k", voxels=n, model="MinkUNet18A(3, 20)", **out))


if __name__ == "__main__":
    emit(dict(kind="env", device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=ITERS))
    loss_rows()
    optim_row()
    step_row()
