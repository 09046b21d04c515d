"""The supervised-baseline head on the MI355X (csrc/seg.hip, osn_sgd_step in csrc/optim.hip): cross-entropy with ignore_index
against torch in float64, argmax and confusion matrix against the reference's formulas, the gathered forward and the
test-repeat vote, determinism, index checks, FlatSGD against torch.optim.SGD, and three supervised steps of MinkUNet18A
both ways (run/train_mink.py:147-148,160,279-306)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from openscene_amd import ops
from openscene_amd._lib import OpenSceneAmdError
from openscene_amd.losses import SegmentationLoss, segmentation_loss
from openscene_amd.metrics import SegmentationMeter
from openscene_amd.optim import FlatSGD

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-300)).item()


def make(n, c, frac, ignore, scale, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, generator=g) * scale
    y = torch.randint(0, c, (n,), generator=g)
    if frac >= 1.0:
        y[:] = ignore
    elif frac > 0:
        y[torch.rand(n, generator=g) < frac] = ignore
    return x, y


def torch_ref(x, y, ignore):
    xd = x.double().requires_grad_()
    loss = F.cross_entropy(xd, y, ignore_index=ignore)
    loss.backward()
    return loss.detach(), xd.grad


def reference_iou(pred, label, K, ignore):
    """intersectionAndUnionGPU (util/util.py:132-145) restated in numpy."""
    output = pred.copy()
    output[label == ignore] = ignore
    inter = output[output == label]
    hist = lambda v: np.histogram(v, bins=np.arange(K + 1))[0] if len(v) else np.zeros(K, np.int64)
    keep = lambda v: v[(v >= 0) & (v < K)]                                 # torch.histc(min=0, max=K-1) drops the rest
    a_i, a_o, a_t = hist(keep(inter)), hist(keep(output)), hist(keep(label))
    return a_i, a_o + a_t - a_i, a_t


def confusion_np(pred, label, K, ignore):
    """util/metric.py:9-25's formula (its UNKNOWN_ID generalised to ignore)."""
    idx = label != ignore
    return np.bincount(pred[idx] * K + label[idx], minlength=K * K).reshape(K, K)


SHAPES = [(1, 20), (7, 3), (5000, 21), (100999, 20), (236000, 16), (150000, 40), (20000, 160), (3000, 256)]


@pytest.mark.parametrize("n,c", SHAPES)
@pytest.mark.parametrize("frac", [0.0, 0.15, 1.0])
@pytest.mark.parametrize("ignore", [255, -100])
@pytest.mark.parametrize("scale", [1.0, 80.0])
def test_loss_and_gradient_against_torch_float64(n, c, frac, ignore, scale):
    x, y = make(n, c, frac, ignore, scale, seed=n + c)
    ref_loss, ref_grad = torch_ref(x, y, ignore)
    xg = x.to(dev()).requires_grad_()
    loss = segmentation_loss(xg, y.to(dev()), ignore_index=ignore)
    loss.backward()
    got = loss.detach().cpu().double()
    if frac >= 1.0:
        assert torch.isnan(ref_loss) and torch.isnan(got)
        assert torch.count_nonzero(xg.grad).item() == 0
        return
    assert abs(got.item() - ref_loss.item()) <= 2e-6 * abs(ref_loss.item()), (got.item(), ref_loss.item())
    assert rel_l2(xg.grad, ref_grad) <= 1e-6


@pytest.mark.parametrize("c", [3, 20, 21, 160])
def test_rows_near_ten_thousand(c):
    """Rows of logits around +-1e4 (float64 torch is still finite there): max - x[y] is exact in fp32 and the log-sum-exp
    is taken after the row maximum is subtracted."""
    g = torch.Generator().manual_seed(c)
    n = 4096
    sign = torch.where(torch.rand(n, 1, generator=g) < 0.5, -1.0, 1.0)
    x = sign * 1e4 + torch.randn(n, c, generator=g) * 3
    y = torch.randint(0, c, (n,), generator=g)
    y[::7] = 255
    ref_loss, ref_grad = torch_ref(x, y, 255)
    xg = x.to(dev()).requires_grad_()
    loss = SegmentationLoss(ignore_index=255)(xg, y.to(dev()))
    loss.backward()
    assert abs(loss.item() - ref_loss.item()) <= 2e-6 * abs(ref_loss.item())
    assert rel_l2(xg.grad, ref_grad) <= 1e-6


@pytest.mark.parametrize("n,c", [(5000, 21), (100999, 20), (20000, 160), (3000, 256), (7, 3)])
def test_argmax_and_confusion_with_ties(n, c):
    g = torch.Generator().manual_seed(3 * n + c)
    ign = 255 if c <= 255 else -100          # (with 256 classes 255 is a class: the reference's histc would count it)
    meter = SegmentationMeter(c, ignore_index=ign, device=dev())
    conf_total = np.zeros((c, c), np.int64)
    sums = [np.zeros(c, np.int64) for _ in range(3)]
    for call in range(3):
        x = torch.randint(-2, 3, (n, c), generator=g).float()             # many exact ties: the lowest column must win
        x[: n // 3] = torch.randn(n // 3, c, generator=g)
        y = torch.randint(0, c, (n,), generator=g)
        y[torch.rand(n, generator=g) < 0.15] = ign
        loss, pred = segmentation_loss(x.to(dev()), y.to(dev()), ignore_index=ign, pred=True, meter=meter)
        ref_pred = x.max(1)[1]
        assert torch.equal(pred.cpu(), ref_pred)
        pn, yn = ref_pred.numpy(), y.numpy()
        conf_total += confusion_np(pn, yn, c, ign)
        for s, v in zip(sums, reference_iou(pn, yn, c, ign)):
            s += v
    assert np.array_equal(meter.matrix(), conf_total)
    inter, union, target = meter.intersection_union_target()
    assert np.array_equal(inter, sums[0]) and np.array_equal(union, sums[1]) and np.array_equal(target, sums[2])
    iou = sums[0] / (sums[1] + 1e-10)
    assert np.allclose(meter.iou(), iou) and abs(meter.miou() - np.mean(iou)) < 1e-12
    assert abs(meter.macc() - np.mean(sums[0] / (sums[2] + 1e-10))) < 1e-12
    assert abs(meter.allacc() - sum(sums[0]) / (sum(sums[2]) + 1e-10)) < 1e-12
    meter.reset()
    assert int(meter.confusion.abs().sum()) == 0


@pytest.mark.parametrize("n,c", [(5000, 21), (30000, 20), (4000, 160)])
def test_gathered_forward_and_votes(n, c):
    """rows = inds_reverse (every voxel at least once, duplicates): loss, pred and confusion of logits[rows] without the
    gather; the vote over three test repeats equals torch's running sum (run/eval_mink.py:210)."""
    g = torch.Generator().manual_seed(n + 7 * c)
    n_pts = 3 * n
    rows = torch.cat([torch.randperm(n, generator=g), torch.randint(0, n, (n_pts - n,), generator=g)])
    rows = rows[torch.randperm(n_pts, generator=g)]
    x = torch.randn(n, c, generator=g) * 4
    y = torch.randint(0, c, (n_pts,), generator=g)
    y[torch.rand(n_pts, generator=g) < 0.15] = 255
    meter = SegmentationMeter(c, device=dev())
    with torch.no_grad():
        loss, pred = segmentation_loss(x.to(dev()), y.to(dev()), rows=rows.to(dev()), pred=True, meter=meter, validate=True)
    ref_loss, _ = torch_ref(x[rows], y, 255)
    assert abs(loss.item() - ref_loss.item()) <= 2e-6 * abs(ref_loss.item())
    ref_pred = x[rows].max(1)[1]
    assert torch.equal(pred.cpu(), ref_pred)
    assert np.array_equal(meter.matrix(), confusion_np(ref_pred.numpy(), y.numpy(), c, 255))
    # votes
    store = torch.zeros(n_pts, c)
    votes = torch.zeros(n_pts, c, device=dev())
    for rep in range(3):
        xr = torch.randn(n, c, generator=g)
        store = xr[rows] + store
        ops.seg_vote(xr.to(dev()), votes, rows=rows.to(dev()))
    assert torch.equal(votes.cpu(), store)
    vm = SegmentationMeter(c, device=dev())
    vm.update(votes, y.to(dev()))
    assert np.array_equal(vm.matrix(), confusion_np(store.max(1)[1].numpy(), y.numpy(), c, 255))


def test_deterministic():
    x, y = make(100999, 20, 0.15, 255, 4.0, seed=11)
    outs = []
    for _ in range(2):
        xg = x.to(dev()).requires_grad_()
        loss = segmentation_loss(xg, y.to(dev()))
        loss.backward()
        outs.append((loss.detach().clone(), xg.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_check_reports_bad_labels_and_rows():
    n, c = 1000, 20
    x = torch.randn(n, c, device=dev())
    for bad in (c, c + 7):
        y = torch.randint(0, c, (n,), device=dev())
        y[17] = bad
        with pytest.raises(OpenSceneAmdError):
            segmentation_loss(x, y, validate=True)
        loss = segmentation_loss(x, y)                                   # not validated: the row counts as ignored
        y2 = y.clone()
        y2[17] = 255
        assert torch.equal(loss, segmentation_loss(x, y2))
    rows = torch.arange(n, device=dev())
    rows[5] = n
    y = torch.randint(0, c, (n,), device=dev())
    with torch.no_grad(), pytest.raises(OpenSceneAmdError):
        segmentation_loss(x, y, rows=rows, validate=True)
    torch.cuda.synchronize()


SGD_SETTINGS = [dict(momentum=m, dampening=d, nesterov=ne, weight_decay=wd)
                for m in (0.0, 0.9) for d in (0.0, 0.1) for ne in (False, True) for wd in (0.0, 1e-4)
                if not (ne and (m == 0 or d != 0))]


def _close(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return bool(((a - b).abs() <= 1e-6 * b.abs() + 1e-9).all())


@pytest.mark.parametrize("kw", SGD_SETTINGS, ids=lambda k: "m%g_d%g_n%d_wd%g" % (k["momentum"], k["dampening"], k["nesterov"], k["weight_decay"]))
def test_flat_sgd_against_torch_sgd(kw):
    d = dev()
    g = torch.Generator().manual_seed(21)
    shapes = [(27, 32, 33), (7,), (96, 5), (1,), (3, 3, 3)]
    init = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) for s in shapes] for _ in range(6)]
    lrs = [0.05 * (1 - i / 6) ** 0.9 for i in range(6)]

    def run(kind, load_from=None, steps=range(6)):
        ps = [torch.nn.Parameter(t.clone().to(d)) for t in init]
        opt = FlatSGD(ps, lr=0.05, **kw) if kind == "ours" else torch.optim.SGD(ps, lr=0.05, **kw)
        return ps, opt

    def step(ps, opt, i):
        opt.param_groups[0]["lr"] = lrs[i]
        for p, gr in zip(ps, grads[i]):
            p.grad = gr.to(d)
        opt.step()

    rp, ro = run("torch")
    op, oo = run("ours")
    sd = {}
    for i in range(6):
        step(rp, ro, i)
        step(op, oo, i)
        for a, b in zip(op, rp):
            assert _close(a, b), "step %d" % i
        if i == 2:
            # (torch's state dict holds its live buffers, which its later steps update in place: a checkpoint is a copy)
            sd = {"torch": copy.deepcopy(ro.state_dict()), "ours": copy.deepcopy(oo.state_dict())}
            saved = [p.detach().clone() for p in rp]
    # checkpoints written after step 3 by one optimizer and loaded into the other continue to the same parameters
    for src, kind in (("torch", "ours"), ("ours", "torch")):
        ps = [torch.nn.Parameter(t.clone()) for t in saved]
        opt = FlatSGD(ps, lr=1.0) if kind == "ours" else torch.optim.SGD(ps, lr=1.0)
        opt.load_state_dict(sd[src])
        for i in range(3, 6):
            step(ps, opt, i)
        for a, b in zip(ps, rp):
            assert _close(a, b), "%s -> %s" % (src, kind)


def test_three_supervised_steps_both_ways():
    """MinkUNet18A(3, 20) through the network executor on a synthetic room, three steps with a poly learning rate:
    (a) SegmentationLoss + FlatSGD + SegmentationMeter, (b) F.cross_entropy + torch.optim.SGD + the reference's metric in
    numpy, from identical weights."""
    from openscene_amd import executor as E
    from openscene_amd import synthetic as syn
    from openscene_amd.mink_unet import mink_unet
    from openscene_amd.sparse import SparseTensor
    assert E.ENABLED
    d = dev()
    rng = np.random.default_rng(4)
    vox = syn.shuffled(syn.grid_voxels(syn.room_points(4, n_pts=36000), 0.03), 4)
    xyz = vox.astype(np.int64)
    labels = ((xyz[:, 0] // 12) * 3 + (xyz[:, 1] // 12) * 5 + xyz[:, 2] // 10) % 20
    labels[rng.random(len(labels)) < 0.15] = 255
    shift = rng.integers(0, 100, size=3)
    coords = torch.from_numpy(syn.batch_coords([vox + shift])).to(d)
    n = coords.shape[0]
    assert 10000 < n < 80000
    feats = torch.rand(n, 3, generator=torch.Generator().manual_seed(1)).to(d)
    label = torch.from_numpy(labels).to(d)
    torch.manual_seed(12)
    model_a = mink_unet(3, 20, 3, "MinkUNet18A").to(d).train()
    model_b = mink_unet(3, 20, 3, "MinkUNet18A").to(d).train()
    model_b.load_state_dict(model_a.state_dict())
    base_lr, max_iter = 0.01, 3                                   # config/scannet/mink.yaml
    kw = dict(momentum=0.9, weight_decay=1e-4)
    opt_a = FlatSGD(model_a, lr=base_lr, **kw)
    opt_b = torch.optim.SGD(model_b.parameters(), lr=base_lr, **kw)
    crit = SegmentationLoss(ignore_index=255)
    meter = SegmentationMeter(20, ignore_index=255, device=d)
    ref_sums = [np.zeros(20, np.int64) for _ in range(3)]
    p0 = {k: p.detach().clone() for k, p in model_b.named_parameters()}
    for it in range(max_iter):
        out_a = model_a(SparseTensor(feats, coords))
        loss_a = crit(out_a, label)
        opt_a.zero_grad()
        loss_a.backward()
        opt_a.step()
        if it == 0:
            meter.update(out_a.detach(), label)                       # warm the path once outside the checked mode
            meter.reset()
        torch.cuda.set_sync_debug_mode("error")
        try:
            meter.update(out_a.detach(), label)
            if it == 0:
                with pytest.raises(RuntimeError):                     # the mode works here: the reference's host copy raises
                    out_a.detach().max(1)[1].cpu()
        finally:
            torch.cuda.set_sync_debug_mode(0)

        out_b = model_b(SparseTensor(feats, coords))
        loss_b = F.cross_entropy(out_b, label, ignore_index=255)
        opt_b.zero_grad()
        loss_b.backward()
        opt_b.step()
        pred_b = out_b.detach().max(1)[1].cpu().numpy()
        for s, v in zip(ref_sums, reference_iou(pred_b, labels, 20, 255)):
            s += v
        if it == 0:
            # the same forward pass both ways: exactly the same counts, and every parameter took the same first update
            assert all(np.array_equal(a, b) for a, b in zip(meter.intersection_union_target(), ref_sums))
            # (per parameter the bound is looser: the logits' gradients differ by fp32 round-off, and the training-mode batch
            # norms behind the convolutions subtract their means -- a cancellation that magnifies it; 7.8e-5 measured)
            pa = dict(model_a.named_parameters())
            upd_a = torch.cat([(pa[k] - p0[k]).detach().flatten() for k in p0])
            upd_b = torch.cat([(p - p0[k]).detach().flatten() for k, p in model_b.named_parameters()])
            assert rel_l2(upd_a, upd_b) <= 1e-5, rel_l2(upd_a, upd_b)
            worst = max(rel_l2(pa[k] - p0[k], p - p0[k]) for k, p in model_b.named_parameters())
            assert worst <= 5e-4, "first update, worst parameter: %.3e" % worst
        la, lb = loss_a.item(), loss_b.item()
        assert abs(la - lb) <= 1e-5 * abs(lb), (it, la, lb)
        lr = base_lr * (1 - float(it + 1) / max_iter) ** 0.9         # poly_learning_rate, run/train_mink.py:303-306
        for o in (opt_a, opt_b):
            for grp in o.param_groups:
                grp["lr"] = lr
    # after three steps, over the whole parameter vector: the second and third forward passes start from weights that differ by
    # fp32 round-off, which flips a few ReLUs and moves those steps' gradients by ~1e-3 of themselves (1.4e-5 measured here,
    # 2.8e-5 at lr 0.05); the first update above, where both forward passes are the same, agrees to 1e-5
    pa = dict(model_a.named_parameters())
    ours = torch.cat([pa[k].detach().flatten() for k, _ in model_b.named_parameters()])
    ref = torch.cat([p.detach().flatten() for _, p in model_b.named_parameters()])
    assert rel_l2(ours, ref) <= 5e-5, rel_l2(ours, ref)
