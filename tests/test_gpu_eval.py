"""Open-vocabulary evaluation on the GPU: the vote epilogue of the query kernels, the argmax-confusion pass and
OpenVocabEvaluator end to end, each against the host formulas of run/evaluate.py:397-424 / util/metric.py."""
import numpy as np
import pytest
import torch

from openscene_amd import metrics, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


def bits_equal(a, b):
    """fp16 tensors equal bit for bit; a NaN matches a NaN (payloads are not part of the contract)."""
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb)
    assert torch.equal(a.view(torch.int16)[~na], b.view(torch.int16)[~nb])


def text_matrix(c, d, gen):
    t = torch.randn(c, d, generator=gen)
    t = t / t.norm(dim=1, keepdim=True)
    t[0] = 1.0 / d ** 0.5                          # all positive: large equal features saturate its score
    if c > 4:
        t[3] = t[1]                                # duplicate labels: exact ties
    return t.half().to(DEV)


def features(nv, d, gen):
    x = torch.randn(nv, d, generator=gen)
    x[0:6] = 3000.0                                # score of label 0 overflows fp16: +inf
    x[6:12] = -3000.0                              # -inf (+inf in another repeat: NaN)
    x[12:14] = float("nan")                        # NaN rows
    return x.to(DEV)


@pytest.mark.parametrize("c,n", [(20, 3001), (80, 5000), (100, 4500), (160, 4600), (13, 700)])
def test_query_vote_matches_cpu_half_add(c, n):
    gen = torch.Generator().manual_seed(c)
    d = 768
    text = text_matrix(c, d, gen)
    nv = 2500
    x = features(nv, d, gen)
    votes = torch.zeros((n, c), dtype=torch.float16, device=DEV)
    store = 0.0
    for r in range(5):
        g = torch.randint(0, nv, (n,), generator=gen)
        g[:40] = torch.arange(14).repeat(3)[:40]    # every repeat meets the saturating and NaN rows
        g = g.to(DEV)
        scores, labels = ops.cosine_query(x, text, g, want_scores=True)
        store = scores.cpu() + store
        got = ops.cosine_query_vote(x, text, votes, g, want_labels=(r % 2 == 0))
        if got is not None:
            assert torch.equal(got, labels)
        bits_equal(votes, store)
    s = store.float()
    assert torch.isinf(s).any() and torch.isnan(s).any()


@pytest.mark.parametrize("c,n", [(20, 2000), (160, 4200)])
def test_ensemble_vote_matches_cpu_half_add(c, n):
    gen = torch.Generator().manual_seed(100 + c)
    d = 768
    text = text_matrix(c, d, gen)
    xd = features(1800, d, gen)
    xf = torch.randn(1800, d, generator=gen).to(DEV)
    votes = torch.zeros((n, c), dtype=torch.float16, device=DEV)
    store = 0.0
    for r in range(5):
        g = torch.randint(0, 1800, (n,), generator=gen).to(DEV)
        scores, labels, sel = ops.query_ensemble(xd, xf, text, g, g, want_scores=True)
        store = scores.cpu() + store
        got, sel2 = ops.query_ensemble_vote(xd, xf, text, votes, g, g, want_labels=True)
        assert torch.equal(got, labels) and torch.equal(sel2, sel)
        bits_equal(votes, store)


def test_vote_into_slot_of_a_larger_matrix():
    gen = torch.Generator().manual_seed(5)
    text = text_matrix(24, 512, gen)
    x = torch.randn(300, 512, generator=gen).to(DEV)
    big = torch.zeros((1000, 24), dtype=torch.float16, device=DEV)
    ops.cosine_query_vote(x, text, big[400:700])
    scores, _ = ops.cosine_query(x, text, want_scores=True)
    assert torch.equal(big[400:700], scores) and not big[:400].any() and not big[700:].any()
    with pytest.raises(ValueError):
        ops.cosine_query_vote(x, text, big[:299])
    with pytest.raises(ValueError):
        ops.cosine_query_vote(x, text, big[:300].float())


# ----------------------------------------------------------------------------------------------- confusion pass
def host_pred(votes):
    """store.float().max(1)[1] on the CPU (first NaN, else the first of equal maxima)."""
    return votes.cpu().float().max(1)[1]


def host_conf(pred, gt, c_out, mapper=None, has_feature=None):
    pred = pred.cpu().clone()
    if mapper is not None:
        pred = mapper.cpu()[pred]
    if has_feature is not None:
        pred[~has_feature.cpu()] = 256
    pred, gt = pred.numpy(), gt.cpu().numpy()
    keep = gt != 255
    pred = np.where(pred == 256, c_out, pred)
    return torch.from_numpy(np.bincount(pred[keep] * c_out + gt[keep], minlength=(c_out + 1) * c_out).reshape(c_out + 1, c_out))


def vote_matrix(n, c, gen):
    v = (torch.randn(n, c, generator=gen) * 2).half()
    if n > 64 and c > 2:
        v[0:20, 2] = v[0:20, 0]                    # ties
        v[20:30] = 0.0
        v[25:30, 1] = -0.0                         # -0.0 == +0.0: the first column wins
        v[30:40, c - 1] = float("inf")
        v[40:45, 1] = float("nan")
        v[42:45, c - 1] = float("nan")             # the first NaN wins
        v[45:50] = float("-inf")
    return v.to(DEV)


CASES = [  # (c_in, c_out, mapper)
    (1, 1, False), (20, 20, False), (43, 16, True), (90, 90, False), (100, 100, False), (160, 160, False), (7, 3, True)]


@pytest.mark.parametrize("c_in,c_out,use_mapper", CASES)
@pytest.mark.parametrize("hist", [1, 0, -1])
@pytest.mark.parametrize("n", [0, 1, 10007])
def test_confusion_votes(c_in, c_out, use_mapper, hist, n):
    gen = torch.Generator().manual_seed(c_in * 1000 + c_out + n)
    v = vote_matrix(n, c_in, gen)
    gt = torch.randint(0, c_out, (n,), generator=gen)
    gt[torch.rand(n, generator=gen) < 0.1] = 255
    mapper = torch.randint(0, c_out, (c_in,), generator=gen) if use_mapper else None
    mask = torch.rand(n, generator=gen) < 0.8
    for m in (None, mask):
        conf = torch.zeros((c_out + 1, c_out), dtype=torch.int64, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.eval_confusion(gt.to(DEV), conf, err, votes=v, mapper=None if mapper is None else mapper.to(DEV),
                           has_feature=None if m is None else m.to(DEV), hist=hist)
        ops.eval_check(err)
        assert torch.equal(conf.cpu(), host_conf(host_pred(v), gt, c_out, mapper, m))
        ids = host_pred(v)
        ops.eval_confusion(gt.to(DEV), conf, err, ids=ids.to(DEV), mapper=None if mapper is None else mapper.to(DEV),
                           has_feature=None if m is None else m.to(DEV), hist=hist)      # accumulates: twice the counts
        ops.eval_check(err)
        assert torch.equal(conf.cpu(), 2 * host_conf(ids, gt, c_out, mapper, m))


def test_confusion_ids_no_feature_256():
    gen = torch.Generator().manual_seed(9)
    n = 5000
    ids = torch.randint(0, 20, (n,), generator=gen)
    ids[torch.rand(n, generator=gen) < 0.2] = 256
    gt = torch.randint(0, 20, (n,), generator=gen)
    conf = torch.zeros((21, 20), dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.eval_confusion(gt.to(DEV), conf, err, ids=ids.to(DEV))
    ops.eval_check(err)
    assert torch.equal(conf.cpu(), host_conf(ids, gt, 20))


def test_confusion_errors():
    n = 3000
    conf = torch.zeros((17, 16), dtype=torch.int64, device=DEV)
    gt = torch.randint(0, 16, (n,), device=DEV)
    v = torch.randn(n, 43, device=DEV).half()
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.eval_confusion(gt, conf, err, votes=v, mapper=torch.arange(40, device=DEV) % 16)   # ids 40 .. 42 fall outside
    with pytest.raises(RuntimeError, match="mapper"):
        ops.eval_check(err)
    err.zero_()
    bad = gt.clone()
    bad[17] = 16
    ops.eval_confusion(bad, conf, err, votes=v, mapper=torch.arange(43, device=DEV) % 16)
    with pytest.raises(RuntimeError, match="gt"):
        ops.eval_check(err)
    err.zero_()
    ops.eval_confusion(gt, conf, err, votes=v)                 # 43 predictions for 16 classes without a mapper
    with pytest.raises(RuntimeError, match="prediction outside"):
        ops.eval_check(err)
    with pytest.raises(ValueError):
        ops.eval_confusion(gt, conf, err)
    with pytest.raises(ValueError):
        ops.eval_confusion(gt, torch.zeros((16, 16), dtype=torch.int64, device=DEV), err, votes=v)
    big = torch.zeros((201, 200), dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError):                          # an LDS histogram of 200 classes does not fit
        ops.eval_confusion(torch.zeros(10, dtype=torch.int64, device=DEV), big, err, ids=torch.zeros(10, dtype=torch.int64, device=DEV), hist=1)


# ----------------------------------------------------------------------------------------------- end to end
def make_dataset(gen, n_scenes=20, c_gt=20, d=768):
    scenes = []
    for k in range(n_scenes):
        n = 0 if k == 7 else int(torch.randint(200, 3000, (1,), generator=gen))
        label = torch.randint(0, c_gt, (n,), generator=gen)
        label[torch.rand(n, generator=gen) < 0.08] = 255
        feat_3d = torch.randn(n, d, generator=gen)
        mask = torch.rand(n, generator=gen) < 0.85
        scenes.append((n, label, feat_3d.to(DEV), mask))
    return scenes


def voxelize(n, gen):
    """A repeat's random inds_reverse (point -> voxel) and a per-voxel network output."""
    nv = max(1, n // 2)
    return torch.randint(0, nv, (n,), generator=gen).to(DEV), nv


def host_replay(per_repeat_scores, gts, masks, mapper, c_out, names, dataset):
    """run/evaluate.py:397-424 on the host: cat, store = pred + store (CPU fp16), store.float().max(1)[1], mapper,
    [~mask] = 256, metric.evaluate (its confusion = host_conf) -> EvalResult and matrix per repeat."""
    gt = torch.cat(gts)
    mask = torch.cat(masks) if masks is not None else None
    store = 0.0
    out = []
    for preds in per_repeat_scores:
        pred = torch.cat(preds)
        if len(per_repeat_scores) > 1:
            store = pred + store
            logit = store.float().max(1)[1]
        else:
            logit = pred.float().max(1)[1]
        conf = host_conf(logit, gt, c_out, mapper, mask)
        out.append((conf, metrics.evaluate_confusion(conf.numpy(), names, dataset, n_points=gt.numel())))
    return out


@pytest.mark.parametrize("mode,repeats", [("distill", 5), ("fusion", 5), ("fusion", 1), ("ensemble", 3), ("scores", 4), ("distill", 1)])
def test_evaluator_end_to_end(mode, repeats):
    gen = torch.Generator().manual_seed(sum(map(ord, mode)) * 10 + repeats)
    d = 768
    nuscenes = mode == "ensemble"
    c_lab, c_out = (43, 16) if nuscenes else (20, 20)
    names = ["class%d" % i for i in range(c_out)]
    dataset = "nuscenes_3d" if nuscenes else "scannet_3d"
    mapper = torch.randint(0, 16, (43,), generator=gen) if nuscenes else None
    mark = mode == "fusion"
    text = text_matrix(c_lab, d, gen)
    scenes = make_dataset(gen, c_gt=c_out, d=d)
    ev = metrics.OpenVocabEvaluator(c_lab, names, dataset, repeats, mapper=mapper, mark_no_feature=mark, device=DEV)
    per_repeat = []
    for r in range(repeats):
        ev.begin_repeat()
        preds = []
        for n, label, feat_3d, mask in scenes:
            inds, nv = voxelize(n, gen)
            net = torch.randn(nv, d, generator=gen).to(DEV)
            if mode == "distill":
                ev.add_distill(net, text, inds, label)
                s, _ = ops.cosine_query(net, text, inds)
            elif mode == "fusion":
                ev.add_fusion(feat_3d, text, None, label, mask)
                s, _ = ops.cosine_query(feat_3d, text)
            elif mode == "ensemble":
                fv = feat_3d[torch.randint(0, max(n, 1), (nv,), generator=gen).to(DEV)] if n else feat_3d[:0]
                ev.add_ensemble(net, fv, text, inds, label)
                s, _, _ = ops.query_ensemble(net, fv, text, inds, inds)
            else:
                s, _ = ops.cosine_query(net, text, inds)
                ev.add_scores(s, label)
            preds.append(s.cpu())
        per_repeat.append(preds)
        got = ev.end_repeat()
        conf, want = host_replay(per_repeat if repeats > 1 else [preds], [s[1] for s in scenes],
                                 [s[3] for s in scenes] if mark else None, mapper, c_out, names, dataset)[-1]
        assert torch.equal(ev.confusion.cpu(), conf)
        assert got.mean_iou == want.mean_iou and got.mean_acc == want.mean_acc
        assert got.class_ious == want.class_ious and got.class_accs == want.class_accs


def test_evaluator_errors():
    gen = torch.Generator().manual_seed(3)
    text = text_matrix(20, 512, gen)
    names = ["c%d" % i for i in range(20)]
    x = torch.randn(100, 512, generator=gen).to(DEV)
    ev = metrics.OpenVocabEvaluator(20, names, "scannet_3d", 2, device=DEV)
    ev.begin_repeat()
    ev.add_distill(x, text, None, torch.zeros(100, dtype=torch.int64))
    ev.end_repeat()
    ev.begin_repeat()
    with pytest.raises(ValueError, match="points"):            # slot 0 held 100 points
        ev.add_distill(x[:90], text, None, torch.zeros(90, dtype=torch.int64))
    ev = metrics.OpenVocabEvaluator(20, names, "scannet_3d", 1, device=DEV)
    ev.begin_repeat()
    bad = torch.zeros(100, dtype=torch.int64)
    bad[5] = 21
    ev.add_distill(x, text, None, bad)
    with pytest.raises(RuntimeError, match="gt"):
        ev.end_repeat()
    ev = metrics.OpenVocabEvaluator(20, names[:16], "nuscenes_3d", 2, mapper=torch.arange(10), device=DEV)
    ev.begin_repeat()
    ev.add_distill(x, text, None, torch.zeros(100, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="mapper"):
        ev.end_repeat()
