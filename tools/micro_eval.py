"""Cost of the open-vocabulary evaluation on the device (csrc/query.hip vote epilogue, csrc/evaluate.hip) against what the
reference runs (run/evaluate.py:390-424, util/metric.py).  HIP events around back-to-back calls after a warm-up.

    python tools/micro_eval.py [iters]

Prints one JSON object per line:
  kind=query_vote  per (n, d, c): the fused query writing labels only, against the same query adding into the vote matrix
  kind=confusion   per (n, c, hist): the argmax-confusion pass over an fp16 vote matrix; bytes it must read and the rate
  kind=repeat      one whole test repeat at ScanNet-val size (312 scenes x 150 k points, 20 labels): the device path
                   (query + vote per scene, one confusion pass, evaluate_confusion) against the reference's host path
                   (per-scene pred.cpu(), torch.cat, CPU fp16 `pred + store`, .float().max(1), metric.evaluate's bincount)"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import metrics, ops                              # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
dev = torch.device("cuda", 0)
HBM_PEAK = 8.0e12


def timed(f, iters=ITERS, warmup=5):
    """us per call: device events around `iters` calls."""
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


def emit(**kw):
    print(json.dumps(kw), flush=True)


def text_matrix(c, d, gen):
    t = torch.randn(c, d, generator=gen)
    return (t / t.norm(dim=1, keepdim=True)).half().to(dev)


def query_vote():
    gen = torch.Generator().manual_seed(1)
    for n, d, c in ((150_000, 768, 20), (500_000, 768, 160)):
        nv = n // 2
        x = torch.randn(nv, d, generator=gen).to(dev)
        g = torch.randint(0, nv, (n,), generator=gen).to(dev)
        text = text_matrix(c, d, gen)
        votes = torch.zeros((n, c), dtype=torch.float16, device=dev)
        # alternate the two forms (A B A B) to see the spread
        r = []
        for _ in range(2):
            r.append(("labels", timed(lambda: ops.cosine_query(x, text, g, want_scores=False))))
            r.append(("vote", timed(lambda: ops.cosine_query_vote(x, text, votes, g))))
            r.append(("vote+labels", timed(lambda: ops.cosine_query_vote(x, text, votes, g, want_labels=True))))
        t = {k: [v for kk, v in r if kk == k] for k in ("labels", "vote", "vote+labels")}
        emit(kind="query_vote", n=n, d=d, c=c, us_labels=t["labels"], us_vote=t["vote"], us_vote_labels=t["vote+labels"],
             ratio_vote=min(t["vote"]) / min(t["labels"]), x_bytes=n * d * 4, vote_bytes=n * c * 4)


def confusion():
    gen = torch.Generator().manual_seed(2)
    for n, c in ((46_800_000, 20), (10_000_000, 43), (10_000_000, 90), (10_000_000, 128), (10_000_000, 160)):
        votes = (torch.randn(n, c, generator=gen) * 2).half().to(dev)
        c_out = 16 if c == 43 else c
        gt = torch.randint(0, c_out, (n,), generator=gen)
        gt[torch.rand(n, generator=gen) < 0.1] = 255
        # realistic predictions are mostly right: put the gt's column on top for 60 % of the rows
        right = (torch.rand(n, generator=gen) < 0.6) & (gt != 255)
        if c == c_out:
            votes[right.to(dev), gt[right].to(dev)] = 20.0
        gt = gt.to(dev)
        mapper = (torch.arange(43) % 16).to(dev) if c == 43 else None
        conf = torch.zeros((c_out + 1, c_out), dtype=torch.int64, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        nbytes = n * c * 2 + n * 8
        for hist in ((1, 0, 1, 0) if c_out <= 160 else (0,)):
            us = timed(lambda: ops.eval_confusion(gt, conf, err, votes=votes, mapper=mapper, hist=hist), iters=max(5, ITERS // 5))
            emit(kind="confusion", n=n, c_in=c, c_out=c_out, hist=hist, us=us, bytes=nbytes, gbps=nbytes / us * 1e-3,
                 hbm_share=nbytes / us * 1e6 / HBM_PEAK)
        ops.eval_check(err)
        del votes


def whole_repeat():
    gen = torch.Generator().manual_seed(3)
    scenes, n, d, c = 312, 150_000, 768, 20
    nv = 75_000
    x = torch.randn(nv, d, generator=gen).to(dev)
    text = text_matrix(c, d, gen)
    gathers = [torch.randint(0, nv, (n,), generator=gen).to(dev) for _ in range(8)]
    labels = [torch.randint(0, c, (n,), generator=gen) for _ in range(8)]
    names = ["class%d" % i for i in range(c)]
    mapper = None
    # device path: first repeat (slots fixed) then a second, timed repeat
    ev = metrics.OpenVocabEvaluator(c, names, "scannet_3d", 2, device=dev)
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.begin_repeat()
        for k in range(scenes):
            ev.add_distill(x, text, gathers[k % 8], labels[k % 8])
        res = ev.end_repeat()
        t_dev = time.perf_counter() - t0
    # the reference's host path for the same scores (the copies wait for the same GPU query)
    preds = []
    gts = []
    store = 0.0
    torch.cuda.synchronize()
    t_copy = t_host = 0.0
    for k in range(scenes):
        s, _ = ops.cosine_query(x, text, gathers[k % 8], want_scores=True)
        t0 = time.perf_counter()
        preds.append(s.cpu())
        gts.append(labels[k % 8])
        t_copy += time.perf_counter() - t0
    t0 = time.perf_counter()
    gt = torch.cat(gts)
    pred = torch.cat(preds)
    store = pred + store
    logit = store.float().max(1)[1]
    if mapper is not None:
        logit = mapper[logit]
    p, g = logit.numpy(), gt.numpy()
    idx = g != 255
    conf = np.bincount(p[idx] * c + g[idx], minlength=c * c).reshape(c, c)
    for i in range(c):
        (g == i).sum()
    t_host = time.perf_counter() - t0
    emit(kind="repeat", scenes=scenes, points=scenes * n, c=c, device_s=t_dev, host_copy_s=t_copy, host_cpu_s=t_host,
         host_total_s=t_copy + t_host, speedup=(t_copy + t_host) / t_dev, threads=torch.get_num_threads(),
         host_counted=int(conf.sum()), device_counted=int(ev.confusion.sum()), mean_iou=float(res.mean_iou))


if __name__ == "__main__":
    query_vote()
    confusion()
    whole_repeat()
