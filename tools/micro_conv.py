#!/usr/bin/env python
"""Micro-benchmark of the dominant convolution launches on the S100k scene (for rocprofv3
--pmc passes): level-0 3^3 conv 96->96 forward (tile-ordered map), its weight gradient, and the
level-1 128->96 pair.  Prints HIP-event times.

ONLY=pieces: the inference precision modes (openscene_amd.precision: pieces 3 / 2 / 1 = bf16x6 / bf16x3 / bf16x1) on the dominant
forward shapes of S100k / MinkUNet18A, one per kernel family -- tile-list 3^3 96 -> 96 at 100 999 rows, register-gather 3^3 32 -> 64 on
the 13 k-row level, weight-stationary 3^3 256 -> 256 on the level-3 map, the 96 -> 768 head -- the three modes interleaved in one process
(ROUNDS rounds of REPS launches each, median round).  One JSON line per (shape, mode): time, the bf16 MFMA work it issued
(pairs x cin x cout x 2 x products) as a fraction of the 2.5 PFLOP/s dense bf16 roof, and the fp32-equivalent rate.  OUT=file appends.
Then the same for the pair-array weight gradient in the training modes (family "wgrad_tl"): 3^3 96 -> 96 at 100 999 rows, the 2^3
256 -> 128 transposed convolution between the two deepest levels (a swap launch) and a 1x1 128 -> 128 shortcut (identity map)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openscene_amd import ops, synthetic as syn  # noqa: E402
from openscene_amd.sparse import CoordinateManager  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


BF16_PEAK_TFLOPS = 2500.0      # dense bf16 MFMA peak (bench.py)
PRODUCTS = {3: 6, 2: 3, 1: 1}


def pieces_modes(cm, dev, reps):
    rounds = int(os.environ.get("ROUNDS", "5"))
    cases = []
    # (family, stride, kernel size, cin, cout)
    for fam, stride, ks, cin, cout in (("tl", 1, 3, 96, 96), ("rg", 4, 3, 32, 64), ("ws", 8, 3, 256, 256), ("dense", 1, 1, 96, 768)):
        n = cm.size(stride)
        x = torch.randn(n, cin, device=dev)
        K = ks ** 3
        w = torch.randn(K, cin, cout, device=dev) * 0.05
        wf, _ = ops.weight_prep_tl(w, want_dgrad=False)
        if fam == "dense":
            pairs = n
            run = lambda p, x=x, wf=wf, cout=cout: ops.dense_fwd(x, wf, cout, pieces=p)
        else:
            nbr = cm.kmap(stride, stride, ks)[0]
            pairs = int(ops.kmap_count(nbr).sum())
            tiles = cm.kmap_tiles(stride, stride, ks)[0]
            tbl, rows = (tiles[1], tiles[0]) if tiles is not None else (nbr, None)
            if fam == "rg":
                assert ops.rg_eligible(K, cin, cout, n)
                run = lambda p, x=x, wf=wf, tbl=tbl, rows=rows, n=n, cout=cout: ops.spconv_fwd_rg(x, wf, tbl, n, cout, out_rows=rows, pieces=p)
            else:
                tl = ops.tile_lists(tbl, out_rows=rows)
                if fam == "tl":
                    run = lambda p, x=x, wf=wf, tl=tl, n=n, K=K, cout=cout: ops.spconv_fwd_tl(x, wf, tl, n, K, cout, pieces=p)
                else:
                    run = lambda p, x=x, wf=wf, tl=tl, nbr=nbr, n=n, K=K, cout=cout: ops.spconv_fwd_ws(x, wf, tl, nbr, n, K, cout, pieces=p)
        cases.append((fam, "s%d k%d %d->%d" % (stride, ks, cin, cout), n, pairs, cin, cout, run))
    # the pair-array weight gradient: (stride of the input rows, stride of the output-gradient rows, kernel size, cin, cout)
    for s_in, s_out, ks, cin, cout in ((1, 1, 3, 96, 96), (16, 8, 2, 256, 128), (2, 2, 1, 128, 128)):
        n_in, n = cm.size(s_in), cm.size(s_out)
        x, g = torch.randn(n_in, cin, device=dev), torch.randn(n, cout, device=dev)
        K = ks ** 3
        if ks == 1:
            pairs, tl, swap = n, None, False
        elif s_in > s_out:            # transposed: the arrays of the strided convolution it mirrors, walked the other way
            pairs, tl, swap = int(ops.kmap_count(cm.kmap(s_out, s_in, ks)[0]).sum()), cm.kmap_lists(s_out, s_in, ks)[0], True
        else:
            pairs, tl, swap = int(ops.kmap_count(cm.kmap(s_in, s_out, ks)[0]).sum()), cm.kmap_lists(s_in, s_out, ks)[0], False
        run = lambda p, x=x, g=g, tl=tl, K=K, swap=swap: ops.spconv_wgrad_tl(x, g, tl, K, swap=swap, pieces=p)
        cases.append(("wgrad_tl", "s%d->s%d k%d %d->%d" % (s_in, s_out, ks, cin, cout), n, pairs, cin, cout, run))
    for fam, shape, n, pairs, cin, cout, run in cases:
        us = {p: [] for p in (3, 2, 1)}
        ref = run(3)
        err = {p: ((run(p) - ref).norm() / ref.norm()).item() for p in (3, 2, 1)}
        for _ in range(rounds):
            for p in (3, 2, 1):
                us[p].append(timed(lambda: run(p), reps))
        for p in (3, 2, 1):
            t = statistics.median(us[p])
            fl = 2.0 * pairs * cin * cout
            rec = {"tool": "micro_conv", "family": fam, "shape": shape, "rows": n, "pairs": pairs, "mode": {3: "bf16x6", 2: "bf16x3", 1: "bf16x1"}[p],
                   "us_median": round(t, 2), "us_rounds": [round(v, 2) for v in us[p]], "reps": reps,
                   "bf16_mfma_roof_frac": round(fl * PRODUCTS[p] / (t * 1e-6) / (BF16_PEAK_TFLOPS * 1e12), 4),
                   "fp32_equiv_TFLOPs": round(fl / t / 1e6, 1), "rel_l2_vs_bf16x6": err[p]}
            print(json.dumps(rec), flush=True)
            if os.environ.get("OUT"):
                with open(os.environ["OUT"], "a") as f:
                    f.write(json.dumps(rec) + "\n")


def main():
    reps = int(os.environ.get("REPS", "3"))
    dev = torch.device("cuda", 0)
    vox = syn.shuffled(syn.grid_voxels(syn.room_points(0), 0.02), 0)
    cm = CoordinateManager(torch.from_numpy(syn.batch_coords([vox])).to(dev))
    only = os.environ.get("ONLY", "")
    if only == "pieces":
        return pieces_modes(cm, dev, max(reps, 20))
    shapes = ((1, 96, 96), (2, 128, 96), (1, 128, 96))
    if only:
        shapes = shapes[:1]
    for stride, cin, cout in shapes:
        n = cm.size(stride)
        nbr = cm.kmap(stride, stride, 3)[0]
        order, tbl, gm = ops.kmap_sort(nbr, cm.kmap_counts(stride, stride, 3))
        pairs = int(ops.kmap_count(nbr).sum())
        x = torch.randn(n, cin, device=dev)
        w = torch.randn(27, cin, cout, device=dev) * 0.05
        g = torch.randn(n, cout, device=dev)
        if only == "fwd":
            print("fwd(tile-ordered) %.1f us" % timed(lambda: ops.spconv_fwd(x, w, tbl, n, out_rows=order, gmask=gm), reps))
            continue
        if only == "fwd_x6":
            wp = ops.weight_prep_x6(w)
            print("fwd_x6(tile-ordered) %.1f us" % timed(
                lambda: ops.spconv_fwd_x6(x, wp, tbl, n, out_rows=order, gmask=gm), reps))
            continue
        if only == "wgrad":
            cnt = ops.kmap_count(nbr)
            print("wgrad(balanced) %.1f us" % timed(lambda: ops.spconv_wgrad(x, g, nbr, 27, cnt), reps))
            continue
        wp = ops.weight_prep_x6(w)
        t_x6 = timed(lambda: ops.spconv_fwd_x6(x, wp, tbl, n, out_rows=order, gmask=gm), reps)
        t_prep = timed(lambda: ops.weight_prep_x6(w), reps)
        ref = ops.spconv_fwd(x, w, tbl, n, out_rows=order, gmask=gm)
        got = ops.spconv_fwd_x6(x, wp, tbl, n, out_rows=order, gmask=gm)
        print("   bf16x6 fwd %.1f us (+ weight prep %.1f us), max|d| vs fp32 kernel = %.2e of max" % (
            t_x6, t_prep, (got - ref).abs().max().item() / ref.abs().max().item()))
        t_fwd_sorted = timed(lambda: ops.spconv_fwd(x, w, tbl, n, out_rows=order, gmask=gm), reps)
        t_fwd_plain = timed(lambda: ops.spconv_fwd(x, w, nbr, n), reps)
        cnt = ops.kmap_count(nbr)
        t_wgrad = timed(lambda: ops.spconv_wgrad(x, g, nbr, 27, cnt), reps)
        t_wgrad_u = timed(lambda: ops.spconv_wgrad(x, g, nbr, 27), reps)
        fl = 2.0 * pairs * cin * cout
        print("stride %d  N=%d pairs=%d  %d->%d : fwd(tile-ordered) %.1f us = %.1f TF exact | fwd(hash order) %.1f us | "
              "wgrad(balanced) %.1f us = %.1f TF | wgrad(uniform) %.1f us" % (
                  stride, n, pairs, cin, cout, t_fwd_sorted, fl / t_fwd_sorted / 1e6, t_fwd_plain, t_wgrad,
                  fl / t_wgrad / 1e6, t_wgrad_u))


if __name__ == "__main__":
    main()
