#!/usr/bin/env python
"""N inference passes (coordinate pyramid + maps + eval-mode forward) of one S100k scene through MinkUNet18A / 768-d -- the workload of
bench.py's `inference_fwd` -- for rocprofv3 (tools/gpu_prof_infer.sh).  PASSES=n, ARCH=...

PRECISION=bf16x6|bf16x3|bf16x1: the inference arithmetic of the passes (openscene_amd.conv_precision; default: the one in force).
MODES=bf16x6,bf16x3,bf16x1: compare modes instead -- ROUNDS (5) rounds, in each round PASSES passes per mode, the modes interleaved
in one process; per mode the median round, the relative L2 of the [N, 768] output against bf16x6's and the share of voxels whose
arg-max over 20 seeded unit text rows agrees with it.  SCENE=S100k (default) | L235k (the 5 cm sweep stack of bench.py's configs[4];
use ARCH=MinkUNet34C).  OUT=file: one JSON line per mode appended."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import openscene_amd as osn  # noqa: E402
from openscene_amd import ops, synthetic as syn  # noqa: E402
from openscene_amd.disnet import DisNet  # noqa: E402
from openscene_amd.sparse import SparseTensor  # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    passes = int(os.environ.get("PASSES", "20"))

    class Cfg:
        arch_3d = os.environ.get("ARCH", "MinkUNet18A")
        feature_2d_extractor = "openseg"

    torch.manual_seed(1463)
    model = DisNet(Cfg()).to(dev).eval()
    scene = os.environ.get("SCENE", "S100k")
    if scene == "L235k":
        vox = syn.shuffled(syn.grid_voxels(syn.lidar_points(0), 0.05), 0)
    else:
        vox = syn.shuffled(syn.grid_voxels(syn.room_points(0), 0.02), 0)
    coords = torch.from_numpy(syn.batch_coords([vox])).to(dev)
    feats = torch.ones(coords.shape[0], 3, device=dev)
    modes = [m for m in os.environ.get("MODES", "").split(",") if m]
    if modes:
        return compare(model, feats, coords, modes, passes, scene, Cfg.arch_3d)
    if os.environ.get("PRECISION"):
        osn.set_conv_precision(os.environ["PRECISION"])
    with torch.no_grad():
        for _ in range(3):
            model(SparseTensor(feats, coords))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(passes):
            model(SparseTensor(feats, coords))
        torch.cuda.synchronize()
    print("inference_fwd %.3f ms per pass (%d passes, %d voxels, %s)" % ((time.perf_counter() - t0) * 1e3 / passes, passes, coords.shape[0],
                                                                         osn.get_conv_precision()), flush=True)


def compare(model, feats, coords, modes, passes, scene, arch):
    rounds = int(os.environ.get("ROUNDS", "5"))
    ms = {m: [] for m in modes}
    outs = {}
    with torch.no_grad():
        for m in modes:
            with osn.conv_precision(m):
                for _ in range(2):
                    outs[m] = model(SparseTensor(feats, coords))
        torch.cuda.synchronize()
        for _ in range(rounds):
            for m in modes:
                with osn.conv_precision(m):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(passes):
                        model(SparseTensor(feats, coords))
                    torch.cuda.synchronize()
                    ms[m].append((time.perf_counter() - t0) * 1e3 / passes)
    text = torch.nn.functional.normalize(torch.randn(20, outs[modes[0]].shape[1], generator=torch.Generator().manual_seed(7)), dim=1)
    text = text.half().to(feats.device)
    ref = outs.get("bf16x6")
    ref_labels = ops.cosine_query(ref, text, want_scores=False)[1] if ref is not None else None
    for m in modes:
        rec = {"tool": "infer_loop", "scene": scene, "arch": arch, "voxels": int(coords.shape[0]), "mode": m, "passes": passes,
               "ms_median": statistics.median(ms[m]), "ms_rounds": [round(v, 4) for v in ms[m]]}
        if ref is not None:
            rec["rel_l2_vs_bf16x6"] = float((outs[m].double() - ref.double()).norm() / ref.double().norm())
            rec["labels_agree"] = float((ops.cosine_query(outs[m], text, want_scores=False)[1] == ref_labels).float().mean())
        print(json.dumps(rec), flush=True)
        if os.environ.get("OUT"):
            with open(os.environ["OUT"], "a") as f:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
