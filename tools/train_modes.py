#!/usr/bin/env python
"""Step time of the training precision modes (openscene_amd.train_precision: bf16x6 / bf16x3 / bf16x1) on the two training
configurations of bench.py: the S100k scene through MinkUNet18A and the L235k sweep stack through MinkUNet34C, both DisNet with the
768-d head.  A step = forward + cosine distillation loss on 20 000 rows + backward + FlatAdam, on ONE coordinate manager built before
the timing (the maps do not depend on the mode; bench.py's headline step builds them on a side stream one step ahead).

The three modes run interleaved in one process: ROUNDS (7) rounds, in each round STEPS (10) steps per mode, the mode order rotated
from round to round; per mode the median round and the spread (min, max) of the rounds.  Every mode trains a model of its own from the
same seed, so no mode sees weights another one moved.  Also per mode: the relative L2 of the flat gradient of the FIRST step (same
weights in every mode) against bf16x6's, and the loss after the last timed step.
CONFIGS=S100k,L235k   MODES=bf16x6,bf16x3,bf16x1   OUT=file: one JSON line per (configuration, mode) appended."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import openscene_amd as osn  # noqa: E402
from openscene_amd import synthetic as syn  # noqa: E402
from openscene_amd.disnet import DisNet  # noqa: E402
from openscene_amd.losses import distill_loss  # noqa: E402
from openscene_amd.optim import FlatAdam  # noqa: E402
from openscene_amd.sparse import SparseTensor  # noqa: E402

CONFIGS = {"S100k": ("MinkUNet18A", lambda: syn.shuffled(syn.grid_voxels(syn.room_points(0), 0.02), 0)),
           "L235k": ("MinkUNet34C", lambda: syn.shuffled(syn.grid_voxels(syn.lidar_points(0), 0.05), 0))}


def run_config(name, modes, rounds, steps, dev):
    arch, voxels = CONFIGS[name]

    class Cfg:
        arch_3d = arch
        feature_2d_extractor = "openseg"

    coords = torch.from_numpy(syn.batch_coords([voxels()])).to(dev)
    n = coords.shape[0]
    feats = torch.ones(n, 3, device=dev)
    cm = SparseTensor(feats, coords).coordinate_manager
    g = torch.Generator().manual_seed(7)
    n_sup = min(20000, n)
    sel = torch.randperm(n, generator=g)[:n_sup].sort()[0].to(dev)
    state, first_grad, last_loss = {}, {}, {}
    for m in modes:
        torch.manual_seed(1463)
        model = DisNet(Cfg()).to(dev).train()
        state[m] = (model, FlatAdam(model, lr=1e-4))
    out_dim = state[modes[0]][0].net3d.final.out_channels
    target = torch.nn.functional.normalize(torch.randn(n_sup, out_dim, generator=g), dim=1).half().float().to(dev)

    def one(m, keep_grad=False):
        model, optim = state[m]
        with osn.train_precision(m):
            loss = distill_loss(model(SparseTensor(feats, coordinate_manager=cm)), sel, target)
            optim.zero_grad(set_to_none=True)
            loss.backward()
        if keep_grad:
            first_grad[m] = torch.cat([p.grad.reshape(-1).double() for p in model.parameters()])
        optim.step()
        return loss

    for m in modes:                                   # the first step of every mode: same weights, gradients compared; then warm-up
        one(m, keep_grad=True)
        for _ in range(3):
            one(m)
    torch.cuda.synchronize(dev)
    ms = {m: [] for m in modes}
    for r in range(rounds):
        for m in modes[r % len(modes):] + modes[:r % len(modes)]:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = one(m)
            torch.cuda.synchronize(dev)
            ms[m].append((time.perf_counter() - t0) * 1e3 / steps)
            last_loss[m] = float(loss.detach())
    ref = first_grad.get("bf16x6")
    for m in modes:
        rec = {"tool": "train_modes", "config": name, "arch": arch, "voxels": int(n), "mode": m, "rounds": rounds, "steps": steps,
               "ms_median": round(statistics.median(ms[m]), 4), "ms_min": round(min(ms[m]), 4), "ms_max": round(max(ms[m]), 4),
               "ms_rounds": [round(v, 4) for v in ms[m]], "loss_after": last_loss[m]}
        if ref is not None:
            rec["grad_rel_l2_vs_bf16x6"] = float((first_grad[m] - ref).norm() / ref.norm())
        print(json.dumps(rec), flush=True)
        if os.environ.get("OUT"):
            with open(os.environ["OUT"], "a") as f:
                f.write(json.dumps(rec) + "\n")


def main():
    dev = torch.device("cuda", 0)
    modes = [m for m in os.environ.get("MODES", "bf16x6,bf16x3,bf16x1").split(",") if m]
    rounds, steps = int(os.environ.get("ROUNDS", "7")), int(os.environ.get("STEPS", "10"))
    for name in [c for c in os.environ.get("CONFIGS", "S100k,L235k").split(",") if c]:
        run_config(name, modes, rounds, steps, dev)


if __name__ == "__main__":
    main()
