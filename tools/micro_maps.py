#!/usr/bin/env python
"""Latency of the coordinate pyramid + every kernel map of one S100k scene (what an inference forward pays before its first
convolution; bench.py phase `maps_only`), wall clock over back-to-back builds.  OSN_MAPS_STREAMS=n: map chains on n streams.

    python tools/micro_maps.py [--legacy 0|1] [--reps 30] [--occ-min-probes N]

--legacy 1 runs the launch sequence of the earlier rounds (ops.maps_set_legacy: every self map probed at every offset, the pair
lists' plan a launch of its own); one side per process.  Besides the wall clock it prints, timed with events on the launch stream
(median of --reps), the level-0 5^3 build alone, the 5^3 + 3^3 builds of level 0 from one call, and the osn_maps_build call of
the whole scene; and the pairs of the 5^3 map."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openscene_amd import ops  # noqa: E402
from openscene_amd import synthetic as syn  # noqa: E402
from openscene_amd.sparse import CoordinateManager, SparseTensor  # noqa: E402


def _median_ms(fn, reps):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0]


def level0_builds(coords, reps, dev):
    """The level-0 self maps by themselves: one ops.maps_build call with the 5^3 job, one with the 5^3 and the 3^3 job."""
    cm = CoordinateManager(coords)
    x, table, n = cm.coords(1), cm._tables[1], cm.size(1)
    occ = torch.empty(ops.maps_occupancy_bytes(n), dtype=torch.uint8, device=dev)
    bufs = {k: (torch.empty((k ** 3, n), dtype=torch.int32, device=dev), torch.empty(k ** 3, dtype=torch.int64, device=dev)) for k in (5, 3)}

    def call(ksizes):
        jobs = [dict(lvl_in=0, lvl_out=0, ksize=k, scale=1, self_map=1, stream=0, nbr_fwd=bufs[k][0], counts=bufs[k][1]) for k in ksizes]
        ops.maps_build([(x, table, n)], jobs, dev, 0, streams=1, occ=[occ])
    for name, ks in (("5^3", (5,)), ("5^3 + 3^3", (5, 3)), ("3^3", (3,))):
        med, lo = _median_ms(lambda: call(ks), reps)
        print("level 0 %-10s build (presets included): median %.4f ms, min %.4f ms" % (name, med, lo), flush=True)
    print("pairs of the 5^3 map: %d, of the 3^3 map: %d (%d rows)" % (int(bufs[5][1].sum()), int(bufs[3][1].sum()), n), flush=True)
    tl = ops.tile_lists(bufs[3][0])

    def pairs():
        tl.pairs = None
        ops.pair_lists(tl)
    med, lo = _median_ms(pairs, reps)
    print("level 0 3^3 pair lists (osn_pair_lists_build): median %.4f ms, min %.4f ms" % (med, lo), flush=True)


def whole_call(feats, coords, reps):
    """The osn_maps_build call of a training step's prebuild (pairs=True), bracketed by events on the launch stream."""
    real = ops.maps_build
    spans = []

    def timed(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real(*a, **k)
        e1.record()
        spans.append((e0, e1))
    ops.maps_build = timed
    try:
        for _ in range(reps + 3):
            SparseTensor(feats, coords).coordinate_manager.prebuild(pairs=True)
            torch.cuda.synchronize()
    finally:
        ops.maps_build = real
    t = sorted(a.elapsed_time(b) for a, b in spans[3:])
    print("osn_maps_build of the scene (pairs=True): median %.4f ms, min %.4f ms, max %.4f ms" % (t[len(t) // 2], t[0], t[-1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legacy", type=int, default=0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--occ-min-probes", type=int, default=None, help="CoordinateManager.OCC_MIN_PROBES (which levels get occupancy)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    vox = syn.shuffled(syn.grid_voxels(syn.room_points(0), 0.02), 0)
    coords = torch.from_numpy(syn.batch_coords([vox])).to(dev)
    feats = torch.ones(coords.shape[0], 3, device=dev)
    ops.maps_set_legacy(bool(args.legacy))
    if args.occ_min_probes is not None:
        CoordinateManager.OCC_MIN_PROBES = args.occ_min_probes
    print("legacy=%d OCC_MIN_PROBES=%d" % (args.legacy, CoordinateManager.OCC_MIN_PROBES), flush=True)
    level0_builds(coords, args.reps, dev)
    whole_call(feats, coords, args.reps)
    for grad in (False, "ws", True):
        def build():
            SparseTensor(feats, coords).coordinate_manager.prebuild(pairs=grad)
        for _ in range(3):
            build()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            build()
        torch.cuda.synchronize()
        print("OSN_MAPS_STREAMS=%s pairs=%s: %.3f ms per scene" % (os.environ.get("OSN_MAPS_STREAMS", "1"), grad, (time.perf_counter() - t0) * 50), flush=True)


if __name__ == "__main__":
    main()
