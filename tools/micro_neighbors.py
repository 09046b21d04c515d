"""Cost of the spatial-neighbour kernels (csrc/neighbors.hip) against the same results written with what torch offers, measured
in the same process:

  knn_self      ops.knn_grid over the grid's own points (cells from grid.nbr / grid.inverse), k = 1 and 8
  knn           150 k foreign queries per scene, jittered copies of the points, k = 1 and 8: the kernel alone (`us_kernel`) and
                PointIndex.knn as a user calls it (`us_call`: the floor, ops.coords_unique, ops.kmap_build and the sort of the
                queries by cell in front of the kernel, and the read of the error word behind it)
  fill_missing  a 32-column fp16 heat-map with 30 % of the rows unseen: the whole call (index over the seen points, search,
                blend, select) and the blend kernel alone
  transfer      768-d fp16 rows to the foreign queries: the blend kernel at k = 1 uniform and k = 4 inverse, and the whole call
  torch route   per scene, in chunks of CHUNK queries: torch.cdist against the scene's points, topk (smallest k), the radius
                mask, and -- for fill_missing / transfer -- a gather of the rows and the weighted mean

    python tools/micro_neighbors.py [iters] [out.jsonl]

8 scenes x 150 k points (openscene_amd.synthetic rooms), 5 cm voxels, radius 5 cm.  Ours: HIP events around windows of about a
quarter of a second of back-to-back calls after a warm-up, the median of three rounds (rounds_us keeps all of them).  The
torch route takes seconds per pass (it forms N x M distances per scene): one warm-up on the first scene, then TORCH_PASSES
whole passes, each timed between events (torch_passes_us keeps all of them).  `bytes_requested` is what the lanes of the kernel
ask for, from the formula below -- per query its row, column, place and 27 table entries, 16 bytes per candidate, the outputs;
for a blend the gathered rows, the output rows and the lists -- not what reaches HBM: the lanes of a wave share most lines.
The two routes are compared: rows whose neighbour lists differ are counted (torch's cdist is not the kernel's float32 chain,
so near-ties and points at the radius may differ).  One JSON object per line (also appended to out.jsonl when given)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import neighbors as N                             # noqa: E402
from openscene_amd import ops                                        # noqa: E402
from openscene_amd import synthetic as syn                           # noqa: E402
from openscene_amd.objects import VoxelGrid                          # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
OUT = sys.argv[2] if len(sys.argv) > 2 else None
dev = torch.device("cuda", 0)
ROUNDS = 3
WINDOW_US = 250_000.0
SCENES, POINTS, VOXEL = 8, 150_000, 0.05
JITTER = 0.01
CHUNK = 4096
TORCH_PASSES = 2


def events_us(f, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def rounds(f):
    """us per call: a warm-up, then ROUNDS windows of about WINDOW_US (at most ITERS * 50 calls) between device events;
    (median, all rounds, calls per window)."""
    f()
    f()
    torch.cuda.synchronize()
    iters = max(3, min(ITERS * 50, int(WINDOW_US / max(events_us(f, 3), 1.0))))
    got = [events_us(f, iters) for _ in range(ROUNDS)]
    return statistics.median(got), got, iters


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as fh:
            fh.write(line + "\n")


def knn_bytes(index, nbr, q_cell, m, k):
    """(candidates, bytes the lanes request): see the module text."""
    per_cell = (index.cell_start[1:] - index.cell_start[:-1]).long()
    rows = nbr.long()
    per_column = torch.where(rows >= 0, per_cell[rows.clamp(min=0)], torch.zeros_like(rows)).sum(0)
    cand = int(torch.where(q_cell >= 0, per_column[q_cell.long().clamp(min=0)], torch.zeros_like(q_cell, dtype=torch.int64)).sum())
    return cand, m * (12 + 4 + 4 + 27 * 4 + 4 + 8 * k) + 16 * cand


def blend_bytes(count, m, k, cols, esize):
    return int(count.sum()) * cols * esize + m * cols * esize + m * (8 * k + 4 + 1)


def torch_knn(xyz, offsets, query, q_offsets, k, radius, scenes=None):
    """(idx int64 [M, k] (-1 beyond the radius), d float32 [M, k]) by cdist + topk per scene and chunk."""
    idx = torch.full((query.shape[0], k), -1, dtype=torch.int64, device=dev)          # (rows of scenes left out: no neighbour)
    dist = torch.zeros((query.shape[0], k), dtype=torch.float32, device=dev)
    for s in (range(len(offsets) - 1) if scenes is None else scenes):
        pts = xyz[offsets[s]:offsets[s + 1]]
        for a in range(q_offsets[s], q_offsets[s + 1], CHUNK):
            b = min(a + CHUNK, q_offsets[s + 1])
            d, i = torch.cdist(query[a:b], pts).topk(k, dim=1, largest=False)
            keep = d <= radius
            idx[a:b] = torch.where(keep, i + offsets[s], torch.full_like(i, -1))
            dist[a:b] = d
    return idx, dist


def torch_blend(values, idx, dist, inverse, eps):
    """The weighted mean of the gathered rows, chunked like the search."""
    out = torch.zeros((idx.shape[0], values.shape[1]), dtype=values.dtype, device=dev)
    for a in range(0, idx.shape[0], CHUNK):
        i, d = idx[a:a + CHUNK], dist[a:a + CHUNK]
        w = (i >= 0).float() * (1.0 / (d * d + eps) if inverse else 1.0)
        rows = values[i.clamp(min=0)].float()
        out[a:a + CHUNK] = ((w[..., None] * rows).sum(1) / w.sum(1, keepdim=True).clamp(min=1e-30)).to(values.dtype)
    return out


def torch_passes(f, warm):
    """([us of each whole pass], the last pass's result)."""
    warm()
    torch.cuda.synchronize()
    kept = []
    return [events_us(lambda: kept.append(f()), 1) for _ in range(TORCH_PASSES)], kept[-1]


def differing(ours_idx, theirs_idx):
    return int((ours_idx.long() != theirs_idx).any(1).sum())


def main():
    rng = np.random.default_rng(0)
    scenes = [syn.room_points(s, n_pts=POINTS).astype(np.float32) for s in range(SCENES)]
    offsets = [0]
    for x in scenes:
        offsets.append(offsets[-1] + x.shape[0])
    xyz = torch.from_numpy(np.concatenate(scenes, 0)).to(dev)
    n = xyz.shape[0]
    grid = VoxelGrid(xyz, offsets, voxel_size=VOXEL)
    index = N.PointIndex(grid)
    query = (xyz + torch.from_numpy(rng.normal(0.0, JITTER, (n, 3)).astype(np.float32)).to(dev)).contiguous()
    scene = torch.repeat_interleave(torch.arange(SCENES, device=dev), POINTS)
    r2 = N._radius(None, VOXEL)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    common = dict(scenes=SCENES, points=n, voxels=grid.n_voxels, voxel_size=VOXEL, radius=VOXEL, window_us=WINDOW_US, chunk=CHUNK)

    # ---- the search, own points and foreign queries
    nbr_f, q_cell_f, order_f = index.query_cells(query, scene)
    lists = {}
    for kind, q, nbr, q_cell, order in (("knn_self", grid.xyz, grid.nbr, grid.inverse, index._self_order), ("knn", query, nbr_f, q_cell_f, order_f)):
        for k in (1, 8):
            kernel = lambda: ops.knn_grid(grid.xyz, index.cell_start, index.cell_points, nbr, q, q_cell, k, r2, order=order, err=err)
            call = (lambda: index.knn_self(k)) if kind == "knn_self" else (lambda: index.knn(q, k, scene=scene))
            ours = kernel()
            us_kernel, spread, iters = rounds(kernel)
            us_call, spread_call, _ = rounds(call)
            ops.knn_check(err)
            passes, theirs = torch_passes(lambda: torch_knn(xyz, offsets, q, offsets, k, VOXEL), lambda: torch_knn(xyz, offsets, q, offsets, k, VOXEL, scenes=[0]))
            cand, nbytes = knn_bytes(index, nbr, q_cell, n, k)
            lists[(kind, k)] = ours
            emit(kind=kind, k=k, queries=n, cells=int(nbr.shape[1]), candidates=cand, neighbours=int(ours[2].sum()),
                 bytes_requested=nbytes, us_kernel=us_kernel, bytes_requested_per_s=nbytes / (us_kernel * 1e-6), us_call=us_call,
                 us_torch=statistics.median(passes), torch_over_kernel=statistics.median(passes) / us_kernel,
                 torch_over_call=statistics.median(passes) / us_call, rows_differing_between_routes=differing(ours[0], theirs[0]),
                 rounds_us=spread, rounds_call_us=spread_call, torch_passes_us=passes, calls_per_window=iters, **common)
            del theirs

    # ---- fill_missing: a 32-column heat-map, 30 % unseen
    gen = torch.Generator(device=dev).manual_seed(1)
    heat = torch.rand((n, 32), generator=gen, device=dev).half()
    seen = torch.rand(n, generator=gen, device=dev) >= 0.3
    holed = torch.where(seen[:, None], heat, torch.zeros_like(heat))
    k = 4
    eps = float(np.float32((1e-3 * VOXEL) ** 2))
    seen_index = N.PointIndex(grid, seen)
    nb = seen_index.knn_self(k)
    blend = lambda: ops.knn_blend(holed, nb.idx, nb.dist2, nb.count, inverse=True, eps=eps, err=err)
    us_blend, spread, iters = rounds(blend)
    us_call, spread_call, _ = rounds(lambda: N.fill_missing(grid, holed, seen, k=k))
    ops.knn_check(err)
    seen_ids = torch.nonzero(seen).reshape(-1)
    seen_offsets = [int((seen_ids < o).sum()) for o in offsets]
    seen_xyz = xyz[seen_ids].contiguous()

    def torch_fill(scenes=None):
        i, d = torch_knn(seen_xyz, seen_offsets, xyz, offsets, k, VOXEL, scenes=scenes)
        i = torch.where(i >= 0, seen_ids[i.clamp(min=0)], i)
        return torch.where(seen[:, None], holed, torch_blend(holed, i, d, True, eps))

    passes, _ = torch_passes(torch_fill, lambda: torch_fill(scenes=[0]))
    nbytes = blend_bytes(nb.count, n, k, 32, 2)
    emit(kind="fill_missing", k=k, columns=32, dtype="float16", unseen=int((~seen).sum()), still_missing=int(N.fill_missing(grid, holed, seen, k=k)[1].sum()),
         blend_bytes_requested=nbytes, us_blend=us_blend, blend_bytes_requested_per_s=nbytes / (us_blend * 1e-6), us_call=us_call,
         us_torch=statistics.median(passes), torch_over_call=statistics.median(passes) / us_call, rounds_us=spread, rounds_call_us=spread_call,
         torch_passes_us=passes, calls_per_window=iters, **common)
    del heat, holed

    # ---- transfer: 768-d fp16 rows to the foreign queries
    feats = torch.randn((n, 768), generator=gen, device=dev).half()
    for k, weights in ((1, "uniform"), (4, "inverse")):
        nb = index.knn(query, k, scene=scene)
        blend = lambda: ops.knn_blend(feats, nb.idx, nb.dist2, nb.count, inverse=weights == "inverse", eps=eps, err=err)
        us_blend, spread, iters = rounds(blend)
        us_call, spread_call, _ = rounds(lambda: N.transfer(index, query, feats, k=k, weights=weights, scene=scene))
        ops.knn_check(err)

        def torch_transfer(scenes=None):
            i, d = torch_knn(xyz, offsets, query, offsets, k, VOXEL, scenes=scenes)
            return torch_blend(feats, i, d, weights == "inverse", eps)

        passes, _ = torch_passes(torch_transfer, lambda: torch_transfer(scenes=[0]))
        nbytes = blend_bytes(nb.count, n, k, 768, 2)
        emit(kind="transfer", k=k, weights=weights, columns=768, dtype="float16", queries=n, found=int((nb.count > 0).sum()),
             blend_bytes_requested=nbytes, us_blend=us_blend, blend_bytes_requested_per_s=nbytes / (us_blend * 1e-6), us_call=us_call,
             us_torch=statistics.median(passes), torch_over_call=statistics.median(passes) / us_call, rounds_us=spread,
             rounds_call_us=spread_call, torch_passes_us=passes, calls_per_window=iters, **common)


if __name__ == "__main__":
    main()
