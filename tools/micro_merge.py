"""Cost of merging regions by mean feature (csrc/merge.hip, openscene_amd.merge) against the same steps written with what
torch offers, measured in the same process:

  contacts   ops.regions_contacts alone (the key array; torch.unique on top of it is timed as `adjacency`)
  pair_dot   ops.rows_pair_dot on the first round's pair list, with the bytes it must read -- (E + distinct lo rows) * 2 d: a hi
             row per pair, a lo row once per run of pairs that share it -- plus the sims written, as a fraction of the HBM roof
  round      ops.regions_merge_round on the same list (preset, best, unite, flatten)
  fold       ops.rows_fold of the first round's groups
  merge      the whole merge_regions from a cut at two thresholds, with its rounds and the regions before and after
  torch      the pair sims as a gather of both rows and (a * b).sum(-1) in slices, the best neighbour by
             scatter_reduce(amax) over 64-bit keys and the star by index arithmetic, the fold by index_add_

    python tools/micro_merge.py [iters] [out.jsonl]

8 scenes x 150 k points x 768 features and the clusters of tools/micro_regions.py (5 cm voxels), both bank kinds.  HIP events
around windows of about a quarter of a second of back-to-back calls after a warm-up; the variants alternate and the median of
three rounds is reported (rounds_us keeps all of them).  Working sets under 256 MB are re-read from the last-level cache between
calls of a window: the region rows of a cut with a few hundred thousand regions are larger than that, the pair list, the sims
and the parent words are not.  One JSON object per line (also appended to out.jsonl when given)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import micro_regions as mreg                                         # noqa: E402  (the case, the timing windows, emit)
from openscene_amd import merge as M                                 # noqa: E402
from openscene_amd import ops                                        # noqa: E402
from openscene_amd import regions as R                               # noqa: E402
from openscene_amd import synthetic as syn                           # noqa: E402
from openscene_amd.objects import VoxelGrid                          # noqa: E402
from openscene_amd.search import FeatureBank                         # noqa: E402

dev = mreg.dev
D = mreg.D
CUTS = (0.95, 0.9)               # the over-segmentations the merge starts from
SIMILARITY = 0.7
SLICE = 1 << 17                  # pairs per slice of the torch pair sims: bounds its float32 temporaries


def torch_pair_dot(x, lo, hi):
    out = torch.empty(lo.shape[0], dtype=torch.float32, device=dev)
    for a in range(0, lo.shape[0], SLICE):
        out[a:a + SLICE] = (x[lo[a:a + SLICE].long()].float() * x[hi[a:a + SLICE].long()].float()).sum(-1)
    return out


def torch_round(lo, hi, sim, r, thr):
    """A representative per region after one star round (any member of the group; the kernel gives the smallest)."""
    lo, hi = lo.long(), hi.long()
    e = torch.arange(lo.shape[0], device=dev)
    bits = sim.view(torch.int32).long()
    mono = torch.where(bits >= 0, bits, -(bits & 0x7FFFFFFF)) + (1 << 31)    # ascending with the float, 0 .. 2^32
    key = torch.where(sim >= thr, (mono << 31) | ((1 << 31) - 1 - e), torch.full_like(mono, -1))
    best = torch.full((r,), -1, dtype=torch.int64, device=dev)
    best.scatter_reduce_(0, lo, key, "amax")
    best.scatter_reduce_(0, hi, key, "amax")
    some = best >= 0
    edge = ((1 << 31) - 1 - (best & ((1 << 31) - 1))).clamp(0, max(lo.shape[0] - 1, 0))
    ids = torch.arange(r, device=dev)
    other = torch.where(lo[edge] == ids, hi[edge], lo[edge])
    other = torch.where(some, other, ids)
    mutual = some & (best[other] == best)
    centre = torch.where(mutual, torch.minimum(ids, other), ids)
    return torch.where(mutual, centre, torch.where(some & mutual[other], centre[other], ids))


def torch_fold(total, new_id, g):
    return torch.zeros((g, total.shape[1]), dtype=torch.float32, device=dev).index_add_(0, new_id, total)


def wall_us(f, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6 / calls


def case(scenes, n, gen):
    rooms = [torch.from_numpy(syn.room_points(s, n_pts=n)) + torch.tensor([6.0 * s, 0.0, 0.0], dtype=torch.float64) for s in range(scenes)]
    xyz = torch.cat(rooms, 0).to(dev)
    offsets = [i * n for i in range(scenes + 1)]
    grid = VoxelGrid(xyz, offsets, voxel_size=mreg.VS)
    feats = mreg.planted_features(grid.xyz, offsets, gen)
    for dtype in ("fp16", "fp8"):
        bank = FeatureBank(D, dev, capacity_rows=scenes * n, dtype=dtype)
        for s in range(scenes):
            bank.add_scene("s%d" % s, feats[offsets[s]:offsets[s + 1]])
        graph = R.SimilarityGraph(bank, grid)
        for cut_at in CUTS:
            cut = graph.segment(cut_at)
            r = cut.n_regions
            lo, hi, contacts = M.region_adjacency(grid, cut.voxel_region, r)
            e = lo.shape[0]
            total = cut.descriptors(bank).sum
            x = M.unit_rows(total)
            sim = ops.rows_pair_dot(x, lo, hi)
            parent = ops.regions_merge_round(lo, hi, sim, r, SIMILARITY).long()
            number = torch.cumsum(parent == torch.arange(r, device=dev), 0) - 1
            new_id = number[parent]
            g = int(number[-1]) + 1
            members = torch.sort(new_id, stable=True)[1].to(torch.int32)
            starts = torch.zeros(g + 1, dtype=torch.int64, device=dev)
            starts[1:] = torch.cumsum(torch.bincount(new_id, minlength=g), 0)
            # the torch route gives the same sims (to rounding), the same groups and the same sums (to rounding)
            ref = torch_pair_dot(x, lo, hi)
            assert float((ref - sim).abs().max()) < 1e-4
            rep = torch_round(lo, hi, sim, r, SIMILARITY)
            assert torch.equal(rep[parent], rep) and torch.equal(parent[rep], parent) and int((rep == torch.arange(r, device=dev)).sum()) == g
            folded = ops.rows_fold(total, starts, members)
            assert float((torch_fold(total, new_id, g) - folded).abs().max()) <= 1e-3 * float(folded.abs().max())
            distinct_lo = int((lo[1:] != lo[:-1]).sum()) + 1 if e else 0
            bytes_dot = (e + distinct_lo) * D * 2 + e * 12
            (us_contacts, us_adjacency, us_dot, us_round, us_fold, us_unit, us_tdot, us_tround, us_tfold), spread, iters = mreg.rounds([
                lambda: ops.regions_contacts(cut.voxel_region, grid.nbr, 26, r),
                lambda: M.region_adjacency(grid, cut.voxel_region, r),
                lambda: ops.rows_pair_dot(x, lo, hi),
                lambda: ops.regions_merge_round(lo, hi, sim, r, SIMILARITY),
                lambda: ops.rows_fold(total, starts, members),
                lambda: M.unit_rows(total),
                lambda: torch_pair_dot(x, lo, hi),
                lambda: torch_round(lo, hi, sim, r, SIMILARITY),
                lambda: torch_fold(total, new_id, g)])
            mreg.emit(kind="merge_steps", bank=dtype, scenes=scenes, rows_per_scene=n, d=D, voxels=grid.n_voxels, cut=cut_at,
                      similarity=SIMILARITY, regions=r, pairs=e, distinct_lo_rows=distinct_lo, pairs_per_lo=e / max(distinct_lo, 1),
                      max_pairs_of_a_region=int(torch.bincount(torch.cat([lo, hi]).long()).max()) if e else 0,
                      groups_after_round=g, rows_bytes=r * D * 2, pair_dot_bytes=bytes_dot, us_contacts=us_contacts,
                      us_adjacency=us_adjacency, us_pair_dot=us_dot, pair_dot_bytes_per_s=bytes_dot / (us_dot * 1e-6),
                      pair_dot_fraction_of_hbm_roof=bytes_dot / (us_dot * 1e-6) / mreg.HBM_ROOF, us_round=us_round, us_fold=us_fold,
                      fold_bytes_per_s=(r + g) * D * 4 / (us_fold * 1e-6), us_unit_rows=us_unit, us_torch_pair_dot=us_tdot,
                      us_torch_round=us_tround, us_torch_fold=us_tfold, torch_over_pair_dot=us_tdot / us_dot,
                      torch_over_round=us_tround / us_round, torch_over_fold=us_tfold / us_fold, rounds_us=spread,
                      calls_per_window=iters, window_us=mreg.WINDOW_US, hbm_roof_bytes_per_s=mreg.HBM_ROOF)
            # the whole loop: device events and the wall clock (the loop reads back once per round: host-bound when they differ)
            res = M.merge_regions(bank, grid, cut, similarity=SIMILARITY)
            us_events = mreg.events_us(lambda: M.merge_regions(bank, grid, cut, similarity=SIMILARITY), 3)
            us_wall = wall_us(lambda: M.merge_regions(bank, grid, cut, similarity=SIMILARITY), 3)
            us_sums = mreg.events_us(lambda: cut.descriptors(bank), 3)
            us_records = mreg.events_us(lambda: ops.regions_records(res.voxel_region, res.n_regions, grid.xyz, grid.inverse, grid.coords), 3)
            mreg.emit(kind="merge", bank=dtype, scenes=scenes, rows_per_scene=n, voxels=grid.n_voxels, cut=cut_at, similarity=SIMILARITY,
                      regions_before=r, regions_after=res.n_regions, rounds=res.rounds, converged=res.converged, history=res.history,
                      us_merge_events=us_events, us_merge_wall=us_wall, us_region_sums=us_sums, us_records=us_records, calls=3)
            del total, x, sim, ref, folded
        del bank, graph


if __name__ == "__main__":
    g = torch.Generator(device=dev).manual_seed(1)
    np.random.seed(0)
    case(8, 150_000, g)
