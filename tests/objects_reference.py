"""numpy restatement of openscene_amd.objects (what the object tests compare against), and CPU stand-ins for the kernels
behind it (tests/test_objects_cpu.py).

The definitions, restated independently of the library:
    hit         heat[p, q] finite and float(heat[p, q]) >= thresholds[q]
    voxel       floor(xyz.double() / voxel_size), per scene
    object      a connected component (26 or 6 neighbours) of the voxels that hold a hit; members = the hits of its voxels
    record      n_points, n_voxels, peak_score (max), peak_point (lowest row inside the scene attaining it),
                score_sum = sum(score * 2**24) as integers, vox_sum, float32 box
    selection   n_points >= min_points; peak_score descending, then peak_point ascending; the first max_objects
A dict from voxel to its hits, union-find over the neighbour offsets, python integers for the sums."""
import itertools

import numpy as np
import torch

FIELDS = ("n_points", "n_voxels", "peak_score", "peak_point", "score_sum", "vox_sum", "box_min", "box_max")


def _offsets(connectivity):
    offs = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
    if connectivity == 6:
        offs = [o for o in offs if abs(o[0]) + abs(o[1]) + abs(o[2]) == 1]
    assert len(offs) == connectivity
    return offs


def _components(voxel_of_hit, connectivity):
    """voxel_of_hit: list of (x, y, z) tuples, one per hit -> component number per hit (numbers are arbitrary)."""
    cells = {}
    for i, v in enumerate(voxel_of_hit):
        cells.setdefault(v, []).append(i)
    parent = {v: v for v in cells}

    def find(v):
        root = v
        while parent[root] != root:
            root = parent[root]
        while parent[v] != root:
            parent[v], v = root, parent[v]
        return root

    offs = _offsets(connectivity)
    for v in cells:
        for o in offs:
            u = (v[0] + o[0], v[1] + o[1], v[2] + o[2])
            if u in parent:
                a, b = find(v), find(u)
                if a != b:
                    parent[a] = b
    number = {}
    comp = [0] * len(voxel_of_hit)
    for v, members in cells.items():
        c = number.setdefault(find(v), len(number))
        for i in members:
            comp[i] = c
    return comp, len(number)


def scene_query_objects(cells, xyz32, scores, threshold, connectivity, min_points, max_objects):
    """One scene, one query.  cells int [n, 3]; xyz32 float32 [n, 3]; scores float16 [n] (numpy).
    -> (records kept, best first; number that passed the filter; rank per point or -1)."""
    sf = scores.astype(np.float32)
    hit = np.isfinite(sf) & (sf >= np.float32(threshold))
    idx = np.nonzero(hit)[0]
    point_rank = np.full(scores.shape[0], -1, dtype=np.int32)
    if idx.size == 0:
        return [], 0, point_rank
    vox = [tuple(int(c) for c in cells[i]) for i in idx]
    comp, n_comp = _components(vox, connectivity)
    members = [[] for _ in range(n_comp)]
    for j, c in enumerate(comp):
        members[c].append(j)
    records = []
    for mem in members:
        pts = idx[mem]                                            # ascending rows
        sc = scores[pts]
        best = sc.astype(np.float32).max()
        peak = int(pts[np.nonzero(sc.astype(np.float32) == best)[0][0]])
        records.append({
            "n_points": len(mem),
            "n_voxels": len({vox[j] for j in mem}),
            "peak_score": scores[peak],
            "peak_point": peak,
            "score_sum": sum(int(round(float(s) * 2 ** 24)) for s in sc),        # float(fp16) * 2**24 is an integer
            "vox_sum": [sum(vox[j][a] for j in mem) for a in range(3)],
            "box_min": xyz32[pts].min(0),
            "box_max": xyz32[pts].max(0),
            "points": pts,
        })
    passed = [r for r in records if r["n_points"] >= min_points]
    passed.sort(key=lambda r: (-float(r["peak_score"]), r["peak_point"]))
    kept = passed[:max_objects]
    for rank, r in enumerate(kept):
        point_rank[r["points"]] = rank
    return kept, len(passed), point_rank


def find_objects(xyz, offsets, heat, thresholds, voxel_size=0.05, connectivity=26, min_points=1, max_objects=16, cells=None):
    """The whole result as a dict of CPU tensors shaped like ops.objects_find's (point_object always present).
    xyz float [N, 3], heat fp16 [N, Q] (torch, any device); offsets: S + 1 python ints; thresholds: Q numbers.
    cells: the voxel of every point, when the caller already has it (the stand-in below)."""
    xyz = xyz.detach().cpu()
    heat_np = heat.detach().cpu().numpy()
    n, q_n = heat_np.shape
    s_n = len(offsets) - 1
    m = max_objects
    if cells is None:
        cells = np.floor(xyz.double().numpy() / float(voxel_size)).astype(np.int64)
    xyz32 = xyz.float().numpy()
    thresholds = np.broadcast_to(np.asarray(thresholds, dtype=np.float32).reshape(-1), (q_n,))
    out = {
        "n_points": torch.zeros((s_n, q_n, m), dtype=torch.int64),
        "n_voxels": torch.zeros((s_n, q_n, m), dtype=torch.int64),
        "peak_score": torch.full((s_n, q_n, m), float("-inf"), dtype=torch.float16),
        "peak_point": torch.full((s_n, q_n, m), -1, dtype=torch.int64),
        "score_sum": torch.zeros((s_n, q_n, m), dtype=torch.int64),
        "vox_sum": torch.zeros((s_n, q_n, m, 3), dtype=torch.int64),
        "box_min": torch.zeros((s_n, q_n, m, 3), dtype=torch.float32),
        "box_max": torch.zeros((s_n, q_n, m, 3), dtype=torch.float32),
        "n_objects": torch.zeros((s_n, q_n), dtype=torch.int64),
        "point_object": torch.full((n, q_n), -1, dtype=torch.int32),
    }
    for s in range(s_n):
        a, b = int(offsets[s]), int(offsets[s + 1])
        for q in range(q_n):
            kept, passed, ranks = scene_query_objects(cells[a:b], xyz32[a:b], heat_np[a:b, q], thresholds[q], connectivity,
                                                      min_points, m)
            out["n_objects"][s, q] = passed
            out["point_object"][a:b, q] = torch.from_numpy(ranks)
            for i, r in enumerate(kept):
                out["n_points"][s, q, i] = r["n_points"]
                out["n_voxels"][s, q, i] = r["n_voxels"]
                out["peak_score"][s, q, i] = float(r["peak_score"])
                out["peak_point"][s, q, i] = r["peak_point"]
                out["score_sum"][s, q, i] = r["score_sum"]
                out["vox_sum"][s, q, i] = torch.tensor(r["vox_sum"], dtype=torch.int64)
                out["box_min"][s, q, i] = torch.from_numpy(r["box_min"])
                out["box_max"][s, q, i] = torch.from_numpy(r["box_max"])
    return out


def derived(out, voxel_size):
    """(mean_score, centroid) by the host formulas of the contract."""
    cnt = out["n_points"].double()
    return out["score_sum"].double() / 2 ** 24 / cnt, (out["vox_sum"].double() / cnt[..., None] + 0.5) * float(voxel_size)


def assert_same(result, ref, voxel_size, point_ids=True):
    """Every field of an ObjectResult against the reference dict: exact."""
    for f in FIELDS:
        got = getattr(result, f).cpu()
        want = ref[f]
        assert got.dtype == want.dtype and got.shape == want.shape, (f, got.dtype, got.shape, want.dtype, want.shape)
        if f in ("box_min", "box_max"):
            assert bool((got == want).all()), f                   # (-0 == +0)
        else:
            assert torch.equal(got, want), (f, got[got != want][:8], want[got != want][:8])
    assert torch.equal(result.n_objects.cpu(), ref["n_objects"]), "n_objects"
    mean, cen = derived(ref, voxel_size)
    kept = ref["n_points"] > 0
    assert torch.equal(result.mean_score.cpu()[kept], mean[kept]) and torch.equal(result.centroid.cpu()[kept], cen[kept])
    if point_ids:
        assert result.point_object is not None and torch.equal(result.point_object.cpu(), ref["point_object"]), "point_object"


def wave_groups():
    """Group per point, int64 [197], for the tests of the wave-combined record reduction (csrc/components.h): three full waves
    of 64 consecutive points and one of 5.  Wave 0: groups 0 .. 4 of 1, 3, 4, 5 and 51 lanes (either side of the threshold of
    4 lanes from which a group is merged before the atomics), interleaved by a fixed permutation of the 64 places so that no
    group is a run of neighbours.  Wave 1: 64 lanes on group 5.  Wave 2: groups 6 .. 69, one lane each.  Wave 3: four lanes
    on group 70 around one lane that is left out (-1)."""
    wave0 = np.empty(64, dtype=np.int64)
    wave0[(np.arange(64) * 37 + 11) % 64] = np.repeat(np.arange(5), [1, 3, 4, 5, 51])          # (37 is odd: a permutation)
    return np.concatenate([wave0, np.full(64, 5), np.arange(6, 70), [70, 70, -1, 70, 70]])


# ---- CPU stand-ins for ops.coords_unique / ops.kmap_build / ops.objects_find (host-logic tests only)
def coords_unique(coords4, stride=1):
    from oracle import coords as oc
    uniq, inv, first = oc.unique_first(coords4.numpy())
    return torch.from_numpy(uniq), torch.from_numpy(inv), torch.from_numpy(first.astype(np.int32)), uniq


def kmap_build(table, out_coords4, ksize, offset_scale, with_counts=False, self_map=False):
    from oracle import coords as oc
    return torch.from_numpy(oc.kernel_map(table, out_coords4.numpy(), oc.kernel_offsets(ksize, offset_scale)))


def objects_find(heat, thresholds, xyz, inverse, coords4, nbr, scene_offsets, connectivity=26, min_points=1, max_objects=16,
                 return_point_ids=False, combine=True):
    cells = coords4[inverse.long()][:, 1:].numpy().astype(np.int64)
    out = find_objects(xyz, scene_offsets.tolist(), heat, thresholds.numpy(), connectivity=connectivity, min_points=min_points,
                       max_objects=max_objects, cells=cells)
    if not return_point_ids:
        out["point_object"] = None
    return out
