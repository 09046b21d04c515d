"""Kernel maps that probe occupied cells only, the 3^3 table copied out of the 5^3 one, the pair lists' plan inside the fill launch:
every product against the launch sequence of the earlier rounds (ops.maps_set_legacy) and against oracle/coords.py, element for
element.  The maps come from ops.maps_build over an arena preset to one byte, so the buffers compare byte for byte."""
import numpy as np
import pytest
import torch

from oracle import coords as oc
from openscene_amd import synthetic as syn

pytestmark = pytest.mark.gpu

FILL = 0x5A


def dev():
    return torch.device("cuda", 0)


def _rows(xyz, batch=0):
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([np.full((xyz.shape[0], 1), batch), xyz], 1).astype(np.int32)


def _axis(a, v):
    p = [0, 0, 0]
    p[a] = v
    return p


def _cases():
    rng = np.random.default_rng(7)
    cases = {"one_row": _rows([[5, -3, 2]])}
    for a in range(3):
        for d in (2, 3):                                               # inside / outside a 5^3 neighbourhood
            cases["two_rows_axis%d_dist%d" % (a, d)] = _rows([[1, 1, 1], np.add([1, 1, 1], _axis(a, d))])
        cases["block_edge_3_4_axis%d" % a] = _rows([_axis(a, 3), _axis(a, 4)])
        cases["block_edge_m1_0_axis%d" % a] = _rows([_axis(a, -1), _axis(a, 0)])
    neg = np.unique(rng.integers(-40, -8, (600, 3)), axis=0)
    cases["all_negative"] = _rows(neg[rng.permutation(neg.shape[0])])
    same = np.unique(rng.integers(0, 6, (40, 3)), axis=0)
    cases["two_batches_same_xyz"] = np.concatenate([_rows(same, 0), _rows(same, 1)], 0)
    for n in (63, 64, 65, 257):
        cases["line_%d" % n] = _rows([[i - 9, 2, -1] for i in range(n)])
    box = np.unique(rng.integers(0, 12, (1000, 3)), axis=0)
    cases["dense_box_12"] = _rows(box[rng.permutation(box.shape[0])])
    g = np.stack(np.meshgrid(np.arange(80), np.arange(80), indexing="ij"), -1).reshape(-1, 2)
    g = g[rng.permutation(g.shape[0])[:5000]]                          # an 80 x 80 plane with 1400 holes
    cases["plane_with_holes"] = _rows(np.stack([g[:, 0] - 17, g[:, 1] - 30, (g[:, 0] + g[:, 1]) // 16], 1))
    return cases


CASES = _cases()
_memo = {}


def _oracle(name, scale, ksize, rows=None):
    key = (name, scale, ksize)
    if key not in _memo:
        c = CASES[name].copy() if rows is None else rows
        if rows is None:
            c[:, 1:] *= scale
        nbr = oc.kernel_map(c, c, oc.kernel_offsets(ksize, scale))
        _memo[key] = (nbr, (nbr >= 0).sum(1).astype(np.int64))
    return _memo[key]


def _build(rows, scale, ksizes, legacy, occupancy=True):
    """Self maps of `ksizes` (one job each, in this order, one stream) over `rows` by ONE ops.maps_build call.
    -> [(nbr [K, n], counts [K])] as numpy, the arena's bytes outside the occupancy buffer"""
    from openscene_amd import ops
    x = torch.from_numpy(rows).to(dev())
    n = x.shape[0]
    table = ops.coords_unique(x, 1)[3]                                 # (the rows are unique: row numbers are the caller's)
    total, plan = 0, []

    def take(nbytes):
        nonlocal total
        off = total
        total += (int(nbytes) + 255) // 256 * 256
        return off
    for k in ksizes:
        plan.append((k, take(4 * k ** 3 * n), take(8 * k ** 3)))
    data_bytes = total
    occ_off = take(ops.maps_occupancy_bytes(n))
    arena = torch.full((total,), FILL, dtype=torch.uint8, device=dev())
    base = arena.data_ptr()
    jobs = [dict(lvl_in=0, lvl_out=0, ksize=k, scale=scale, self_map=1, stream=0, nbr_fwd=base + o_n, counts=base + o_c)
            for k, o_n, o_c in plan]
    prev = ops.maps_set_legacy(legacy)
    try:
        ops.maps_build([(x, table, n)], jobs, dev(), 0, streams=1, occ=[base + occ_off if occupancy else None])
        torch.cuda.synchronize()
    finally:
        ops.maps_set_legacy(prev)
    host = arena.cpu().numpy()
    out = []
    for k, o_n, o_c in plan:
        K = k ** 3
        out.append((host[o_n:o_n + 4 * K * n].view(np.int32).reshape(K, n), host[o_c:o_c + 8 * K].view(np.int64)))
    return out, host[:data_bytes]


def _check(name, scale, rows=None):
    c = CASES[name].copy() if rows is None else rows
    if rows is None:
        c[:, 1:] *= scale                                              # a level of tensor stride `scale`
    new, new_bytes = _build(c, scale, (5, 3), False)                   # 5^3 through the occupancy table, 3^3 copied out of it
    old, old_bytes = _build(c, scale, (5, 3), True)
    swapped, _ = _build(c, scale, (3, 5), False)                       # both probed, both through the occupancy table
    plain, plain_bytes = _build(c, scale, (5, 3), False, occupancy=False)   # 5^3 probed at every offset, 3^3 copied
    for ksize, got, leg, sw, pl in ((5, new[0], old[0], swapped[1], plain[0]), (3, new[1], old[1], swapped[0], plain[1])):
        want_nbr, want_counts = _oracle(name, scale, ksize, rows)
        for what, (nbr, counts) in (("occupancy / copied", got), ("legacy", leg), ("occupancy, probed", sw), ("no occupancy", pl)):
            assert np.array_equal(nbr, want_nbr), (name, scale, ksize, what)
            assert np.array_equal(counts, want_counts), (name, scale, ksize, what)
    assert np.array_equal(new_bytes, old_bytes) and np.array_equal(plain_bytes, old_bytes), (name, scale)


@pytest.mark.parametrize("scale", [1, 2, 4])
@pytest.mark.parametrize("name", sorted(CASES))
def test_self_maps_match_legacy_and_oracle(name, scale):
    _check(name, scale)


@pytest.mark.parametrize("scale", [2, 4])
def test_rows_that_are_no_multiple_of_the_scale(scale):
    """A dilated kernel over rows of stride 1: the block words cannot describe the cells -- the builder probes every offset."""
    rng = np.random.default_rng(11)
    box = np.unique(rng.integers(-9, 14, (1500, 3)), axis=0)
    rows = _rows(box[rng.permutation(box.shape[0])])
    assert (rows[:, 1:] % scale != 0).any()
    _check("dilated_%d" % scale, scale, rows=rows)


@pytest.mark.parametrize("name", ["one_row", "line_65", "dense_box_12", "all_negative"])
def test_ksize_7_keeps_the_legacy_kernel(name):
    c = CASES[name]
    want_nbr, want_counts = _oracle(name, 1, 7)
    (new,), nb = _build(c, 1, (7,), False)
    (old,), ob = _build(c, 1, (7,), True)
    for nbr, counts in (new, old):
        assert np.array_equal(nbr, want_nbr) and np.array_equal(counts, want_counts)
    assert np.array_equal(nb, ob)


class _PresetTorch:
    """torch, with empty() preset to one byte: what the map builder leaves unwritten then compares equal between two builds"""
    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kwargs):
        t = torch.empty(*args, **kwargs)
        if t.dtype == torch.uint8:
            t.fill_(FILL)
            self.made.append(t)
        return t


def _prebuild(coords, legacy, monkeypatch):
    from openscene_amd import ops, sparse
    proxy = _PresetTorch()
    calls = []
    real = ops.maps_build

    def spy(levels, jobs, dev_, sort_rows, streams=None, occ=None):
        calls.append((jobs, [r for _, _, r in levels], occ))
        return real(levels, jobs, dev_, sort_rows, streams, occ=occ)
    with monkeypatch.context() as m:
        m.setattr(sparse, "torch", proxy)
        m.setattr(ops, "maps_build", spy)
        m.setattr(sparse.CoordinateManager, "OCC_MIN_PROBES", 0)       # every level through the occupancy table
        m.setattr(sparse.CoordinateManager, "SORT_MIN_ROWS", 1000)     # tile-ordered tables at this size too
        prev = ops.maps_set_legacy(legacy)
        try:
            cm = sparse.CoordinateManager(coords)
            cm.prebuild(pairs=True)
            torch.cuda.synchronize()
        finally:
            ops.maps_set_legacy(prev)
    assert len(calls) == 1
    arena = max(proxy.made, key=lambda t: t.numel())
    jobs, rows, occ = calls[0]
    host = arena.cpu().numpy().copy()
    base = arena.data_ptr()
    n_occ = 0
    for r, o in zip(rows, occ):                                        # the occupancy buffers are the new path's scratch
        if o:
            host[o - base:o - base + ops.maps_occupancy_bytes(r)] = 0
            n_occ += 1
    return cm, jobs, host, base, n_occ


def test_minkunet_job_list_every_buffer_equal(monkeypatch):
    """One osn_maps_build call with MinkUNet's job list (5^3 stem map, 3^3 map per level, 2^3 stride-2 maps with transposes,
    tile orders, tile lists, pair lists) on a 3 000-voxel scene, several streams: the whole arena -- neighbour tables, counts,
    transposed and tile-ordered tables, orders, group masks, tile lists, pair lists -- byte for byte between the two settings."""
    vox = syn.shuffled(syn.grid_voxels(syn.room_points(3, n_pts=4000), 0.05), 3)[:3000]
    coords = torch.from_numpy(syn.batch_coords([vox])).to(dev())
    assert coords.shape[0] == 3000
    cm_new, jobs_new, new, base_new, n_occ = _prebuild(coords, False, monkeypatch)
    cm_old, jobs_old, old, base_old, _ = _prebuild(coords, True, monkeypatch)
    assert n_occ == 5
    assert len(jobs_new) == len(jobs_old) == 10 and new.shape == old.shape
    ptrs = ("nbr_fwd", "nbr_bwd", "counts", "order_fwd", "sorted_fwd", "gmask_fwd", "order_bwd", "sorted_bwd", "gmask_bwd",
            "tl_fwd", "tl_bwd", "pl_fwd")
    for a, b in zip(jobs_new, jobs_old):                               # the same layout: the arenas compare as a whole
        assert all((a.get(f, 0) or 0) - base_new == (b.get(f, 0) or 0) - base_old for f in ptrs if a.get(f) or b.get(f))
    assert sum(1 for q in jobs_new if q.get("pl_fwd")) == 9 and sum(1 for q in jobs_new if q.get("sorted_fwd")) >= 1
    diff = np.nonzero(new != old)[0]
    assert diff.size == 0, "first differing byte at arena offset %d of %d" % (diff[0], new.size)
    ref = oc.CoordinateManager(coords.cpu().numpy())
    for key in [(1, 1, 5)] + [(s, s, 3) for s in (1, 2, 4, 8, 16)]:
        assert np.array_equal(cm_new.kmap(*key)[0].cpu().numpy(), ref.kmap(*key)), key
        assert np.array_equal(cm_new.kmap_counts(*key).cpu().numpy(), (ref.kmap(*key) >= 0).sum(1)), key
