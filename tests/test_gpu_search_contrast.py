"""Search with negative queries on the device (csrc/search.hip: osn_bank_search_contrast, osn_bank_search_contrast_fp8).

Relevancy values: against tests/search_contrast_reference.expected -- the plain search of cat([queries, negatives]) on the same
bank, split into s and g, the formula of include/openscene_amd.h in float64, rounded to fp16 once.  Every element within
1 fp16 ulp, compared as bit patterns: the kernel's fp32 evaluation errs by a few 2^-24 |z| relative, far below half an fp16
ulp, so it can only flip a rounding next to a tie; and at most 1 % of the elements differ at all (a float32 torch evaluation
of the same formula differs from float64 in 0 - 0.06 % of the elements on these inputs).
Selection: exact against tests/search_reference.select applied to the kernel's own relevancy map."""
import functools

import pytest
import torch

import search_contrast_reference as cr
import search_reference as sr
from search_reference import check_selection, text, unit_rows

pytestmark = pytest.mark.gpu

K = 16
SCENES = (0, 7, 993)          # an empty scene, one shorter than k, 1000 rows in all: the last workgroup is partial
WIDTHS = (64, 272)            # one partial 128-wide chunk; two full chunks and a tail (a multiple of 16 for the fp8 bank)
SETS = ((5, 4), (130, 33))    # (queries, negatives): the second crosses a column-group boundary with both, 32 or 64 wide
KINDS = ("fp16", "fp8")


def dev():
    return torch.device("cuda", 0)


def make_bank(kind, d, scenes):
    from openscene_amd.search import FeatureBank
    bank = FeatureBank(d, dev(), capacity_rows=64, dtype=kind)
    for i, f in enumerate(scenes):
        bank.add_scene("scene%04d" % i, f.to(dev()))
    return bank


@functools.lru_cache(maxsize=None)
def inputs(d):
    """(rows [1000, d] float32, queries fp16 [130, d], negatives fp16 [33, d]) of seed 7; the smaller sets are their heads."""
    g = torch.Generator().manual_seed(7)
    return unit_rows(sum(SCENES), d, g), text(SETS[1][0], d, g), text(SETS[1][1], d, g)


@functools.lru_cache(maxsize=None)
def the_bank(kind, d):
    x = inputs(d)[0]
    return make_bank(kind, d, torch.split(x, SCENES))


def same_result(a, b):
    return (sr.same_bits(a.heat, b.heat) and sr.same_bits(a.topk_scores, b.topk_scores) and torch.equal(a.topk_points, b.topk_points)
            and (a.counts is None) == (b.counts is None) and (a.counts is None or torch.equal(a.counts, b.counts)))


# ---------------------------------------------------------------------------------------- 1, 2: values and selection
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_relevancy_is_within_one_ulp_of_the_float64_formula_and_the_selection_is_exact(kind, normalize):
    from openscene_amd.search import search
    zeros = ones = 0
    for d in WIDTHS:
        bank = the_bank(kind, d)
        _, t_all, n_all = inputs(d)
        for q, m in SETS:
            t, neg = t_all[:q].to(dev()), n_all[:m].to(dev())
            for tau in (0.1, 0.01):
                res = search(bank, t, k=K, thresholds=0.5, normalize=normalize, return_heat=True, negatives=neg, temperature=tau)
                assert res.relevancy and res.temperature == tau
                assert res.heat.shape == (sum(SCENES), q) and res.heat.dtype == torch.float16
                want = cr.expected(search, bank, t, neg, tau, normalize)
                dist = cr.ulp_distance(res.heat, want)
                differ = (dist != 0).double().mean().item()
                share = (res.heat.float() >= 0.5).double().mean().item()
                print("%s normalize=%d d=%d q=%d m=%d tau=%g: max ulp %d, %.4f %% differ, %.1f %% >= 0.5"
                      % (kind, normalize, d, q, m, tau, dist.max().item(), 100 * differ, 100 * share))
                assert dist.min().item() >= 0 and dist.max().item() <= 1
                assert differ <= 0.01
                assert 0.01 < share < 0.9                       # the threshold selects a set that is neither empty nor everything
                check_selection(res, res.heat, bank.offsets, K, torch.full((q,), 0.5, device=dev()))
                if tau == 0.01:
                    zeros += int((res.heat == 0).sum())
                    ones += int((res.heat == 1).sum())
    assert zeros > 100 and ones > 100                           # saturation: large tie groups at both ends


# ---------------------------------------------------------------------------- 3: one arithmetic for both column kinds
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_a_query_that_is_its_own_negative_scores_exactly_one_half(kind, normalize):
    from openscene_amd.search import search
    d = 272
    x, t_all, _ = inputs(d)
    x = x[:300].clone()
    x[17] = 0                                                 # normalize = 0: 0 - 0
    bank = make_bank(kind, d, [x])
    t = t_all[:1].to(dev())
    res = search(bank, t, k=K, normalize=normalize, return_heat=True, negatives=t)
    assert (res.heat.view(torch.int16) == 0x3800).all()
    t = t_all.to(dev())                                       # q = m = 130: a column meets itself in another group's place
    res = search(bank, t, k=K, normalize=normalize, return_heat=True, negatives=t)
    assert (res.heat.float().max(dim=1)[0] == 0.5).all()


# ---------------------------------------------------------------------------------------------------------- 4: NaN
@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_row_is_nan_for_every_query_orders_last_and_counts_for_nothing(kind):
    from openscene_amd.search import search
    d = 64
    x, t_all, n_all = inputs(d)
    t, neg = t_all[:5].to(dev()), n_all[:4].to(dev())
    bad = x.clone()
    row = 3                                                   # inside the 7-row scene: every one of its rows is selected
    bad[row, 11] = float("nan")
    clean, dirty = the_bank(kind, d), make_bank(kind, d, torch.split(bad, SCENES))
    thr = torch.zeros(5)                                      # every number counts
    for normalize in (True, False):
        ref = search(clean, t, k=K, thresholds=thr, normalize=normalize, return_heat=True, negatives=neg)
        res = search(dirty, t, k=K, thresholds=thr, normalize=normalize, return_heat=True, negatives=neg)
        assert torch.isnan(res.heat[row]).all()
        keep = torch.arange(sum(SCENES)) != row
        assert sr.same_bits(res.heat[keep], ref.heat[keep])
        assert (res.topk_points[1, :, 6] == row).all() and torch.isnan(res.topk_scores[1, :, 6]).all()
        assert not torch.isnan(res.topk_scores[1, :, :6]).any() and (res.topk_points[1, :, 7:] == -1).all()
        assert res.counts[1].tolist() == [6] * 5 and ref.counts[1].tolist() == [7] * 5
        assert torch.equal(res.counts[2], ref.counts[2])
        check_selection(res, res.heat, dirty.offsets, K, thr.to(dev()))


# ------------------------------------------------------------------------------------------- 5, 7: repeats, plain path
@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_agree_bit_for_bit_and_the_plain_search_is_what_it_was(kind):
    from openscene_amd.search import search
    d = 272
    bank = the_bank(kind, d)
    _, t_all, n_all = inputs(d)
    t, neg = t_all.to(dev()), n_all.to(dev())
    a = search(bank, t, k=K, thresholds=0.5, return_heat=True, negatives=neg, temperature=0.01)
    b = search(bank, t, k=K, thresholds=0.5, return_heat=True, negatives=neg, temperature=0.01)
    assert same_result(a, b)
    no_heat = search(bank, t, k=K, thresholds=0.5, negatives=neg, temperature=0.01)
    assert no_heat.heat is None and torch.equal(no_heat.topk_points, a.topk_points) and torch.equal(no_heat.counts, a.counts)
    plain = search(bank, t, k=K, thresholds=0.1, return_heat=True)
    same = search(bank, t, k=K, thresholds=0.1, return_heat=True, negatives=None)
    assert same_result(plain, same) and not plain.relevancy and plain.temperature is None
    assert same_result(plain, search(bank, t, k=K, thresholds=0.1, return_heat=True))        # (after the contrast calls, too)


def test_heat_map_with_negatives_is_the_search_of_a_one_scene_bank():
    from openscene_amd.search import heat_map, search
    d = 64
    x, t_all, n_all = inputs(d)
    t, neg = t_all[:5].to(dev()), n_all[:4].to(dev())
    inv = torch.tensor([4, 0, 0, 199, 2])
    hm = heat_map(x[:200].to(dev()), t, inv.to(dev()), negatives=neg, temperature=0.05)
    res = search(make_bank("fp16", d, [x[:200][inv]]), t, k=1, return_heat=True, negatives=neg, temperature=0.05)
    assert hm.shape == (5, 5) and sr.same_bits(hm, res.heat) and sr.same_bits(hm[1], hm[2])


# --------------------------------------------------------------------------------------------------- 6: downstream
@pytest.mark.parametrize("kind", KINDS)
def test_objects_and_scene_ranks_of_a_relevancy_search(kind):
    """the planted cluster of tests/test_gpu_search_fp8.py::test_objects_of_an_fp8_search"""
    from openscene_amd.objects import VoxelGrid, find_objects
    from openscene_amd.search import search
    d = 48
    g = torch.Generator().manual_seed(41)
    t = text(2, d, g)
    neg = text(4, d, g)
    n = 400
    xyz = torch.rand(n, 3, generator=g)
    x = unit_rows(n, d, g)
    blob = (xyz - torch.tensor([0.3, 0.3, 0.3])).norm(dim=1) < 0.2
    x[blob] = t[0].float() + 0.02 * torch.randn(int(blob.sum()), d, generator=g)
    bank = make_bank(kind, d, [x[:250], x[250:]])
    grid = VoxelGrid(xyz.to(dev()), bank.offsets, voxel_size=0.1)
    res = search(bank, t.to(dev()), k=8, thresholds=0.5, return_heat=True, negatives=neg.to(dev()))
    got = res.find_objects(grid, 0.5, return_point_ids=True)
    ref = find_objects(grid, res.heat, 0.5, return_point_ids=True)
    assert got.names == bank.names and got.n_objects[:, 0].sum().item() >= 1
    assert torch.equal(got.n_objects, ref.n_objects) and torch.equal(got.point_object, ref.point_object)
    for f in ("n_points", "n_voxels", "peak_point", "score_sum", "vox_sum", "box_min", "box_max"):
        assert torch.equal(getattr(got, f), getattr(ref, f)), f
    assert sr.same_bits(got.peak_score, ref.peak_score)
    in_blob = (res.heat[:, 0].float().cpu() >= 0.5)[blob]
    assert in_blob.all()                                      # the cluster looks more like the query than like any negative
    for j in range(2):
        counts = res.counts[:, j].tolist()
        ranked = res.rank_scenes(j, by="count")
        assert dict(ranked) == dict(zip(bank.names, counts))
        assert [c for _, c in ranked] == sorted(counts, reverse=True)
        whole = [int((res.scene_heat(i)[:, j].float() >= 0.5).sum()) for i in range(2)]
        assert counts == whole
    pooled = got.descriptors(bank)                            # (runs: the objects of a relevancy search pool as any others)
    assert pooled is not None
