"""csrc/search.hip on the device: the bank append (bit for bit), the heat-map against the float64 evaluation of the
reference's expressions (abs <= 2e-3), and the selection -- exact against a torch selection computed from
the kernel's own heat-map (tests/search_reference.py: stable sort by descending score, then index, NaN last).

Heat-map tolerance: with unit-norm queries, dividing the fp32 accumulator by the norm instead of rounding the normalised
vector to fp16 first moves a score by at most 2^-11 = 4.9e-4 (Cauchy-Schwarz on the per-element rounding); one fp16
rounding of a value below 1 adds 2.4e-4 (below 2: 4.9e-4, the raw mode's rows keep |score| < 2).  Under 1e-3 either way;
2e-3 is asserted and the largest deviation printed.  That 2e-3 is the distance to the REFERENCE's expression, which rounds the
normalised vector to fp16 before the product, on unit_rows against unit queries; it is 5 % of a typical score at d = 768 and says
little about the kernel's own arithmetic, which is held element by element in tests/test_gpu_search_bounds.py (the fp16 rounding
of the float64 interval of tests/search_bounds.py, on rows of every magnitude)."""
import pytest
import torch

import search_reference as sr
from search_reference import check_selection, text, unit_rows

pytestmark = pytest.mark.gpu

TOL = 2e-3


def dev():
    return torch.device("cuda", 0)


def make_bank(scenes, d, capacity_rows=1 << 10):
    from openscene_amd.search import FeatureBank
    bank = FeatureBank(d, dev(), capacity_rows=capacity_rows)
    for i, f in enumerate(scenes):
        bank.add_scene("scene%04d" % i, f)
    return bank


# ----------------------------------------------------------------------------------------------------------- append
@pytest.mark.parametrize("d", [512, 768])
def test_append_equals_gather_then_half_bit_for_bit(d):
    from openscene_amd.search import FeatureBank
    g = torch.Generator().manual_seed(d)
    x = (torch.randn(1337, d, generator=g) * 3).to(dev())
    x[5, :4] = torch.tensor([1e-6, -7e4, 65520.0, float("nan")], device=dev())      # subnormal, overflow, the rounding edge, NaN
    inv = torch.randint(0, 1337, (2501,), generator=g).to(dev())
    bank = FeatureBank(d, dev(), capacity_rows=1000)
    bank.add_scene("plain", x)
    bank.add_scene("gathered", x, inv)
    assert bank.offsets == [0, 1337, 3838]
    assert sr.same_bits(bank.scene("plain"), x.half())
    assert sr.same_bits(bank.scene("gathered"), x[inv].half())
    before = bank.features.clone()
    for bad in (-1, 1337):
        inv_bad = inv.clone()
        inv_bad[1234] = bad
        with pytest.raises(Exception, match="gather index"):
            bank.add_scene("bad", x, inv_bad)
        assert bank.offsets == [0, 1337, 3838] and bank.names == ["plain", "gathered"]
        assert sr.same_bits(bank.features, before)
    bank.add_scene("after", x, inv[:100])                    # the error word was cleared
    assert sr.same_bits(bank.scene("after"), x[inv[:100]].half())


# --------------------------------------------------------------------------------------------------------- heat-map
@pytest.mark.parametrize("d", [512, 768])
@pytest.mark.parametrize("q", [1, 20, 32, 33, 70])
@pytest.mark.parametrize("normalize", [True, False])
def test_heat_map_matches_the_float64_reference_expressions(normalize, q, d):
    from openscene_amd.search import search
    g = torch.Generator().manual_seed(1000 * q + d + int(normalize))
    n = 1337                                                  # not a multiple of the 128-row tile
    x = unit_rows(n, d, g).half()
    zero_rows = torch.tensor([0, 77, 128, 1336])
    x[zero_rows] = 0
    x[300] = float("nan")
    x[301, 17] = float("nan")
    t = text(q, d, g)
    bank = make_bank([x], d)
    heat = search(bank, t.to(dev()), k=4, normalize=normalize, return_heat=True).heat.cpu()
    assert heat.shape == (n, q) and heat.dtype == torch.float16
    assert torch.isnan(heat[300]).all() and torch.isnan(heat[301]).all()
    assert (heat[zero_rows] == 0).all()                      # exactly zero: 0 / (0 + 1e-5)
    ok = torch.ones(n, dtype=torch.bool)
    ok[300] = ok[301] = False
    worst = 0.0
    for rounded in (False, True):
        ref = sr.scores_f64(x, t, normalize, round_normalised=rounded)
        dev_ = (heat.double() - ref)[ok].abs().max().item()
        print("heat-map normalize=%d q=%d d=%d vs float64%s: max abs deviation %.3e"
              % (normalize, q, d, " (normalised vector rounded to fp16)" if rounded else "", dev_))
        worst = max(worst, dev_)
    assert not torch.isnan(heat[ok]).any()
    assert worst <= TOL


# -------------------------------------------------------------------------------------------------------- selection
def selection_scenes(d, gen):
    """Four scenes: duplicates straddling the k-th place, an empty scene, thousands of zero rows where the k-th score is 0
    (queries 0 and 1: ten rows score above 0, the rest of the non-zero rows below), a scene shorter than any k > 50."""
    t = text(5, d, gen)
    a = unit_rows(300, d, gen)
    dup = 0.9 * t[0].float() + 0.05 * torch.nn.functional.normalize(torch.randn(d, generator=gen), dim=0)
    a[100:141] = dup                                          # 41 equal rows, the best of the scene for query 0
    a[7] = dup
    a[250] = float("nan")
    b = unit_rows(5000, d, gen)
    u = t[0].float() + t[1].float()
    e0 = torch.nn.functional.normalize(t[0].float(), dim=0)
    e1 = torch.nn.functional.normalize(t[1].float() - t[1].float().dot(e0) * e0, dim=0)
    for e in (e0, e1):
        b = b - (b @ e[:, None]) * e[None, :]                 # orthogonal to queries 0 and 1 ...
    sign = -torch.ones(5000, 1)
    pos = torch.tensor([11, 500, 999, 1500, 2222, 3000, 3333, 4000, 4500, 4999])
    sign[pos] = 1
    b = b + sign * (0.3 * u[None, :])                         # ... then pushed to one side of both
    zero = torch.randperm(5000, generator=gen)[:3000]
    zero = zero[~torch.isin(zero, pos)]
    b[zero] = 0
    c = unit_rows(50, d, gen)
    return [a.half(), torch.zeros(0, d, dtype=torch.float16), b.half(), c.half()], t


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("k", [1, 16, 128])
def test_selection_is_exact_against_the_kernels_own_heat_map(k, normalize):
    from openscene_amd.search import search
    d = 512
    g = torch.Generator().manual_seed(7)
    scenes, t = selection_scenes(d, g)
    bank = make_bank(scenes, d)
    t = t.to(dev())
    res = search(bank, t, k=k, normalize=normalize, return_heat=True)
    heat = res.heat
    # thresholds at values that occur in the data: a duplicated score, exact zero, and three sampled scores
    thr = torch.tensor([heat[100, 0].item(), 0.0, heat[400, 2].item(), heat[4000, 3].item(), heat[20, 4].item()])
    res = search(bank, t, k=k, thresholds=thr, normalize=normalize, return_heat=True)
    assert sr.same_bits(res.heat, heat)
    check_selection(res, heat, bank.offsets, k, thr.to(dev()))
    # the hard cases really are in the data
    if k >= 16:
        assert res.topk_points[0, 0, :16].tolist() == [7] + list(range(100, 115))       # ties: the lowest indices
        assert (res.topk_scores[2, 0, 10:k].float() == 0).all() and (res.topk_scores[2, 0, :10].float() > 0).all()
        pts = res.topk_points[2, 0, 10:k]
        assert (pts[1:] > pts[:-1]).all()
    if k == 128:
        assert (res.topk_points[3, :, 50:] == -1).all() and torch.isinf(res.topk_scores[3, :, 50:].float()).all()
        assert (res.topk_points[3, :, :50] >= 0).all()
        assert res.topk_points[0, 1, 127].item() >= 0 and not torch.isnan(res.topk_scores[0].float()).any()   # 299 numbers before the NaN row
    assert (res.topk_points[1] == -1).all() and res.counts[1].tolist() == [0] * 5
    assert res.counts[2, 1].item() >= 2500                   # >= 0: the zero rows count
    # without the heat-map: the same selection
    res2 = search(bank, t, k=k, thresholds=thr, normalize=normalize)
    assert res2.heat is None
    assert torch.equal(res2.topk_points, res.topk_points) and sr.same_bits(res2.topk_scores, res.topk_scores)
    assert torch.equal(res2.counts, res.counts)


def test_nan_orders_below_every_number_and_ties_by_index():
    """A scene of 40 rows, 30 of them NaN, k = 16: the ten numbers first, then NaN rows by index."""
    from openscene_amd.search import search
    d = 512
    g = torch.Generator().manual_seed(9)
    x = unit_rows(40, d, g).half()
    keep = torch.tensor([3, 4, 9, 10, 11, 20, 25, 31, 38, 39])
    nan = torch.ones(40, dtype=torch.bool)
    nan[keep] = False
    x[nan] = float("nan")
    t = text(3, d, g)
    bank = make_bank([x], d)
    res = search(bank, t.to(dev()), k=16, return_heat=True)
    check_selection(res, res.heat, bank.offsets, 16)
    assert sorted(res.topk_points[0, 0, :10].tolist()) == keep.tolist()
    assert res.topk_points[0, 0, 10:].tolist() == [0, 1, 2, 5, 6, 7]
    assert torch.isnan(res.topk_scores[0, :, 10:].float()).all()


@pytest.mark.parametrize("q", [33, 256])
def test_selection_over_many_queries_and_chunks(q):
    """More than one column tile, scenes longer than one 4096-row select chunk and not aligned to 8 rows."""
    from openscene_amd.search import search
    d = 512
    g = torch.Generator().manual_seed(q)
    scenes = [unit_rows(n, d, g).half() for n in (4099, 13, 9001)]
    scenes[2][::3] = 0                                        # 3001 zero rows spread over three chunks
    bank = make_bank(scenes, d)
    t = text(q, d, g).to(dev())
    thr = torch.zeros(q)
    res = search(bank, t, k=16, thresholds=thr, return_heat=True)
    check_selection(res, res.heat, bank.offsets, 16, thr.to(dev()))
    ref = sr.scores_f64(bank.features.cpu(), t.cpu(), True)
    assert (res.heat.cpu().double() - ref).abs().max().item() <= TOL


# ---------------------------------------------------------------------------------------------------- repeatability
def test_two_calls_are_bitwise_equal_and_scenes_do_not_see_each_other():
    from openscene_amd.search import search
    d = 768
    g = torch.Generator().manual_seed(11)
    scenes = [unit_rows(n, d, g).half() for n in (700, 129, 4500, 1, 2048, 333, 5000, 64)]
    for s in scenes:
        s[::5] = 0
    t = text(20, d, g).to(dev())
    thr = torch.full((20,), 0.02)
    bank = make_bank(scenes, d)
    r1 = search(bank, t, k=16, thresholds=thr, return_heat=True)
    r2 = search(bank, t, k=16, thresholds=thr, return_heat=True)
    for a, b in ((r1.heat, r2.heat), (r1.topk_scores, r2.topk_scores)):
        assert sr.same_bits(a, b)
    assert torch.equal(r1.topk_points, r2.topk_points) and torch.equal(r1.counts, r2.counts)
    for i, s in enumerate(scenes):
        one = search(make_bank([s], d), t, k=16, thresholds=thr, return_heat=True)
        assert sr.same_bits(one.heat, r1.scene_heat(i))
        assert sr.same_bits(one.topk_scores[0], r1.topk_scores[i]) and torch.equal(one.topk_points[0], r1.topk_points[i])
        assert torch.equal(one.counts[0], r1.counts[i])


# ---------------------------------------------------------------------------------------------------------- at size
def test_eight_scenes_of_150k_points_at_768():
    from openscene_amd.search import FeatureBank, search
    d, n, s_n, q, k = 768, 150_000, 8, 32, 16
    g = torch.Generator(device=dev()).manual_seed(5)
    bank = FeatureBank(d, dev(), capacity_rows=s_n * n)
    for i in range(s_n):
        x = torch.nn.functional.normalize(torch.randn(n, d, generator=g, device=dev()), dim=1)
        x = x * (0.5 + 1.5 * torch.rand(n, 1, generator=g, device=dev()))
        x[torch.rand(n, generator=g, device=dev()) < 0.1] = 0          # points without a feature
        bank.add_scene("scene%d" % i, x.half())
        del x
    t = torch.nn.functional.normalize(torch.randn(q, d, generator=g, device=dev()), dim=1).half()
    thr = torch.full((q,), 0.05)
    res = search(bank, t, k=k, thresholds=thr, return_heat=True)
    check_selection(res, res.heat, bank.offsets, k, thr.to(dev()))
    rows = torch.randint(0, s_n * n, (4096,), generator=torch.Generator().manual_seed(6)).to(dev())
    ref = sr.scores_f64(bank.features[rows], t, True)
    worst = (res.heat[rows].double() - ref).abs().max().item()
    print("at size: max abs deviation of 4096 sampled rows %.3e" % worst)
    assert worst <= TOL
    res2 = search(bank, t, k=k, thresholds=thr)
    assert torch.equal(res2.topk_points, res.topk_points) and sr.same_bits(res2.topk_scores, res.topk_scores)


# ------------------------------------------------------------------------------------------------------- end to end
def test_disnet_forward_to_bank_to_search():
    """run/evaluate.py:288-290 (`predictions = feat_3d[inds_reverse]`) -> add_scene -> search, every point checked."""
    from openscene_amd.disnet import DisNet
    from openscene_amd.search import FeatureBank, heat_map, search
    from openscene_amd.sparse import SparseTensor
    from openscene_amd import synthetic as syn

    class Cfg:
        arch_3d = "MinkUNet14A"
        feature_2d_extractor = "openseg"
    torch.manual_seed(3)
    net = DisNet(Cfg()).to(dev()).eval()
    coords = syn.batch_coords([syn.shuffled(syn.grid_voxels(syn.room_points(5, n_pts=9000), 0.05), 5)])
    c = torch.from_numpy(coords).to(dev())
    feats = torch.rand(coords.shape[0], 3, device=dev())
    g = torch.Generator().manual_seed(1)
    inds_reverse = torch.randint(0, coords.shape[0], (12001,), generator=g).to(dev())
    t = text(20, 768, g).to(dev())
    with torch.no_grad():
        pred = net(SparseTensor(feats, c))
    bank = FeatureBank(768, dev(), capacity_rows=1000)
    bank.add_scene("room", pred, inds_reverse)
    rows = pred[inds_reverse].half()
    assert sr.same_bits(bank.features, rows)
    thr = torch.full((20,), 0.1)
    res = search(bank, t, k=16, thresholds=thr, return_heat=True)
    ref = sr.scores_f64(rows.cpu(), t.cpu(), True)
    worst = (res.heat.cpu().double() - ref).abs().max().item()
    print("end to end: max abs deviation over all %d points %.3e" % (rows.shape[0], worst))
    assert worst <= TOL
    check_selection(res, res.heat, bank.offsets, 16, thr.to(dev()))
    assert sr.same_bits(heat_map(pred, t, inds_reverse), res.heat)
    assert res.rank_scenes(0)[0][0] == "room"
