"""Descriptors on the device (csrc/pool.hip: osn_bank_pool, osn_bank_pool_fp8 through openscene_amd.descriptors).

Sums: every element within  POOL_C * abs-sum + 6e-8 |want| + 1e-37  of the float64 evaluation on the stored values
(tests/pool_reference.py: pool_f64; POOL_C is four times the worst error / abs-sum of an independent float32 evaluation in
chunks of BANK_POOL_CHUNK over these very inputs, measured in tests/test_pool_cpu.py).  count exact, wsum within
POOL_C * sum |w|.  Without any tolerance: a group of one row, a group of 2^k copies of a row, repeated calls, permuted groups,
the groups next to a NaN row.  The guards: a row outside the bank, a bad weight.  End to end: find, describe, search again."""
import functools

import pytest
import torch

import pool_reference as pr
import search_reference as sr

pytestmark = pytest.mark.gpu

C = pr.CHUNK


def dev():
    return torch.device("cuda", 0)


def make_bank(kind, scenes):
    from openscene_amd.search import FeatureBank
    bank = FeatureBank(scenes[0].shape[1], dev(), capacity_rows=8, dtype=kind)
    for i, f in enumerate(scenes):
        bank.add_scene("scene%d" % i, f.to(dev()))
    return bank


def stored(bank):
    return (bank.features.float() if bank.dtype == "fp16" else bank.dequantize()).cpu()


def groups_of(starts, rows, n_entries=None, shape=None):
    from openscene_amd.descriptors import PointGroups
    return PointGroups(starts.to(dev()), None if rows is None else rows.to(dev()), shape=shape, n_entries=n_entries)


def pool(bank, starts, rows, weights=None, normalize=True):
    from openscene_amd.descriptors import pool as f
    g = groups_of(starts, rows, n_entries=int(starts[-1]))
    return f(bank, g, weights=None if weights is None else weights.to(dev()), normalize=normalize)


@functools.lru_cache(maxsize=None)
def on_the_device(name):
    """One bound case: its bank, the float64 reference on the bank's stored values (computed once), the kernel's result."""
    case = pr.bound_case(name)
    bank = make_bank(case["kind"], case["scenes"])
    want = pr.pool_f64(stored(bank), case["starts"], case["rows"], case["weights"], case["normalize"])
    got = pool(bank, case["starts"], case["rows"], case["weights"], case["normalize"])
    return case, bank, want, got


def within(got, want, bound, label):
    ratio, n_bad = pr.worst_ratio(got, want, bound, pr.POOL_C)
    print("%s: worst err / limit %.3f" % (label, ratio))
    assert n_bad == 0, "%s: %d elements beyond the bound, worst ratio %.2f" % (label, n_bad, ratio)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ bound
@pytest.mark.parametrize("name", pr.case_names())
def test_sums_weights_and_counts_against_float64(name):
    from openscene_amd import ops
    assert ops.BANK_POOL_CHUNK == C and pr.POOL_C <= pr.POOL_C_CAP
    case, bank, (want, bound, wsum, count), got = on_the_device(name)
    g = case["starts"].shape[0] - 1
    assert got.sum.shape == (g, bank.dim) and got.sum.dtype == torch.float32 and got.count.dtype == torch.int64
    within(got.sum, want, bound, name)
    assert torch.equal(got.count.cpu(), count)
    w_err = (got.weight.double().cpu() - wsum).abs()
    assert bool((w_err <= pr.POOL_C * wsum).all()), float(w_err.max())            # (wsum = sum |w|: no weight is negative)
    empty = count == 0
    assert bool((got.sum.cpu()[empty] == 0).all()) and bool((got.mean.cpu()[empty] == 0).all())


def test_two_calls_give_the_same_bits():
    for name in ("fp16-768-weighted", "fp8-768-weighted", "fp16-24-many", "fp8-16-scenes"):
        case, bank, _, got = on_the_device(name)
        again = pool(bank, case["starts"], case["rows"], case["weights"], case["normalize"])
        assert same_bits(got.sum, again.sum) and same_bits(got.weight, again.weight), name


@pytest.mark.parametrize("name", ["fp16-520-weighted", "fp8-528-weighted", "fp16-24-many"])
def test_permuting_the_groups_permutes_the_results_bit_for_bit(name):
    case, bank, _, got = on_the_device(name)
    starts, rows, w = case["starts"], case["rows"], case["weights"]
    g = starts.shape[0] - 1
    perm = torch.randperm(g, generator=torch.Generator().manual_seed(5))
    length = (starts[1:] - starts[:-1])[perm]
    entry = torch.cat([torch.arange(int(starts[p]), int(starts[p + 1])) for p in perm.tolist()])
    p_starts = torch.zeros(g + 1, dtype=torch.int64)
    p_starts[1:] = torch.cumsum(length, 0)
    moved = pool(bank, p_starts, rows[entry], w[entry], case["normalize"])
    assert same_bits(moved.sum.cpu(), got.sum.cpu()[perm]) and same_bits(moved.weight.cpu(), got.weight.cpu()[perm])
    assert torch.equal(moved.count.cpu(), got.count.cpu()[perm])


# ------------------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("kind,d", [("fp16", 8), ("fp16", 512), ("fp16", 520), ("fp16", 768), ("fp16", 1024), ("fp8", 16), ("fp8", 528), ("fp8", 1024)])
def test_one_row_comes_back_bit_for_bit_and_copies_of_a_row_have_it_as_their_mean(kind, d):
    gen = torch.Generator().manual_seed(d)
    bank = make_bank(kind, [sr.unit_rows(40, d, gen).half()])
    values = stored(bank)
    rows = torch.randperm(40, generator=gen)
    one = pool(bank, torch.arange(41), rows, normalize=False)                   # forty groups of one row each
    assert same_bits(one.sum.cpu(), values[rows]) and same_bits(one.mean.cpu(), values[rows])
    assert one.count.tolist() == [1] * 40 and one.weight.tolist() == [1.0] * 40
    lengths = [2 ** k for k in range(11)]                                       # 1 .. 1024 copies: up to two chunks
    which = torch.randint(0, 40, (11,), generator=gen)
    copies = pool(bank, pr._csr(lengths), torch.repeat_interleave(which, torch.tensor(lengths)), normalize=False)
    assert same_bits(copies.mean.cpu(), values[which]) and copies.count.tolist() == lengths


# ------------------------------------------------------------------------------------------------------------ guards
@pytest.mark.parametrize("kind", ["fp16", "fp8"])
def test_a_bad_row_or_weight_raises_clears_the_error_word_and_leaves_the_bank_searchable(kind):
    from openscene_amd.search import search
    gen = torch.Generator().manual_seed(9)
    d = 64
    feats = [sr.unit_rows(70, d, gen).half(), sr.unit_rows(30, d, gen).half()]
    bank = make_bank(kind, feats)
    text = sr.text(3, d, gen).to(dev())
    before = search(bank, text, k=4, return_heat=True)
    rows = torch.arange(0, 100, 3)
    starts = torch.tensor([0, 10, rows.shape[0]])
    good = pool(bank, starts, rows)
    ones = torch.ones(rows.shape[0])
    for at, bad_row, bad_w in ((5, bank.rows, None), (20, -1, None), (7, None, float("nan")), (33, None, -1.0)):
        r, w = rows.clone(), ones.clone()
        if bad_row is not None:
            r[at] = bad_row
        else:
            w[at] = bad_w
        with pytest.raises(RuntimeError, match="osn_bank_pool"):
            pool(bank, starts, r, w)
        assert int(bank._err_word().item()) == 0
    after = search(bank, text, k=4, return_heat=True)
    assert sr.same_bits(after.heat, before.heat) and torch.equal(after.topk_points, before.topk_points)
    sr.check_selection(after, after.heat, bank.offsets, 4)
    assert same_bits(pool(bank, starts, rows).sum, good.sum)


@pytest.mark.parametrize("kind", ["fp16", "fp8"])
def test_a_nan_row_makes_its_own_group_nan_and_no_other(kind):
    gen = torch.Generator().manual_seed(13)
    d = 48
    x = sr.unit_rows(60, d, gen).half()
    clean = make_bank(kind, [x])
    x[17, 5] = float("nan")
    dirty = make_bank(kind, [x])
    lengths = [3, 0, C + 2, 5, 1]
    starts = pr._csr(lengths)
    rows = torch.randint(0, 60, (sum(lengths),), generator=gen)
    rows[rows == 17] = 18
    rows[3 + C] = 17                                                            # in the second chunk of group 2
    a, b = pool(clean, starts, rows), pool(dirty, starts, rows)
    assert bool(torch.isnan(b.mean[2]).all())
    others = [0, 1, 3, 4]
    assert same_bits(a.sum[others], b.sum[others]) and not bool(torch.isnan(a.sum).any())


# ------------------------------------------------------------------------------------------------------------ fp8 and fp16
def test_an_fp16_bank_and_its_fp8_twin_each_stay_inside_the_bound_of_their_own_stored_values():
    case = pr.bound_case("fp8-528-weighted")
    bank = make_bank("fp16", case["scenes"])
    twin = bank.to_fp8()
    for b in (bank, twin):
        want, bound, _, count = pr.pool_f64(stored(b), case["starts"], case["rows"], case["weights"], True)
        got = pool(b, case["starts"], case["rows"], case["weights"], True)
        within(got.sum, want, bound, b.dtype)
        assert torch.equal(got.count.cpu(), count)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_find_an_object_describe_it_and_find_its_like_in_every_scene():
    from openscene_amd.descriptors import describe_scenes
    from openscene_amd.objects import VoxelGrid
    from openscene_amd.search import search
    p = pr.planted()
    ref = pr.planted_reference_route()
    bank = make_bank("fp16", p["feats"])
    grid = VoxelGrid.from_scenes([x.to(dev()) for x in p["xyz"]], voxel_size=pr.PLANT_VOXEL)
    res = search(bank, p["a"].half()[None].to(dev()), thresholds=pr.PLANT_THRESHOLD, return_heat=True)
    objs = res.find_objects(grid, pr.PLANT_THRESHOLD, max_objects=8, return_point_ids=True)
    desc = objs.descriptors(bank)
    assert desc.shape == (3, 1, 8) and torch.equal(desc.count.reshape(3, 1, 8), objs.n_points)
    starts, rows = pr.objects_csr(objs.point_object, objs.offsets, 1, 8)
    want, bound, _, _ = pr.pool_f64(stored(bank), starts, rows, None, True)
    within(desc.sum, want, bound, "object descriptors")
    best = bank.names.index(objs.rank_scenes(0, by="peak")[0][0])
    q2 = desc.queries()[best * 8:best * 8 + 1]
    res2 = search(bank, q2, thresholds=pr.PLANT_THRESHOLD, return_heat=True)
    objs2 = res2.find_objects(grid, pr.PLANT_THRESHOLD, max_objects=8)
    is_a = torch.cat(p["is_a"])
    for s in range(3):                                                          # every scene's best match is a planted class-A cluster
        assert bool(is_a[bank.offsets[s] + int(objs2.peak_point[s, 0, 0])])
    assert res2.rank_scenes(0, by="count") == list(zip(bank.names, ref["counts2"]))
    assert objs2.rank_scenes(0, by="objects") == list(zip(bank.names, ref["n_objects2"]))
    weighted = objs.descriptors(bank, heat=res.heat)
    w = res.heat[rows.to(dev()), 0].float().clamp(min=0).cpu()
    want, bound, _, _ = pr.pool_f64(stored(bank), starts, rows, w, True)
    within(weighted.sum, want, bound, "heat-weighted object descriptors")
    for b in (bank, bank.to_fp8()):                                             # scenes ranked by their planted share of class A
        scores = describe_scenes(b).queries().float().cpu() @ torch.stack([p["a"], p["b"]]).t()
        assert torch.sort(scores[:, 0], descending=True)[1].tolist() == [0, 1, 2]
        assert torch.sort(scores[:, 1], descending=True)[1].tolist() == [2, 1, 0]
