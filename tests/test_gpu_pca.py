"""Second moments and feature colours on the device (csrc/gram.hip: osn_bank_gram, osn_bank_gram_fp8 through
openscene_amd.pca).

Gram elements within  (R + GRAM_C) * abs-gram + 6e-8 |want| + 1e-37  of the float64 evaluation on the stored values with
unrounded normalised rows, the sums within the same with R_SUM and abs-sum (tests/gram_reference.py: gram_f64; R = 0 where the
operands are exact; GRAM_C is four times the worst error / abs-sum of an independent float32 evaluation in slices of
BANK_GRAM_SLICE over these very inputs, measured in tests/test_pca_cpu.py).  count exact.  Without any tolerance: rows of
small integers against the integer computation, a group of one row, symmetry, repeated calls, permuted groups, a group alone
and inside a list, the groups next to a NaN row.  The guard: a row outside the bank.  End to end: moments, principal
directions, projection, colours, a rendered picture -- on the planted scenes of the CPU test, under its conditions."""
import functools

import pytest
import torch

import gram_reference as gr
import search_reference as sr

pytestmark = pytest.mark.gpu

S = gr.SLICE


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


def moments(bank, starts, rows, normalize=True):
    from openscene_amd.descriptors import PointGroups
    from openscene_amd.pca import moments as f
    g = PointGroups(starts.to(dev()), None if rows is None else rows.to(dev()), n_entries=int(starts[-1]))
    return f(bank, g, normalize=normalize)


@functools.lru_cache(maxsize=None)
def on_the_device(name):
    """One bound case: its bank, the float64 reference on the bank's stored values (computed once), the kernel's result."""
    case = gr.bound_case(name)
    bank = make_bank(case["kind"], case["scenes"])
    values = stored(bank)
    want = gr.gram_f64(values, case["starts"], case["rows"], case["normalize"])
    got = moments(bank, case["starts"], case["rows"], case["normalize"])
    return case, bank, values, want, got


def within(got, want, bound, c, label):
    ratio, n_bad = gr.worst_ratio(got, want, bound, c)
    print("%s: worst err / limit %.3f" % (label, ratio))
    assert n_bad == 0, "%s: %d elements beyond the bound, worst ratio %.2f" % (label, n_bad, ratio)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def symmetric(gram):
    return same_bits(gram, gram.transpose(1, 2).contiguous())


# ------------------------------------------------------------------------------------------------------------ bound
@pytest.mark.parametrize("name", gr.case_names())
def test_gram_sums_and_counts_against_float64(name):
    from openscene_amd import ops
    assert ops.BANK_GRAM_SLICE == S and gr.GRAM_C <= gr.GRAM_C_CAP
    case, bank, values, (want, bound, total, tbound, count), got = on_the_device(name)
    g, d = case["starts"].shape[0] - 1, bank.dim
    assert got.gram.shape == (g, d, d) and got.gram.dtype == torch.float32
    assert got.sum.shape == (g, d) and got.sum.dtype == torch.float32 and got.count.dtype == torch.int64
    r_gram, r_sum = gr.case_r(case, values)
    within(got.gram, want, bound, r_gram + gr.GRAM_C, name + " gram")
    within(got.sum, total, tbound, r_sum + gr.GRAM_C, name + " sum")
    assert torch.equal(got.count.cpu(), count)
    assert symmetric(got.gram)
    empty = count == 0
    assert bool((got.gram.cpu()[empty] == 0).all()) and bool((got.sum.cpu()[empty] == 0).all())
    assert bool((got.mean.cpu()[empty] == 0).all())


@pytest.mark.parametrize("kind", ["fp16", "fp8"])
def test_components_below_fp16s_normal_range_meet_the_bound_with_its_absolute_terms(kind):
    """Unfloored rows over six decades: a normalised component below 2^-14 rounds to fp16 within 2^-25, not within 2^-11 of itself
    (tests/gram_reference.py: tiny_case, tiny_slack; tests/test_pca_cpu.py shows that the relative term alone cannot hold)."""
    case = gr.tiny_case(kind)
    bank = make_bank(kind, case["scenes"])
    want, bound, total, tbound, count = gr.gram_f64(stored(bank), case["starts"], case["rows"], True)
    got = moments(bank, case["starts"], case["rows"], True)
    g_slack, s_slack = gr.tiny_slack(tbound, count)
    ratio, n_bad = gr.beyond(got.gram, want, bound, gr.R_GRAM + gr.GRAM_C, g_slack)
    print("%s gram: worst err / limit %.3f" % (kind, ratio))
    assert n_bad == 0
    ratio, n_bad = gr.beyond(got.sum, total, tbound, gr.R_SUM + gr.GRAM_C, s_slack)
    print("%s sum: worst err / limit %.3f" % (kind, ratio))
    assert n_bad == 0 and torch.equal(got.count.cpu(), count) and symmetric(got.gram)


# ------------------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("kind,d", [("fp16", 24), ("fp16", 520), ("fp16", 768), ("fp8", 16), ("fp8", 528), ("fp8", 768)])
def test_small_integers_give_the_integer_gram_matrix_bit_for_bit(kind, d):
    """|v| <= 8: every product and every sum (at most 64 * (2 S + 3) < 2^24) is an integer that float32 holds, whatever the
    order -- any indexing, transposition, tile-edge or slice-edge error shows."""
    gen = torch.Generator().manual_seed(d)
    x = torch.randint(-8, 9, (700, d), generator=gen)
    bank = make_bank(kind, [x.half()])
    assert torch.equal(stored(bank).long(), x)                                  # (an e4m3 row with a power-of-two scale holds them)
    starts = gr._csr(gr.FULL)
    rows = torch.randint(0, 700, (int(starts[-1]),), generator=gen)
    got = moments(bank, starts, rows, normalize=False)
    for g, length in enumerate(gr.FULL):
        xg = x[rows[int(starts[g]):int(starts[g + 1])]].double()               # (float64 holds these integers exactly too)
        assert torch.equal(got.gram[g].cpu().long(), (xg.t() @ xg).long()), (g, length)
        assert torch.equal(got.sum[g].cpu().long(), xg.sum(0).long()), (g, length)
    assert got.count.tolist() == list(gr.FULL) and symmetric(got.gram)


@pytest.mark.parametrize("kind,d", [("fp16", 24), ("fp16", 520), ("fp16", 768), ("fp16", 1024), ("fp8", 16), ("fp8", 528), ("fp8", 1024)])
def test_a_group_of_one_row_gives_the_outer_product_of_its_operand_exactly(kind, d):
    gen = torch.Generator().manual_seed(d + 1)
    bank = make_bank(kind, [sr.unit_rows(40, d, gen).half()])
    values = stored(bank)
    rows = torch.randperm(40, generator=gen)
    raw = moments(bank, torch.arange(41), rows, normalize=False)               # forty groups of one row each
    v = values[rows]
    assert same_bits(raw.sum.cpu(), v) and same_bits(raw.mean.cpu(), v)
    assert same_bits(raw.gram.cpu(), v[:, :, None] * v[:, None, :])            # (two fp16 values: the float32 product is exact)
    assert raw.count.tolist() == [1] * 40
    unit = moments(bank, torch.arange(41), rows, normalize=True)
    h = unit.sum.cpu()                                                         # the operand itself: an fp16 value next to v / (|v| + 1e-5)
    assert torch.equal(h.half().float(), h)
    x = values[rows].double()
    x = x / (x.norm(dim=1, keepdim=True) + 1e-5)
    assert bool(((h.double() - x).abs() <= 2.0 ** -11 * x.abs() + 2.0 ** -25).all())
    assert same_bits(unit.gram.cpu(), h[:, :, None] * h[:, None, :])


def test_two_calls_give_the_same_bits():
    for name in ("fp16-768-plain", "fp8-768-scaled", "fp16-24-many", "fp8-16-scenes"):
        case, bank, _, _, got = on_the_device(name)
        again = moments(bank, case["starts"], case["rows"], case["normalize"])
        assert same_bits(got.gram, again.gram) and same_bits(got.sum, again.sum), name


@pytest.mark.parametrize("name", ["fp16-520-scaled", "fp8-528-plain", "fp16-24-many"])
def test_permuting_the_groups_permutes_the_results_bit_for_bit(name):
    case, bank, _, _, got = on_the_device(name)
    starts, rows = case["starts"], case["rows"]
    g = starts.shape[0] - 1
    perm = torch.randperm(g, generator=torch.Generator().manual_seed(5))
    length = (starts[1:] - starts[:-1])[perm]
    entry = torch.cat([torch.arange(int(starts[p]), int(starts[p + 1])) for p in perm.tolist()])
    p_starts = torch.zeros(g + 1, dtype=torch.int64)
    p_starts[1:] = torch.cumsum(length, 0)
    moved = moments(bank, p_starts, rows[entry], case["normalize"])
    assert same_bits(moved.gram.cpu(), got.gram.cpu()[perm]) and same_bits(moved.sum.cpu(), got.sum.cpu()[perm])
    assert torch.equal(moved.count.cpu(), got.count.cpu()[perm])


@pytest.mark.parametrize("name", ["fp16-24-plain", "fp8-528-scaled"])
def test_a_group_alone_has_the_bits_it_has_inside_a_list(name):
    case, bank, _, _, got = on_the_device(name)
    starts, rows = case["starts"].tolist(), case["rows"]
    for g in range(len(starts) - 1):
        alone = moments(bank, torch.tensor([0, starts[g + 1] - starts[g]]), rows[starts[g]:starts[g + 1]], case["normalize"])
        assert same_bits(alone.gram[0], got.gram[g]) and same_bits(alone.sum[0], got.sum[g]), g
        assert int(alone.count[0]) == int(got.count[g])


# ------------------------------------------------------------------------------------------------------------ guards
@pytest.mark.parametrize("kind", ["fp16", "fp8"])
def test_a_nan_row_makes_its_own_group_nan_and_no_other(kind):
    gen = torch.Generator().manual_seed(13)
    d = 48
    x = sr.unit_rows(60, d, gen).half()
    clean = make_bank(kind, [x])
    x[17, 5] = float("nan")
    x[29, 40] = float("inf")
    dirty = make_bank(kind, [x])
    lengths = [3, 0, S + 2, 5, 1, 4]
    starts = gr._csr(lengths)
    rows = torch.randint(0, 60, (sum(lengths),), generator=gen)
    rows[(rows == 17) | (rows == 29)] = 18
    rows[3 + S] = 17                                                            # in the second slice of group 2
    rows[-2] = 29                                                               # the inf row, in the last group
    a, b = moments(clean, starts, rows), moments(dirty, starts, rows)
    assert bool(torch.isnan(b.gram[2]).all()) and bool(torch.isnan(b.sum[2]).all())
    assert bool(torch.isnan(b.gram[5]).any()) and bool(torch.isnan(b.sum[5]).any())
    others = [0, 1, 3, 4]
    assert same_bits(a.gram[others], b.gram[others]) and same_bits(a.sum[others], b.sum[others])
    assert not bool(torch.isnan(a.gram).any())


@pytest.mark.parametrize("kind", ["fp16", "fp8"])
def test_a_row_outside_the_bank_raises_and_leaves_the_bank_usable(kind):
    from openscene_amd.search import search
    gen = torch.Generator().manual_seed(9)
    d = 64
    bank = make_bank(kind, [sr.unit_rows(70, d, gen).half(), sr.unit_rows(30, d, gen).half()])
    text = sr.text(3, d, gen).to(dev())
    before = search(bank, text, k=4, return_heat=True)
    rows = torch.arange(0, 100, 3)
    starts = torch.tensor([0, 10, rows.shape[0]])
    good = moments(bank, starts, rows)
    for at, bad_row in ((5, bank.rows), (20, -1)):
        r = rows.clone()
        r[at] = bad_row
        with pytest.raises(RuntimeError, match="osn_bank"):
            moments(bank, starts, r)
        assert int(bank._err_word().item()) == 0
    after = search(bank, text, k=4, return_heat=True)
    assert sr.same_bits(after.heat, before.heat) and torch.equal(after.topk_points, before.topk_points)
    again = moments(bank, starts, rows)
    assert same_bits(again.gram, good.gram) and same_bits(again.sum, good.sum)


# ------------------------------------------------------------------------------------------------------------ end to end
def project_within(coords, basis, values, group=0):
    """The library's coordinates against float64 ones on the same fp16-rounded components, under the CPU test's condition: one
    fp16 rounding of the score, 2^-11 max(|score|, 2^-14), plus the float32 roundings of the offset and of the difference."""
    x = values.double()
    x = x / (x.norm(dim=1, keepdim=True) + 1e-5)
    c = basis.components[group].half().double()
    score = x @ c.t()
    offset = c @ basis.mean[group].double()
    err = (coords.double().cpu() - (score - offset)).abs()
    lim = 2.0 ** -11 * score.abs().clamp(min=2.0 ** -14) + 2.0 ** -23 * (offset.abs() + score.abs())
    print("projection: worst err / limit %.3f" % float((err / lim).max()))
    return bool((err <= lim).all())


def test_moments_directions_projection_colours_and_a_picture_of_the_planted_scenes():
    from openscene_amd import render as R
    from openscene_amd.descriptors import PointGroups
    from openscene_amd.pca import feature_colors, moments as lib_moments, principal_directions
    p = gr.planted()
    cls = torch.cat(p["cls"])
    planes = {}
    for kind in ("fp16", "fp8"):
        bank = make_bank(kind, p["feats"])
        per_scene = principal_directions(lib_moments(bank, PointGroups.from_scenes(bank)), k=3)
        for s in range(3):
            align = gr.plane_alignment(per_scene.components[s], p["plane"])
            print("%s scene %d: plane alignment %.5f, explained %s" % (kind, s, align, per_scene.explained[s].tolist()))
            assert align >= 0.99
        assert float(per_scene.explained.sum(1).max()) <= 1.0 + 1e-12
        assert bool((per_scene.variance[:, :-1] >= per_scene.variance[:, 1:]).all()) and gr.sign_rule_holds(per_scene.components)
        basis = principal_directions(lib_moments(bank), k=3)
        assert gr.plane_alignment(basis.components[0], p["plane"]) >= 0.99 and gr.sign_rule_holds(basis.components)
        planes[kind] = basis.components[0, :2]
        coords = basis.project(bank)
        assert coords.shape == (bank.rows, 3) and coords.dtype == torch.float32
        assert project_within(coords, basis, stored(bank))
        rgb = basis.colors(bank)
        assert rgb.dtype == torch.uint8 and rgb.shape == (bank.rows, 3) and rgb.device == bank.device
        between, spread = gr.class_colour_stats(rgb, cls)
        print("%s: class mean colours %.1f apart at least, within-class spread %.1f at most" % (kind, between, spread))
        assert between >= gr.PLANT_BETWEEN_MIN and spread <= gr.PLANT_SPREAD_MAX and between > spread
        assert torch.equal(feature_colors(bank), rgb)
        own = feature_colors(bank, per_scene=True)
        assert own.shape == rgb.shape and torch.equal(own[:bank.offsets[1]], per_scene.colors(bank, 0, scene=0))
        xyz = p["xyz"][0]
        cams = R.Cameras.orbit(xyz, 2, image_hw=(48, 64))
        raster = R.rasterize(xyz.to(dev()), cams, radius=0.02, max_px=4)
        scene_rgb = rgb[:bank.offsets[1]]
        picture = raster.colors(scene_rgb)
        assert picture.shape == (2, 48, 64, 3) and picture.dtype == torch.uint8
        covered = raster.point_id >= 0
        assert int(covered.sum()) > 0
        assert torch.equal(picture[covered], scene_rgb[raster.point_id[covered].long()])
    # the two banks find the same plane: the first two components of one, projected on those of the other
    both = float(torch.linalg.svdvals(planes["fp16"].double() @ planes["fp8"].double().t()).min())
    print("fp16 and fp8 bases: smallest singular value %.5f" % both)
    assert both >= 0.99
