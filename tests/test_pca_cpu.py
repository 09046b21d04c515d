"""Host logic of openscene_amd.pca WITHOUT a GPU: the kernels' ops (ops.bank_gram, ops.bank_gram_fp8, and those of the bank
and the search) are replaced by the stand-ins of tests/gram_reference.py, search_reference.py and search_fp8_reference.py;
Moments, the eigen-decomposition, the sign rule, the projection, the colours and the argument checks are the code under
test.  The bound constant of tests/test_gpu_pca.py is measured here, on the same inputs, with the stand-in."""
import os
import re

import numpy as np
import pytest
import torch

import gram_reference as gr
import search_fp8_reference as f8
import search_reference as sr
from openscene_amd import descriptors as D
from openscene_amd import ops
from openscene_amd import pca as P
from openscene_amd import search as S

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exact_bank_search(bank, scene_offsets, queries, k=16, thresholds=None, normalize=True, want_heat=False, max_scene_rows=None, err=None):
    """The heat pass as the fp8 stand-in has it: the float64 score rounded once to fp16 (sr.bank_search accumulates in float32,
    whose error near a zero score is beyond one fp16 rounding; the host code under test is held to exactly that rounding)."""
    heat = sr.scores_f64(bank, queries, normalize).half()
    top_s, top_p, counts = sr.select(heat, scene_offsets.tolist(), k, thresholds)
    return (heat if want_heat else None), top_s, top_p, counts


@pytest.fixture(autouse=True)
def cpu_kernels(monkeypatch):
    monkeypatch.setattr(ops, "bank_append", sr.bank_append)
    monkeypatch.setattr(ops, "bank_check", sr.bank_check)
    monkeypatch.setattr(ops, "bank_search", exact_bank_search)
    monkeypatch.setattr(ops, "bank_append_fp8", f8.bank_append_fp8)
    monkeypatch.setattr(ops, "bank_search_fp8", f8.bank_search_fp8)
    monkeypatch.setattr(ops, "bank_gram", gr.bank_gram)
    monkeypatch.setattr(ops, "bank_gram_fp8", gr.bank_gram_fp8)


def small_bank(dtype="fp16", d=16, sizes=(5, 0, 9), seed=0):
    g = torch.Generator().manual_seed(seed)
    bank = S.FeatureBank(d, CPU, capacity_rows=4, dtype=dtype)
    for i, n in enumerate(sizes):
        bank.add_scene("s%d" % i, sr.unit_rows(n, d, g).half())
    return bank


def planted_bank(dtype="fp16"):
    p = gr.planted()
    bank = S.FeatureBank(gr.PLANT_DIM, CPU, dtype=dtype)
    for i, f in enumerate(p["feats"]):
        bank.add_scene("scene%d" % i, f)
    return p, bank


def stored(bank):
    return bank.features.float() if bank.dtype == "fp16" else bank.dequantize()


def unit64(values):
    x = values.double()
    return x / (x.norm(dim=1, keepdim=True) + 1e-5)


def test_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "openscene_amd.h")).read()
    assert int(re.search(r"#define OSN_BANK_GRAM_SLICE (\d+)", src).group(1)) == ops.BANK_GRAM_SLICE == gr.SLICE
    assert "run/evaluate.py:305" in src[src.index("csrc/gram.hip"):src.index("osn_bank_gram_ws_bytes(")]
    assert gr.R_GRAM == 2.0 ** -10 + 2.0 ** -20 >= (1 + 2.0 ** -11) ** 2 - 1 and gr.R_SUM == 2.0 ** -11


# ---------------------------------------------------------------------------------------------------- the bound constant
def case_on_the_cpu(name):
    """-> (the stand-in's results, the float64 moments on the rounded operands, on the unrounded rows, the stored values)"""
    case = gr.bound_case(name)
    feats = torch.cat(case["scenes"])
    kw = dict(rows=case["rows"], normalize=case["normalize"], n_entries=int(case["starts"][-1]))
    if case["kind"] == "fp8":
        codes, exps = f8.quantize(feats)
        got = gr.bank_gram_fp8(codes, exps, case["starts"], **kw)
        values, kept = f8.dequantize(codes, exps), (codes, exps)
    else:
        got = gr.bank_gram(feats, case["starts"], **kw)
        values, kept = feats.float(), feats
    same = gr.rounded_moments_f64(case["kind"], kept, case["starts"], case["rows"], case["normalize"])
    want = gr.gram_f64(values, case["starts"], case["rows"], case["normalize"])
    return case, got, same, want, values


def test_the_bound_constant_is_four_times_the_stand_ins_worst_ratio():
    worst, worst_name = 0.0, None
    for name in gr.case_names():
        case, (gram, total, count), (s_gram, s_bound, s_total, s_tbound), (want, bound, w_total, w_tbound, w_count), values = \
            case_on_the_cpu(name)
        assert torch.equal(count, w_count), name
        assert torch.equal(gram, gram.transpose(1, 2)), name
        r = max(gr.error_over_abs_sum(gram, s_gram, s_bound), gr.error_over_abs_sum(total, s_total, s_tbound))
        print("%-18s error / abs-sum %.3e" % (name, r))
        if r > worst:
            worst, worst_name = r, name
        # the bound the device is held to holds for the stand-in: the cases lie where the derivation of R does
        r_gram, r_sum = gr.case_r(case, values)
        assert gr.worst_ratio(gram, want, bound, r_gram + gr.GRAM_C)[1] == 0, name
        assert gr.worst_ratio(total, w_total, w_tbound, r_sum + gr.GRAM_C)[1] == 0, name
    print("worst: %s %.3e; recorded %.3e; GRAM_C %.3e" % (worst_name, worst, gr.GRAM_MEASURED_RATIO, gr.GRAM_C))
    # the record is this measurement rounded up in its third digit: GRAM_C stays at 4 x measured and cannot drift upwards
    assert worst <= gr.GRAM_MEASURED_RATIO <= 1.01 * worst, (worst_name, worst)
    assert gr.GRAM_C == 4 * gr.GRAM_MEASURED_RATIO and gr.GRAM_C <= gr.GRAM_C_CAP


@pytest.mark.parametrize("kind", ["fp16", "fp8"])
def test_components_below_the_normal_range_need_and_meet_the_absolute_terms(kind):
    case = gr.tiny_case(kind)
    feats = case["scenes"][0]
    kw = dict(rows=case["rows"], normalize=True, n_entries=int(case["starts"][-1]))
    if kind == "fp8":
        codes, exps = f8.quantize(feats)
        gram, total, count = gr.bank_gram_fp8(codes, exps, case["starts"], **kw)
        values = f8.dequantize(codes, exps)
    else:
        gram, total, count = gr.bank_gram(feats, case["starts"], **kw)
        values = feats.float()
    want, bound, w_total, w_tbound, w_count = gr.gram_f64(values, case["starts"], case["rows"], True)
    x = unit64(values[case["rows"]])
    assert int(((x.abs() < 2.0 ** -14) & (x != 0)).sum()) > 100                  # the case is about them
    plain = gr.worst_ratio(gram, want, bound, gr.R_GRAM + gr.GRAM_C)
    print("%s: without the absolute terms %d elements beyond, worst %.2f" % (kind, plain[1], plain[0]))
    assert plain[1] > 0                                                         # R alone does not cover a one-row group
    g_slack, s_slack = gr.tiny_slack(w_tbound, w_count)
    assert gr.beyond(gram, want, bound, gr.R_GRAM + gr.GRAM_C, g_slack)[1] == 0
    assert gr.beyond(total, w_total, w_tbound, gr.R_SUM + gr.GRAM_C, s_slack)[1] == 0
    assert torch.equal(count, w_count)


def test_the_bound_cases_cover_the_lengths_the_dims_and_one_wide_case_across_a_slice_edge():
    s = gr.SLICE
    assert gr.FULL == (0, 1, s - 1, s, s + 1, 2 * s + 3)
    wide_and_long = 0
    for name in gr.case_names():
        case = gr.bound_case(name)
        d = case["scenes"][0].shape[1]
        longest = int((case["starts"][1:] - case["starts"][:-1]).max())
        wide_and_long += d >= 768 and longest > s
        if d <= 24 and name.split("-")[2] in gr.VARIANTS:
            assert (case["starts"][1:] - case["starts"][:-1]).tolist() == list(gr.FULL)
        if case["rows"] is not None and case["rows"].numel():
            assert case["rows"].unique().numel() < case["rows"].numel()           # duplicates
    assert wide_and_long == 1


# ---------------------------------------------------------------------------------------------------- Moments
@pytest.mark.parametrize("dtype", ["fp16", "fp8"])
def test_covariance_against_numpy_on_the_stored_rows(dtype):
    bank = small_bank(dtype, sizes=(6, 0, 10))
    groups = D.PointGroups.from_lists([[0, 1, 2, 7, 9], [], [3, 3, 9], [4], [15, 7, 8, 1, 2, 3, 4, 5, 6]])
    for normalize in (True, False):
        m = P.moments(bank, groups, normalize=normalize)
        assert m.shape == (5,) and m.dim == 16 and m.count.tolist() == [5, 0, 3, 1, 9] and m.gram.shape == (5, 16, 16)
        x = unit64(stored(bank)) if normalize else stored(bank).double()
        cov = m.covariance()
        assert cov.dtype == torch.float64 and cov.shape == (5, 16, 16)
        assert bool((cov[[1, 3]] == 0).all()) and bool((m.mean[1] == 0).all())    # fewer than two rows
        for g in (0, 2, 4):
            rows = groups.rows[int(groups.starts[g]):int(groups.starts[g + 1])]
            want = np.cov(x[rows].numpy(), rowvar=False, bias=True)
            # the operands are rounded to fp16 (a relative 2^-11 each, exact when not normalised); entries of a unit row of 16 are below 1
            assert np.abs(cov[g].numpy() - want).max() <= (3 * 2.0 ** -11 if normalize else 1e-6)
            assert torch.allclose(m.mean[g].double(), x[rows].mean(0), atol=2.0 ** -11 if normalize else 1e-6)
    whole = P.moments(bank)
    assert whole.shape == (1,) and whole.count.tolist() == [16]
    scenes = P.moments(bank, D.PointGroups.from_scenes(bank))
    assert scenes.count.tolist() == [6, 0, 10]
    import openscene_amd
    assert torch.equal(openscene_amd.moments(bank).gram, whole.gram)


# ---------------------------------------------------------------------------------------------------- principal directions
def reference_basis(x, k=3, center=True):
    """float64 on the unrounded rows x [n, d]: (components [k, d], eigenvalues [k], trace)"""
    m = x.t() @ x / x.shape[0]
    if center:
        mu = x.mean(0)
        m = m - mu[:, None] * mu[None, :]
    vals, vecs = torch.linalg.eigh(m)
    return vecs.flip(-1)[:, :k].t(), vals.flip(-1)[:k], float(torch.diagonal(m).sum())


def test_the_float64_reference_is_clearly_inside_the_planted_conditions():
    p = gr.planted()
    for f in p["feats"] + [torch.cat(p["feats"])]:
        comps, vals, trace = reference_basis(unit64(f.float()))
        align = gr.plane_alignment(comps, p["plane"])
        print("reference: plane alignment %.6f, explained %s" % (align, (vals / trace).tolist()))
        assert align >= 0.999                                  # ten times closer to 1 than the 0.99 asked of the library
        assert float(vals[1] / vals[2]) > 20                   # the plane stands well clear of the noise


@pytest.mark.parametrize("dtype", ["fp16", "fp8"])
def test_principal_directions_of_the_planted_scenes(dtype):
    p, bank = planted_bank(dtype)
    basis = P.principal_directions(P.moments(bank, D.PointGroups.from_scenes(bank)), k=3)
    assert basis.components.shape == (3, 3, gr.PLANT_DIM) and basis.components.dtype == torch.float32
    assert basis.mean.shape == (3, gr.PLANT_DIM) and basis.variance.shape == (3, 3) and basis.total_variance.shape == (3,)
    for s in range(3):
        align = gr.plane_alignment(basis.components[s], p["plane"])
        print("%s scene %d: plane alignment %.5f" % (dtype, s, align))
        assert align >= 0.99
    assert float(basis.explained.sum(1).max()) <= 1.0 + 1e-12
    assert bool((basis.variance[:, :-1] >= basis.variance[:, 1:]).all())
    assert torch.allclose(basis.explained, basis.variance / basis.total_variance[:, None])
    assert gr.sign_rule_holds(basis.components)
    assert torch.allclose(basis.components.double().norm(dim=-1), torch.ones(3, 3, dtype=torch.float64), atol=1e-6)
    whole = P.principal_directions(P.moments(bank), k=2)
    assert whole.components.shape == (1, 2, gr.PLANT_DIM) and gr.plane_alignment(whole.components[0], p["plane"]) >= 0.99


def test_the_sign_rule_on_constructed_moments():
    d = 4
    v = torch.tensor([[0.5, -0.5, 0.5, -0.5], [-0.1, 0.2, -0.9, 0.3]], dtype=torch.float64)
    v[1] = v[1] - (v[1] @ v[0]) * v[0] / (v[0] @ v[0])
    v = v / v.norm(dim=1, keepdim=True)
    gram = (3.0 * v[0][:, None] * v[0][None, :] + 1.0 * v[1][:, None] * v[1][None, :])[None].float()
    m = P.Moments(torch.tensor([1]), torch.zeros(1, d), gram, (1,))
    basis = P.principal_directions(m, k=2, center=False)
    c = basis.components[0]
    assert torch.allclose(c[0].double().abs(), v[0].abs(), atol=1e-6) and float(c[0, 0]) > 0      # a four-way tie: the lowest index
    assert torch.allclose(c[1].double().abs(), v[1].abs(), atol=1e-6) and float(c[1, c[1].abs().argmax()]) > 0
    assert torch.allclose(basis.variance[0], torch.tensor([3.0, 1.0], dtype=torch.float64), atol=1e-5)
    assert bool((basis.mean == 0).all())


@pytest.mark.parametrize("dtype", ["fp16", "fp8"])
def test_without_centring_a_groups_first_direction_is_its_mean_direction(dtype):
    """One group per planted class: its rows stand around one direction, which the second moment's leading eigenvector is.
    (Over a whole scene the second moment of orthogonal classes is diag(shares): its leading eigenvector is the largest
    class, not the mean direction -- the claim is a group's, where one direction dominates.)"""
    p, bank = planted_bank(dtype)
    groups = D.PointGroups.from_labels(torch.cat(p["cls"]), 3)
    m = P.moments(bank, groups)
    basis = P.principal_directions(m, k=1, center=False)
    assert bool((basis.mean == 0).all())
    mean_dir = torch.nn.functional.normalize(m.mean.double(), dim=1)
    for c in range(3):
        assert abs(float(basis.components[c, 0].double() @ mean_dir[c])) >= 0.999      # (the sign is the sign rule's)
        assert abs(float(basis.components[c, 0].double() @ p["dirs"][c].double())) >= 0.99
    assert float(basis.explained.min()) > 0.9
    # and over the scenes, what does hold there: the second moment of a scene is diag(shares) in the classes' basis plus noise, so
    # the first uncentred component is the scene's largest class, the cosine with the scene's mean direction is
    # max(shares) / |shares| (0.913, 0.816, 0.913), and the eigenvalues are the shares themselves
    ms = P.moments(bank, D.PointGroups.from_scenes(bank))
    scenes = P.principal_directions(ms, k=3, center=False)
    assert bool((scenes.mean == 0).all()) and gr.sign_rule_holds(scenes.components)
    scene_mean = torch.nn.functional.normalize(ms.mean.double(), dim=1)
    for s, shares in enumerate(gr.PLANT_SHARES):
        share = torch.tensor(shares, dtype=torch.float64) / sum(shares)
        first = scenes.components[s, 0].double()
        assert abs(float(first @ p["dirs"][int(share.argmax())].double())) >= 0.99
        assert abs(abs(float(first @ scene_mean[s])) - float(share.max() / share.norm())) <= 0.02
        assert torch.allclose(scenes.variance[s], share.sort(descending=True)[0], atol=0.02)
    assert float(scenes.explained.sum(1).max()) <= 1.0 + 1e-12 and float(scenes.explained.sum(1).min()) > 0.9


# ---------------------------------------------------------------------------------------------------- project, colours
def project_within(coords, basis, values, group=0):
    """tests/test_gpu_pca.py's: one fp16 rounding of the score plus the float32 roundings of the offset and the difference"""
    x = unit64(values)
    c = basis.components[group].half().double()
    score = x @ c.t()
    offset = c @ basis.mean[group].double()
    err = (coords.double() - (score - offset)).abs()
    lim = 2.0 ** -11 * score.abs().clamp(min=2.0 ** -14) + 2.0 ** -23 * (offset.abs() + score.abs())
    print("projection: worst err / limit %.3f" % float((err / lim).max()))
    return bool((err <= lim).all())


@pytest.mark.parametrize("dtype", ["fp16", "fp8"])
def test_projection_and_colours_of_the_planted_bank(dtype):
    p, bank = planted_bank(dtype)
    cls = torch.cat(p["cls"])
    basis = P.principal_directions(P.moments(bank), k=3)
    coords = basis.project(bank)
    assert coords.shape == (bank.rows, 3) and coords.dtype == torch.float32
    assert project_within(coords, basis, stored(bank))
    one = basis.project(bank, scene="scene1")
    assert torch.equal(one, coords[bank.offsets[1]:bank.offsets[2]])
    rgb = basis.colors(bank)
    assert rgb.dtype == torch.uint8 and rgb.shape == (bank.rows, 3)
    # the quantile map itself, restated in float64 (the library maps in float32: a level apart at a tie, at the most)
    assert int((rgb.int() - gr.colors_f64(coords).int()).abs().max()) <= 1
    between, spread = gr.class_colour_stats(rgb, cls)
    comps, _, _ = reference_basis(unit64(stored(bank)))
    x = unit64(stored(bank))
    ref_between, ref_spread = gr.class_colour_stats(gr.colors_f64((x - x.mean(0)) @ comps.t()), cls)
    print("%s: between %.1f spread %.1f; float64 reference: between %.1f spread %.1f" % (dtype, between, spread, ref_between, ref_spread))
    assert ref_between >= 2 * gr.PLANT_BETWEEN_MIN and ref_spread <= gr.PLANT_SPREAD_MAX / 2
    assert between >= gr.PLANT_BETWEEN_MIN and spread <= gr.PLANT_SPREAD_MAX and between > spread
    assert torch.equal(P.feature_colors(bank), rgb)
    own = P.feature_colors(bank, per_scene=True)
    per_scene = P.principal_directions(P.moments(bank, D.PointGroups.from_scenes(bank)), k=3)
    for s in range(3):
        assert torch.equal(own[bank.offsets[s]:bank.offsets[s + 1]], per_scene.colors(bank, s, scene=s))
    import openscene_amd
    assert torch.equal(openscene_amd.feature_colors(bank), rgb)


def test_a_constant_component_is_drawn_at_128():
    d = 16
    bank = S.FeatureBank(d, CPU, capacity_rows=4)
    x = torch.zeros(50, d)
    x[:, 0] = 1.0
    x[:, 1] = torch.linspace(-0.5, 0.5, 50)
    bank.add_scene("line", x.half())                                            # the rows vary along one direction only
    comps = torch.zeros(1, 3, d)
    comps[0, 0, 1] = comps[0, 1, 5] = comps[0, 2, 0] = 1.0                      # along the line, a direction nothing varies in, the constant
    basis = P.Basis(torch.zeros(1, d), comps, torch.ones(1, 3, dtype=torch.float64), torch.ones(1, dtype=torch.float64), normalize=False)
    rgb = basis.colors(bank, lo=0.0, hi=1.0)
    assert rgb[:, 1].tolist() == [128] * 50 and rgb[:, 2].tolist() == [128] * 50
    assert int(rgb[0, 0]) == 0 and int(rgb[-1, 0]) == 255 and bool((rgb[1:, 0] >= rgb[:-1, 0]).all())
    empty = S.FeatureBank(d, CPU, capacity_rows=4)
    assert basis.colors(empty).shape == (0, 3) and basis.project(empty).shape == (0, 3)


# ---------------------------------------------------------------------------------------------------- arguments
def test_argument_errors():
    bank = small_bank()
    with pytest.raises(TypeError):
        P.moments(bank.features)                                                # the wrong kind of bank
    with pytest.raises(TypeError):
        P.moments(bank, (torch.tensor([0, 14]), None))
    far = D.PointGroups(torch.zeros(2, dtype=torch.int64, device="meta"), None, n_entries=0, _checked=True)
    with pytest.raises(ValueError, match="device"):
        P.moments(bank, far)
    wide = S.FeatureBank(ops.BANK_POOL_MAX_DIM + 16, CPU, capacity_rows=2)
    wide.add_scene("w", torch.ones(2, ops.BANK_POOL_MAX_DIM + 16, dtype=torch.float16))
    with pytest.raises(ValueError, match=str(ops.BANK_POOL_MAX_DIM)):
        P.moments(wide)
    big = S.FeatureBank(1024, CPU, capacity_rows=2)
    big.add_scene("b", torch.ones(1, 1024, dtype=torch.float16))
    with pytest.raises(ValueError, match=r"513 groups x 1024 x 1024 float32 are 2151677952 bytes \(2\.00 GiB\)"):
        P.moments(big, D.PointGroups.from_lists([[0]] * 513))                   # refused before anything is allocated
    assert P.moments(big, D.PointGroups.from_lists([[0]] * 2)).gram.shape == (2, 1024, 1024)
    m = P.moments(bank)
    with pytest.raises(TypeError):
        P.principal_directions(m.gram)
    for k in (0, 17):
        with pytest.raises(ValueError, match="k must be"):
            P.principal_directions(m, k=k)
    assert P.principal_directions(m, k=16).components.shape == (1, 16, 16)
    two = P.principal_directions(m, k=2)
    with pytest.raises(ValueError, match="three components"):
        two.colors(bank)
    with pytest.raises(ValueError):
        P.principal_directions(m, k=3).colors(bank, lo=0.9, hi=0.1)
    with pytest.raises(TypeError):
        two.project(bank.features)
    with pytest.raises(IndexError):
        two.project(bank, group=1)
    with pytest.raises(ValueError, match="features"):
        two.project(S.FeatureBank(32, CPU, capacity_rows=2))
    with pytest.raises(TypeError):
        P.feature_colors(bank.features)


def test_the_checks_the_gram_ops_share_with_the_pool():
    """ops.bank_gram / bank_gram_fp8 run these before anything is allocated or launched (no device is needed to call them)."""
    starts, rows = torch.tensor([0, 2]), torch.tensor([0, 1])
    with pytest.raises(ValueError, match="multiple of 16"):
        ops._bank_groups(24, 16, CPU, starts, rows, None, None)                 # an fp8 bank with d % 16 != 0
    with pytest.raises(ValueError, match="multiple of 8"):
        ops._bank_groups(20, 8, CPU, starts, rows, None, None)
    with pytest.raises(ValueError, match="at most"):
        ops._bank_groups(ops.BANK_POOL_MAX_DIM + 16, 16, CPU, starts, rows, None, None)
    with pytest.raises(TypeError):
        ops._bank_groups(16, 8, CPU, starts.int(), rows, None, None)
    with pytest.raises(TypeError):
        ops._bank_groups(16, 8, CPU, starts, rows.int(), None, None)
    with pytest.raises(ValueError, match="device"):
        ops._bank_groups(16, 8, CPU, starts.to("meta"), rows, None, None)
    with pytest.raises(ValueError, match="device"):
        ops._bank_groups(16, 8, CPU, starts, rows.to("meta"), None, None)
    with pytest.raises(ValueError, match="n_entries"):
        ops._bank_groups(16, 8, CPU, starts, None, None, None)
    with pytest.raises(ValueError):
        ops._bank_groups(16, 8, CPU, starts, rows, 3, None)
    with pytest.raises(ValueError, match="err"):
        ops._bank_groups(16, 8, CPU, starts, rows, None, torch.zeros(1))
    s, g, r, n_entries, err, own = ops._bank_groups(16, 8, CPU, starts, rows, None, None)
    assert g == 1 and n_entries == 2 and own and err.dtype == torch.int32
    with pytest.raises(TypeError):
        ops._fp16_bank(torch.zeros(2, 16))
    with pytest.raises(ValueError):
        ops._fp16_bank(torch.zeros(2, 32, dtype=torch.float16)[:, ::2])
    with pytest.raises(TypeError):
        ops._fp8_bank(torch.zeros(2, 16, dtype=torch.int8), torch.zeros(2, dtype=torch.int8))
    with pytest.raises(TypeError):
        ops._fp8_bank(torch.zeros(2, 16, dtype=torch.uint8), torch.zeros(2, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops._fp8_bank(torch.zeros(2, 16, dtype=torch.uint8), torch.zeros(3, dtype=torch.int8))
    assert tuple(ops._fp8_bank(torch.zeros(2, 16, dtype=torch.uint8), torch.zeros(2, dtype=torch.int8))) == (2, 16)


@pytest.mark.parametrize("dtype", ["fp16", "fp8"])
def test_a_row_outside_the_bank_raises_and_leaves_the_bank_usable(dtype):
    bank = small_bank(dtype)
    good = P.moments(bank).gram
    for rows in ([0, bank.rows], [-1, 2]):
        with pytest.raises(RuntimeError):
            P.moments(bank, D.PointGroups.from_lists([rows]))
        assert int(bank._err_word().item()) == 0
    assert torch.equal(P.moments(bank).gram, good)
