"""Two banks searched as one on the device (csrc/search.hip: osn_bank_search_ensemble, osn_bank_search_ensemble_fp8).

The definitions (include/openscene_amd.h, tests/search_ensemble_reference.py) are stated on what the plain and the contrast search
write for each bank alone, so the ensemble is held to them bit for bit: heat, source, top-k and counts equal what the pick gives
on the two banks' own results.  No tolerance anywhere.  The float64 contract of the pick itself (where the score intervals of
tests/search_bounds.py decide it) is checked on top.

Inputs: search_reference.unit_rows / text of seed 7; every seventh row of B is zero, as for points fusion never saw."""
import functools

import pytest
import torch

import search_bounds as sb
import search_ensemble_reference as er
import search_reference as sr
from search_reference import text, unit_rows

pytestmark = pytest.mark.gpu

K = 16
SCENES = (0, 7, 993)          # an empty scene, one shorter than k, 1000 rows in all: the last workgroup is partial
N = sum(SCENES)
WIDTHS = (64, 272)            # one partial 128-wide chunk; two full chunks and a tail (a multiple of 16 for the fp8 bank)
SETS = ((1, 0), (5, 4), (33, 0), (65, 33), (130, 33))   # (queries, negatives): one column tile, two, a group boundary, both cross it
KINDS = ("fp16", "fp8")
MODES = er.MODES
CONTRACT = ((64, 1), (64, 5), (64, 20), (272, 33), (272, 130), (768, 65))      # (d, Q) of the float64 contract


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
    """(rows of A [1000, d], rows of B, queries fp16 [130, d], negatives fp16 [33, d]) of seed 7; shared, never modified."""
    g = torch.Generator().manual_seed(7)
    a, b = unit_rows(N, d, g), unit_rows(N, d, g)
    b[::7] = 0
    return a, b, text(SETS[-1][0], d, g), text(SETS[-1][1], d, g)


@functools.lru_cache(maxsize=None)
def the_banks(kind, d):
    a, b = inputs(d)[:2]
    return make_bank(kind, d, torch.split(a, SCENES)), make_bank(kind, d, torch.split(b, SCENES))


def queries(d, q, m):
    _, _, t, neg = inputs(d)
    return t[:q].to(dev()), (neg[:m].to(dev()) if m else None)


def same_result(a, b):
    return (sr.same_bits(a.heat, b.heat) and sr.same_bits(a.topk_scores, b.topk_scores) and torch.equal(a.topk_points, b.topk_points)
            and (a.counts is None) == (b.counts is None) and (a.counts is None or torch.equal(a.counts, b.counts)))


def composed_equals(bank_a, bank_b, t, neg, mode, normalize, tau=0.1, threshold=0.3):
    """the ensemble search equals the definitions applied to the two banks' own results, bit for bit -> (result, source)"""
    from openscene_amd.search import search
    thr = 0.5 if neg is not None else threshold
    res = search(bank_a, t, k=K, thresholds=thr, normalize=normalize, return_heat=True, negatives=neg, temperature=tau,
                 ensemble=bank_b, ensemble_mode=mode)
    heat, source = er.compose(search, bank_a, bank_b, t, mode, normalize, neg, tau)
    assert res.ensemble_mode == mode and res.source.dtype == torch.bool and res.source.shape == source.shape
    assert torch.equal(res.source, source)
    assert sr.same_bits(res.heat, heat)
    sr.check_selection(res, heat, bank_a.offsets, K, torch.full((t.shape[0],), thr, device=dev()))
    return res, source


# ------------------------------------------------------------------------------------------------- 1: composition
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_the_ensemble_is_the_pick_on_the_two_banks_own_results_bit_for_bit(kind, normalize, mode, d):
    bank_a, bank_b = the_banks(kind, d)
    for q, m in SETS:
        t, neg = queries(d, q, m)
        _, source = composed_equals(bank_a, bank_b, t, neg, mode, normalize)
        share = source.double().mean().item()
        print("%s normalize=%d %s d=%d q=%d m=%d: %.1f %% from B" % (kind, normalize, mode, d, q, m, 100 * share))
        assert 0.25 <= share <= 0.75                        # a kernel that always answers A (or B) cannot pass


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_composition_at_768_columns_wide_rows(kind, mode):
    bank_a, bank_b = the_banks(kind, 768)
    t, neg = queries(768, 65, 33)
    for negatives in (None, neg):
        _, source = composed_equals(bank_a, bank_b, t, negatives, mode, True)
        assert 0.25 <= source.double().mean().item() <= 0.75


# ------------------------------------------------------------------------------------------ 2: the float64 contract
@pytest.mark.parametrize("kind", KINDS)
def test_the_pick_is_the_one_float64_decides(kind):
    from openscene_amd.search import search
    for d, q in CONTRACT:
        a, b, t_all, _ = inputs(d)
        bank_a, bank_b = the_banks(kind, d)
        va, vb = er.stored_values(a, kind), er.stored_values(b, kind)
        t = t_all[:q]
        for mode in MODES:
            for normalize in ((True,) if mode == "vocabulary" else (True, False)):
                ref_a, ref_b = (sb.interval(v, t.double().numpy(), normalize) for v in (va, vb))
                must_b, must_a = er.decided(mode, ref_a, ref_b)
                undecided = 1.0 - float((must_a | must_b).mean())
                res = search(bank_a, t.to(dev()), k=K, normalize=normalize, return_heat=True, ensemble=bank_b, ensemble_mode=mode)
                got = res.source.cpu().numpy()
                print("%s %s normalize=%d d=%d q=%d: %.3f %% undecided by the intervals" % (kind, mode, normalize, d, q, 100 * undecided))
                assert got[must_b].all() and not got[must_a].any()
                assert undecided <= 0.01


# -------------------------------------------------------------------------------------------------------- 3: closure
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_searching_the_selected_bank_gives_the_vocabulary_ensemble(kind, normalize):
    from openscene_amd.search import search
    d = 272
    bank_a, bank_b = the_banks(kind, d)
    t, neg = queries(d, 65, 33)
    for negatives in (None, neg):
        kw = dict(k=K, thresholds=0.4, normalize=normalize, return_heat=True, negatives=negatives, temperature=0.05)
        res = search(bank_a, t, ensemble=bank_b, **kw)
        picked = bank_a.select(bank_b, res.source)
        assert picked.dtype == kind and picked.names == bank_a.names and picked.offsets == bank_a.offsets
        again = search(picked, t, **kw)
        assert same_result(res, again) and again.source is None and again.ensemble_mode is None


# --------------------------------------------------------------------------------------------------- 4: independence
@pytest.mark.parametrize("kind", KINDS)
def test_a_query_mode_column_depends_on_its_query_alone(kind):
    from openscene_amd.search import search
    d = 272
    bank_a, bank_b = the_banks(kind, d)
    t, neg = queries(d, 65, 33)
    for negatives in (None, neg):
        kw = dict(k=K, return_heat=True, negatives=negatives, ensemble=bank_b, ensemble_mode="query")
        whole = search(bank_a, t, **kw)
        for j in (0, 31, 32, 64):
            one = search(bank_a, t[j:j + 1], **kw)
            assert sr.same_bits(one.heat[:, 0], whole.heat[:, j]) and torch.equal(one.source[:, 0], whole.source[:, j])
            assert sr.same_bits(one.topk_scores[:, 0], whole.topk_scores[:, j]) and torch.equal(one.topk_points[:, 0], whole.topk_points[:, j])


@pytest.mark.parametrize("kind", KINDS)
def test_permuting_the_queries_permutes_the_columns_of_a_vocabulary_search(kind):
    from openscene_amd.search import search
    d = 272
    bank_a, bank_b = the_banks(kind, d)
    t, neg = queries(d, 65, 33)
    perm = torch.randperm(65, generator=torch.Generator().manual_seed(3)).to(dev())
    for negatives in (None, neg):
        kw = dict(k=K, return_heat=True, negatives=negatives, ensemble=bank_b)
        a, b = search(bank_a, t, **kw), search(bank_a, t[perm].contiguous(), **kw)
        assert torch.equal(a.source, b.source) and sr.same_bits(a.heat[:, perm], b.heat)
        assert sr.same_bits(a.topk_scores[:, perm], b.topk_scores) and torch.equal(a.topk_points[:, perm], b.topk_points)
        fewer = search(bank_a, t[:5], **kw)                     # and a column DOES depend on the other queries of the call
        assert not torch.equal(fewer.source, a.source)


# ------------------------------------------------------------------------------------------------- 5: self-ensemble
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_bank_with_itself_is_the_plain_search(kind, mode):
    from openscene_amd.search import search
    d = 272
    bank_a = the_banks(kind, d)[0]
    t, neg = queries(d, 130, 33)
    for normalize in (True, False):
        for negatives in (None, neg):
            kw = dict(k=K, thresholds=0.4, normalize=normalize, return_heat=True, negatives=negatives)
            res = search(bank_a, t, ensemble=bank_a, ensemble_mode=mode, **kw)
            assert same_result(res, search(bank_a, t, **kw))
            assert not res.source.any() and res.source.shape == ((N,) if mode == "vocabulary" else (N, 130))


# --------------------------------------------------------------------------------------------------- 6: planted rows
PLANTS = ("zero_b", "zero_a", "zero_both", "nan_a", "nan_b", "equal", "negated", "inf_b")
BASES = (0, 500, 990)         # the first workgroup, the middle, the partial last one (rows 896 .. 999)


@functools.lru_cache(maxsize=None)
def planted(d):
    a, b = (x.clone() for x in inputs(d)[:2])
    for base in BASES:
        r = {name: base + i for i, name in enumerate(PLANTS)}
        b[r["zero_b"]] = 0
        a[r["zero_a"]] = 0                                   # (rows 1, 501, 991 of B: none of its zeroed sevenths)
        a[r["zero_both"]] = 0
        b[r["zero_both"]] = 0
        a[r["nan_a"], 5] = float("nan")
        b[r["nan_b"], 9] = float("nan")
        b[r["equal"]] = a[r["equal"]]
        b[r["negated"]] = -a[r["negated"]]
        b[r["inf_b"], 3] = float("inf")
    return a, b


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_planted_rows_follow_the_definitions_exactly(kind, normalize, mode):
    d = 64
    a, b = planted(d)
    bank_a, bank_b = make_bank(kind, d, torch.split(a, SCENES)), make_bank(kind, d, torch.split(b, SCENES))
    for q, m in ((5, 0), (65, 33)):
        t, neg = queries(d, q, m)
        res, source = composed_equals(bank_a, bank_b, t, neg, mode, normalize)          # (same_bits: -0 is not +0)
        for base in BASES:
            r = {name: base + i for i, name in enumerate(PLANTS)}
            for name in ("zero_both", "nan_a", "nan_b", "equal"):
                assert not res.source[r[name]].any(), (name, base)
            assert torch.isnan(res.heat[r["nan_a"]]).all()
            assert not torch.isnan(res.heat[r["nan_b"]]).any()
            if m == 0:
                assert (res.heat[r["zero_both"]].view(torch.int16) == 0).all()          # +0.0, bit for bit
                if normalize and mode == "vocabulary":
                    assert not res.source[r["inf_b"]]                                   # B's normalised row is NaN
                if mode == "query":                                                     # the larger of s and -s, of s and 0
                    assert (res.heat[r["negated"]].float() >= 0).all() and (res.heat[r["zero_b"]].float() >= 0).all()
                    assert (res.heat[r["zero_a"]].float() >= 0).all()


# ------------------------------------------------------------------------------------------ 7: small banks, repeats
@pytest.mark.parametrize("kind", KINDS)
def test_one_row_and_129_rows_and_two_calls_agree(kind):
    from openscene_amd.search import search
    d = 272
    a, b = inputs(d)[:2]
    t, neg = queries(d, 65, 33)
    for n in (1, 129):
        bank_a, bank_b = make_bank(kind, d, [a[1:1 + n]]), make_bank(kind, d, [b[1:1 + n]])
        for mode in MODES:
            for negatives in (None, neg):
                res, _ = composed_equals(bank_a, bank_b, t, negatives, mode, True)
                again, _ = composed_equals(bank_a, bank_b, t, negatives, mode, True)
                assert same_result(res, again) and torch.equal(res.source, again.source)
    bank_a, bank_b = the_banks(kind, d)
    kw = dict(k=K, thresholds=0.5, return_heat=True, negatives=neg, temperature=0.01, ensemble=bank_b)
    x, y = search(bank_a, t, **kw), search(bank_a, t, **kw)
    assert same_result(x, y) and torch.equal(x.source, y.source)
    no_heat = search(bank_a, t, **dict(kw, return_heat=False, ensemble_mode="query"))
    assert no_heat.heat is None and no_heat.source is None and no_heat.ensemble_mode == "query"
    with_heat = search(bank_a, t, **dict(kw, ensemble_mode="query"))
    assert torch.equal(no_heat.topk_points, with_heat.topk_points) and torch.equal(no_heat.counts, with_heat.counts)


@pytest.mark.parametrize("mode", MODES)
def test_heat_map_with_an_ensemble_is_the_search_of_two_one_scene_banks(mode):
    from openscene_amd.search import heat_map, search
    d = 64
    a, b = inputs(d)[:2]
    t, neg = queries(d, 5, 4)
    inv = torch.tensor([4, 0, 0, 199, 2, 7])
    for negatives in (None, neg):
        hm = heat_map(a[:200].to(dev()), t, inv.to(dev()), negatives=negatives, temperature=0.05, ensemble=b[:200].to(dev()),
                      ensemble_mode=mode)
        res = search(make_bank("fp16", d, [a[:200][inv]]), t, k=1, return_heat=True, negatives=negatives, temperature=0.05,
                     ensemble=make_bank("fp16", d, [b[:200][inv]]), ensemble_mode=mode)
        assert hm.shape == (6, 5) and sr.same_bits(hm, res.heat) and sr.same_bits(hm[1], hm[2])
