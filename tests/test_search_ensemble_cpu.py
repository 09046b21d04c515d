"""Host logic of the two-bank search WITHOUT a GPU: ops.bank_search_ensemble / ops.bank_search_ensemble_fp8 are replaced by the
torch stand-ins of tests/search_ensemble_reference.py (the definitions, composed from the plain and contrast stand-ins); the
argument checks of openscene_amd.search, SearchResult's new fields, FeatureBank.select, heat_map(ensemble=), the registration of
the two C entries and their own argument checks are the code under test."""
import ctypes
import os
import re

import pytest
import torch

import search_bounds as sb
import search_contrast_reference as cr
import search_ensemble_reference as er
import search_fp8_reference as f8
import search_reference as sr
from openscene_amd import _lib, ops
from openscene_amd import search as S

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("osn_bank_search_ensemble", "osn_bank_search_ensemble_fp8")


@pytest.fixture(autouse=True)
def cpu_kernels(monkeypatch):
    calls = []

    def spy(name, f):
        def g(*a, **kw):
            calls.append((name, len(a), sorted(kw)))
            return f(*a, **kw)
        return g
    monkeypatch.setattr(ops, "bank_append", sr.bank_append)
    monkeypatch.setattr(ops, "bank_check", sr.bank_check)
    monkeypatch.setattr(ops, "bank_append_fp8", f8.bank_append_fp8)
    monkeypatch.setattr(ops, "bank_search", spy("search", cr.bank_search))              # (the current signatures)
    monkeypatch.setattr(ops, "bank_search_fp8", spy("search_fp8", cr.bank_search_fp8))
    monkeypatch.setattr(ops, "bank_search_ensemble", spy("ensemble", er.bank_search_ensemble))
    monkeypatch.setattr(ops, "bank_search_ensemble_fp8", spy("ensemble_fp8", er.bank_search_ensemble_fp8))
    return calls


def unit(n, d, gen):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=1)


def bank_of(rows, kind, d=16, names=None, device=CPU):
    bank = S.FeatureBank(d, device, dtype=kind)
    for i, r in enumerate(rows):
        bank.add_scene(names[i] if names else "s%d" % i, r)
    return bank


def two_banks(gen, kind, d=16):
    a = [unit(3, d, gen), torch.zeros(0, d), unit(50, d, gen)]
    b = [unit(3, d, gen), torch.zeros(0, d), unit(50, d, gen)]
    b[2][::7] = 0
    return bank_of(a, kind, d), bank_of(b, kind, d)


# ---------------------------------------------------------------------------------------------------- registration
def test_the_header_the_prototypes_and_the_build_name_the_entries():
    src = open(os.path.join(ROOT, "include", "openscene_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = {n for n in re.findall(r"\b(osn_[a-z0-9_]+)\s*\(", code) if n.startswith("osn_bank_search_ensemble")}
    assert declared == set(ENTRIES) == {n for n in _lib.PROTOTYPES if n.startswith("osn_bank_search_ensemble")}
    for name in ENTRIES:
        decl = re.search(r"\b%s\s*\((.*?)\);" % name, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.PROTOTYPES[name][1]), name
        plain = name.replace("_ensemble", "")
        assert len(_lib.PROTOTYPES[name][1]) == len(_lib.PROTOTYPES[plain][1]) + (1 if name == ENTRIES[0] else 2) + 5
    assert src.index("int osn_bank_search_contrast_fp8(") < src.index("int osn_bank_search_ensemble(") < src.index("csrc/pool.hip")
    block = src[src.index("int osn_bank_search_contrast_fp8("):src.index("int osn_bank_search_ensemble(")]
    for word in ("run/evaluate.py:302-324", "s_X(p, j)", "n_X(p, j)", "r_X(p, j)", "vocabulary", "max_j n_A(p, j) < max_j n_B(p, j)",
                 "propagates NaN", "-0 against +0", "whatever normalize is", "x_A(p, j) < x_B(p, j)", "osn_bank_search_ws_bytes"):
        assert word in block, word
    import __graft_entry__ as ge
    ge.build()
    h = _lib.load()
    assert all(hasattr(h, name) for name in ENTRIES)
    from openscene_amd import build
    assert "search.hip" in build.SOURCES
    assert ops.BANK_ENSEMBLE_MODES == er.MODES == ("vocabulary", "query")


# ---------------------------------------------------------------------------------------------------- argument errors
def test_banks_that_do_not_go_together_raise_naming_the_first_difference():
    g = torch.Generator().manual_seed(0)
    a16, b16 = two_banks(g, "fp16")
    a8, _ = two_banks(g, "fp8")
    t = unit(3, 16, g).half()
    with pytest.raises(TypeError, match="FeatureBank"):
        S.search(a16, t, ensemble=b16.features)
    with pytest.raises(ValueError, match="kind"):
        S.search(a16, t, ensemble=a8)
    with pytest.raises(ValueError, match="kind"):
        S.search(a8, t, ensemble=a16)
    wide = bank_of([unit(3, 32, g), torch.zeros(0, 32), unit(50, 32, g)], "fp16", 32)
    with pytest.raises(ValueError, match="dim"):
        S.search(a16, t, ensemble=wide)
    meta = bank_of([], "fp16", device=torch.device("meta"))
    meta.names, meta.offsets = list(a16.names), list(a16.offsets)
    with pytest.raises(ValueError, match="device"):
        S.search(a16, t, ensemble=meta)
    renamed = bank_of([b16.scene(i).float() for i in range(3)], "fp16", names=["s0", "other", "s2"])
    with pytest.raises(ValueError, match="names.*'s1' and 'other'"):
        S.search(a16, t, ensemble=renamed)
    fewer = bank_of([b16.scene(0).float()], "fp16")
    with pytest.raises(ValueError, match="names"):
        S.search(a16, t, ensemble=fewer)
    cut = bank_of([unit(3, 16, g), unit(1, 16, g), unit(49, 16, g)], "fp16")
    with pytest.raises(ValueError, match="offsets"):
        S.search(a16, t, ensemble=cut)
    for bad in ("Vocabulary", "element", None, 0):
        with pytest.raises(ValueError, match="ensemble_mode"):
            S.search(a16, t, ensemble=b16, ensemble_mode=bad)
    S.search(a16, t, ensemble_mode="nonsense")                  # (without a second bank the word is not looked at)
    # the kind is named before the dim, the dim before the names
    with pytest.raises(ValueError, match="kind"):
        S.search(a16, t, ensemble=bank_of([unit(2, 32, g)], "fp8", 32))
    with pytest.raises(ValueError, match="dim"):
        S.search(a16, t, ensemble=bank_of([unit(2, 32, g)], "fp16", 32))


def test_select_checks_its_arguments():
    g = torch.Generator().manual_seed(1)
    a16, b16 = two_banks(g, "fp16")
    a8, _ = two_banks(g, "fp8")
    src = torch.zeros(53, dtype=torch.bool)
    with pytest.raises(TypeError, match="FeatureBank"):
        a16.select(b16.features, src)
    with pytest.raises(ValueError, match="kind"):
        a16.select(a8, src)
    for bad in (src[:52], src[:, None].expand(53, 2), src.to(torch.uint8), src.float(), src.tolist(), None):
        with pytest.raises(ValueError, match="source"):
            a16.select(b16, bad)


def test_heat_map_checks_the_second_feature_matrix():
    g = torch.Generator().manual_seed(2)
    x, y, t = unit(5, 16, g), unit(5, 16, g), unit(2, 16, g).half()
    with pytest.raises(ValueError, match="ensemble"):
        S.heat_map(x, t, ensemble=y[:4])
    with pytest.raises(ValueError, match="ensemble"):
        S.heat_map(x, t, ensemble=unit(5, 32, g))
    with pytest.raises(ValueError, match="ensemble"):
        S.heat_map(x, t, ensemble=y.to("meta"))
    with pytest.raises(TypeError, match="ensemble"):
        S.heat_map(x, t, ensemble=y[0])
    with pytest.raises(TypeError, match="ensemble"):
        S.heat_map(x, t, ensemble=[1.0])
    with pytest.raises(ValueError, match="ensemble_mode"):
        S.heat_map(x, t, ensemble=y, ensemble_mode="both")


# --------------------------------------------------------------------------------------- results, dispatch, values
PLAIN = ["err", "k", "max_scene_rows", "normalize", "thresholds", "want_heat"]


@pytest.mark.parametrize("kind", ["fp16", "fp8"])
def test_result_fields_dispatch_and_values(cpu_kernels, kind):
    g = torch.Generator().manual_seed(3)
    a, b = two_banks(g, kind)
    t, neg = unit(6, 16, g).half(), unit(4, 16, g).half()
    old, new = ("search", "ensemble") if kind == "fp16" else ("search_fp8", "ensemble_fp8")
    n_bank = 1 if kind == "fp16" else 2
    # a search without a second bank calls the old op with the old arguments, and only that
    del cpu_kernels[:]
    plain = S.search(a, t, k=8, thresholds=0.1, return_heat=True)
    contrast = S.search(a, t, k=8, thresholds=0.5, return_heat=True, negatives=neg, ensemble=None, ensemble_mode="query")
    assert cpu_kernels == [(old, n_bank + 2, PLAIN), (old, n_bank + 2, sorted(PLAIN + ["negatives", "temperature"]))]
    for r in (plain, contrast):
        assert r.source is None and r.ensemble_mode is None
    for mode in er.MODES:
        for negatives in (None, neg):
            for normalize in (True, False):
                del cpu_kernels[:]
                res = S.search(a, t, k=8, thresholds=0.2, normalize=normalize, return_heat=True, negatives=negatives, ensemble=b,
                               ensemble_mode=mode)
                extra = ["mode", "want_source"] + (["negatives", "temperature"] if negatives is not None else [])
                assert cpu_kernels[0] == (new, 2 * n_bank + 2, sorted(PLAIN + extra))
                assert res.ensemble_mode == mode and res.relevancy is (negatives is not None)
                assert res.source.dtype == torch.bool and res.source.shape == ((53,) if mode == "vocabulary" else (53, 6))
                heat, source = er.compose(S.search, a, b, t, mode, normalize, negatives)
                assert sr.same_bits(res.heat, heat) and torch.equal(res.source, source)
                assert 0.2 < source.double().mean().item() < 0.8
                sr.check_selection(res, res.heat, a.offsets, 8, torch.full((6,), 0.2))
                assert res.heat.shape == (53, 6) and res.topk_scores.shape == (3, 6, 8) and res.counts.shape == (3, 6)
                assert res.rank_scenes(0)[0][0] in a.names and res.scene_heat("s2").shape == (50, 6)
                no_heat = S.search(a, t, k=8, negatives=negatives, normalize=normalize, ensemble=b, ensemble_mode=mode)
                assert no_heat.heat is None and (no_heat.source is None) == (mode == "query")
                assert torch.equal(no_heat.topk_points, res.topk_points)
    # the bank with itself: the plain search, nothing from the second source
    same = S.search(a, t, k=8, thresholds=0.1, return_heat=True, ensemble=a)
    assert sr.same_bits(same.heat, plain.heat) and not same.source.any() and torch.equal(same.topk_points, plain.topk_points)


@pytest.mark.parametrize("kind", ["fp16", "fp8"])
def test_select_is_the_stored_ensemble(kind):
    g = torch.Generator().manual_seed(4)
    a, b = two_banks(g, kind)
    t, neg = unit(6, 16, g).half(), unit(4, 16, g).half()
    for negatives in (None, neg):
        res = S.search(a, t, k=8, return_heat=True, negatives=negatives, ensemble=b)
        picked = a.select(b, res.source)
        assert picked is not a and picked.dtype == kind and picked.names == a.names and picked.offsets == a.offsets and picked.rows == 53
        for mine, theirs, got in zip(a._store, b._store, picked._store):
            assert torch.equal(got[:53][res.source], theirs[:53][res.source])
            assert torch.equal(got[:53][~res.source], mine[:53][~res.source])
        again = S.search(picked, t, k=8, return_heat=True, negatives=negatives)
        assert sr.same_bits(again.heat, res.heat) and torch.equal(again.topk_points, res.topk_points)
    assert torch.equal(a.select(b, torch.zeros(53, dtype=torch.bool))._store[0][:53], a._store[0][:53])
    assert torch.equal(a.select(b, torch.ones(53, dtype=torch.bool))._store[-1][:53], b._store[-1][:53])


def test_heat_map_sends_both_matrices_through_inds_reverse():
    g = torch.Generator().manual_seed(5)
    x, y, t, neg = unit(5, 16, g), unit(5, 16, g), unit(3, 16, g).half(), unit(2, 16, g).half()
    y[0] = 0
    inv = torch.tensor([1, 1, 4, 0, 3])
    for mode in er.MODES:
        for negatives in (None, neg):
            hm = S.heat_map(x, t, inv, negatives=negatives, temperature=0.2, ensemble=y, ensemble_mode=mode)
            want, _ = er.compose(S.search, bank_of([x[inv]], "fp16"), bank_of([y[inv]], "fp16"), t, mode, True, negatives, 0.2)
            assert hm.shape == (5, 3) and sr.same_bits(hm, want) and sr.same_bits(hm[0], hm[1])
    assert sr.same_bits(S.heat_map(x, t, inv), S.heat_map(x, t, inv, ensemble=None))


def test_the_reference_pick():
    nan, inf = float("nan"), float("inf")
    h = lambda rows: torch.tensor(rows, dtype=torch.float16)
    a = h([[0.5, 0.1], [0.5, 0.1], [0.0, -1.0], [nan, 0.9], [0.2, 0.1], [-inf, -inf], [0.3, 0.3]])
    b = h([[0.4, 0.6], [0.5, 0.2], [-0.0, -2.0], [1.0, 1.0], [nan, 0.9], [-inf, 0.0], [0.3, 0.3]])
    heat, source = er.pick("vocabulary", a, b, a, b)
    assert source.tolist() == [True, False, False, False, False, True, False]
    assert sr.same_bits(heat, torch.where(source[:, None], b, a))
    heat, source = er.pick("query", a, b, a, b)
    assert source.tolist() == [[False, True], [False, True], [False, False], [False, True], [False, True], [False, True], [False, False]]
    assert sr.same_bits(heat[2], a[2]) and torch.isnan(heat[3, 0]) and sr.same_bits(heat[4, :1], a[4, :1])      # +0 kept over -0; NaN: A


# ------------------------------------------------------------------------------- the float64 contract of the pick
@pytest.mark.parametrize("kind", ["fp16", "fp8"])
def test_the_score_intervals_decide_all_but_a_per_cent_of_the_picks(kind):
    """the undecided share test_gpu_search_ensemble.py allows for, on its inputs (seed 7, every seventh row of B zero)"""
    for d, q in ((64, 1), (64, 5), (64, 20), (272, 33), (272, 130), (768, 65)):
        gen = torch.Generator().manual_seed(7)
        a, b = sr.unit_rows(1000, d, gen), sr.unit_rows(1000, d, gen)
        b[::7] = 0
        t = sr.text(130, d, gen)[:q].double().numpy()
        va, vb = er.stored_values(a, kind), er.stored_values(b, kind)
        for mode in er.MODES:
            for normalize in ((True,) if mode == "vocabulary" else (True, False)):
                ref_a, ref_b = sb.interval(va, t, normalize), sb.interval(vb, t, normalize)
                share = er.undecided_share(mode, ref_a, ref_b)
                must_b, must_a = er.decided(mode, ref_a, ref_b)
                print("%s %s normalize=%d d=%d q=%d: %.3f %% undecided, %.1f %% B" % (kind, mode, normalize, d, q, 100 * share, 100 * must_b.mean()))
                assert share <= 0.01 and not (must_a & must_b).any()
                assert 0.25 <= must_b.mean() <= 0.75


# ---- the C entries' argument checks (no kernel is launched: every call returns before it touches the device)
@pytest.mark.parametrize("fp8", [False, True])
def test_ensemble_entries_argument_errors(fp8):
    import __graft_entry__ as ge
    ge.build()
    h = _lib.load()
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    need = h.osn_bank_search_ws_bytes(8, 1, 2, 4, 8)         # the plain search's workspace suffices
    name = ENTRIES[1] if fp8 else ENTRIES[0]

    def call(rows=p, other=p + 128, n=8, d=16, off=p + 512, s=1, max_rows=8, t=p + 1024, q=2, normalize=1, k=4, thr=None, heat=None,
             ts=p + 2048, tp=p + 3072, counts=None, e=p + 4000, ws=p + 4096, ws_bytes=need, neg=p + 1536, m=3, tau=0.1, mode=0,
             source=p + 6000, other_exps=p + 384):
        head = (rows, p + 256, other, other_exps) if fp8 else (rows, other)
        return getattr(h, name)(*head, n, d, off, s, max_rows, t, q, normalize, k, thr, heat, ts, tp, counts, e, ws, ws_bytes, None,
                                neg, m, tau, mode, source)
    bad_calls = [dict(mode=2), dict(mode=-1), dict(other=None), dict(other=p + 132), dict(source=None), dict(m=0), dict(m=-1),
                 dict(m=1025), dict(neg=None), dict(neg=p + 1540), dict(neg=None, m=0, tau=0.1, mode=3), dict(tau=0.0),
                 dict(tau=float("nan")), dict(tau=float("inf")), dict(d=24 if fp8 else 12), dict(q=0), dict(q=1025), dict(k=129),
                 dict(t=None), dict(rows=None), dict(normalize=2)]
    if fp8:
        bad_calls.append(dict(other_exps=None))
    for bad in bad_calls:
        assert call(**bad) == -1, bad                         # OSN_E_ARG
        assert name + ":" in _lib.last_error(), bad
    for rc in (call(ws_bytes=need - 1), call(ws_bytes=need - 1, neg=None, m=0, mode=1, source=None)):
        assert rc not in (0, -1) and "workspace" in _lib.last_error()      # (every argument passed: only the workspace is short)
