"""Host logic of the search with negative queries WITHOUT a GPU: ops.bank_search / ops.bank_search_fp8 are replaced by the
torch stand-ins of tests/search_contrast_reference.py (the plain stand-ins behind the formula); the argument checks of
openscene_amd.search, SearchResult's new fields and the C entries' own checks are the code under test."""
import ctypes

import pytest
import torch

import search_contrast_reference as cr
import search_fp8_reference as f8
import search_reference as sr
from openscene_amd import ops
from openscene_amd import search as S

CPU = torch.device("cpu")


@pytest.fixture(autouse=True)
def cpu_kernels(monkeypatch):
    calls = []

    def spy(name, f):
        def g(*a, **kw):
            calls.append((name, sorted(kw)))
            return f(*a, **kw)
        return g
    monkeypatch.setattr(ops, "bank_append", sr.bank_append)
    monkeypatch.setattr(ops, "bank_check", sr.bank_check)
    monkeypatch.setattr(ops, "bank_search", spy("search", cr.bank_search))
    monkeypatch.setattr(ops, "bank_append_fp8", f8.bank_append_fp8)
    monkeypatch.setattr(ops, "bank_search_fp8", spy("search_fp8", cr.bank_search_fp8))
    return calls


def unit(n, d, gen):
    return torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=1)


def banks(gen, d=16):
    rows = [unit(3, d, gen), torch.zeros(0, d), unit(50, d, gen)]
    out = []
    for kind in ("fp16", "fp8"):
        bank = S.FeatureBank(d, CPU, dtype=kind)
        for i, r in enumerate(rows):
            bank.add_scene("s%d" % i, r)
        out.append(bank)
    return out


def test_argument_errors_of_the_negatives_and_the_temperature():
    g = torch.Generator().manual_seed(0)
    bank = banks(g)[0]
    t, neg = unit(3, 16, g).half(), unit(2, 16, g).half()
    with pytest.raises(TypeError, match="negatives"):
        S.search(bank, t, negatives=neg.float())
    with pytest.raises(TypeError, match="negatives"):
        S.search(bank, t, negatives=neg.numpy())
    with pytest.raises(ValueError, match="negatives"):
        S.search(bank, t, negatives=neg[:, :8])
    with pytest.raises(ValueError, match="negatives"):
        S.search(bank, t, negatives=neg[0])
    with pytest.raises(ValueError, match="negatives"):
        S.search(bank, t, negatives=neg[:0])
    for bad in (0.0, -0.1, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="temperature"):
            S.search(bank, t, negatives=neg, temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            S.heat_map(unit(4, 16, g), t, negatives=neg, temperature=bad)


def test_result_fields_dispatch_and_values(cpu_kernels):
    g = torch.Generator().manual_seed(1)
    t, neg = unit(2, 16, g).half(), unit(4, 16, g).half()
    for bank, name in zip(banks(g), ("search", "search_fp8")):
        del cpu_kernels[:]
        plain = S.search(bank, t, k=8, thresholds=0.1, return_heat=True)
        assert cpu_kernels == [(name, ["err", "k", "max_scene_rows", "normalize", "thresholds", "want_heat"])]   # the plain arguments
        assert plain.relevancy is False and plain.temperature is None
        res = S.search(bank, t, k=8, thresholds=0.5, return_heat=True, negatives=neg)
        assert cpu_kernels[-1] == (name, ["err", "k", "max_scene_rows", "negatives", "normalize", "temperature", "thresholds", "want_heat"])
        assert res.relevancy is True and res.temperature == 0.1
        assert S.search(bank, t, negatives=neg, temperature=0.05).temperature == 0.05
        assert res.heat.shape == (53, 2) and res.topk_scores.shape == (3, 2, 8) and res.counts.shape == (3, 2)
        both = S.search(bank, torch.cat([t, neg]), k=1, return_heat=True).heat
        want = cr.relevancy_f64(both[:, :2], both[:, 2:], 0.1)
        assert sr.same_bits(res.heat, want)
        f = want.float()
        assert ((f >= 0) & (f <= 1)).all()
        sr.check_selection(res, res.heat, bank.offsets, 8, torch.full((2,), 0.5))
        assert res.rank_scenes(0, by="count") == sorted(zip(bank.names, res.counts[:, 0].tolist()), key=lambda p: -p[1])
        assert res.scene_heat("s2").shape == (50, 2)
        # a query among the negatives can reach one half at the most, and the queries as their own negatives reach it
        assert (S.search(bank, t, return_heat=True, negatives=torch.cat([neg, t])).heat.float() <= 0.5).all()
        assert (S.search(bank, t, return_heat=True, negatives=t).heat.float().max(dim=1)[0] == 0.5).all()


def test_heat_map_passes_the_negatives_on():
    g = torch.Generator().manual_seed(2)
    x, t, neg = unit(5, 16, g), unit(2, 16, g).half(), unit(3, 16, g).half()
    inv = torch.tensor([1, 1, 4, 0])
    hm = S.heat_map(x, t, inv, negatives=neg, temperature=0.2)
    both = S.heat_map(x, torch.cat([t, neg]), inv)
    assert hm.shape == (4, 2) and sr.same_bits(hm, cr.relevancy_f64(both[:, :2], both[:, 2:], 0.2))
    assert sr.same_bits(S.heat_map(x, t, inv), both[:, :2].contiguous())


def test_reference_helpers():
    nan, inf = float("nan"), float("inf")
    s = torch.tensor([[0.25], [0.25], [nan], [inf], [0.0]], dtype=torch.float16)
    g = torch.tensor([[0.25, -1.0], [nan, 0.0], [0.0, 0.0], [inf, 0.0], [-0.0, -1.0]], dtype=torch.float16)
    rel = cr.relevancy_f64(s, g, 0.1)
    assert rel[0].item() == 0.5 and rel[4].item() == 0.5 and torch.isnan(rel[1:4]).all()
    a = torch.tensor([0.5, 1.0, 0.0, nan, nan, 1.0], dtype=torch.float16)
    b = torch.tensor([0.5, 1.0 - 2.0 ** -11, -0.0, nan, 1.0, 1.0 + 2.0 ** -10], dtype=torch.float16)
    assert cr.ulp_distance(a, b).tolist() == [0, 1, 0, 0, -1, 1]


# ---- the C entries' argument checks (no kernel is launched: every call returns before it touches the device)
@pytest.mark.parametrize("fp8", [False, True])
def test_contrast_entries_argument_errors(fp8):
    import __graft_entry__ as ge
    ge.build()
    from openscene_amd import _lib
    h = _lib.load()
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    need = h.osn_bank_search_ws_bytes(8, 1, 2, 4, 8)         # sized by q alone
    name = "osn_bank_search_contrast" + ("_fp8" if fp8 else "")

    def call(rows=p, n=8, d=16, off=p + 512, s=1, max_rows=8, t=p + 1024, q=2, normalize=1, k=4, thr=None, heat=None, ts=p + 2048,
             tp=p + 3072, counts=None, e=p + 4000, ws=p + 4096, ws_bytes=need, neg=p + 1536, m=3, tau=0.1):
        head = (rows, p + 256) if fp8 else (rows,)
        return getattr(h, name)(*head, n, d, off, s, max_rows, t, q, normalize, k, thr, heat, ts, tp, counts, e, ws, ws_bytes, None,
                                neg, m, tau)
    for bad in (dict(m=0), dict(m=-1), dict(m=1025), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")),
                dict(neg=None), dict(neg=p + 1540), dict(d=24 if fp8 else 12), dict(q=0), dict(k=129), dict(t=None), dict(rows=None)):
        assert call(**bad) == -1, bad                         # OSN_E_ARG
        assert name in _lib.last_error()
    rc = call(ws_bytes=need - 1)
    assert rc not in (0, -1) and "workspace" in _lib.last_error()
    assert h.osn_version() == 3
