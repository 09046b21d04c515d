"""The pieces heat_kernel and heat_fp8_kernel share (csrc/search.hip: query staging, MFMA loop, row norms, score output),
driven through both kernels at the chunk and tile edges the other search tests leave out.

    d   fp16 bank   8 (one partial 128-wide chunk), 136 (a whole one and a partial), 384 (three whole)
        fp8 bank    128 (one chunk: the two-stage loop leaves at its first half), 272 (three, the last partial), 384 (three
                    whole), 512 (four whole: leaves at the loop's end, the last stash skipped)
    n   1 (one row), 129 (one row in a second workgroup, the ragged column store), 300 (several workgroups, n % 8 != 0)
    q   1 and 32 (the one-tile instance and its full tile), 33 (two tiles, one column in the second), 65 (two column groups)

Oracle and bound: the float64 formulas of tests/search_reference.py and tests/search_fp8_reference.py on the stored rows, abs <=
2e-3 as in test_gpu_search.py / test_gpu_search_fp8.py (derived there for any d; a smaller d only has less rounding).  That 2e-3
is the distance to the REFERENCE's expression, which rounds the normalised vector to fp16 first; this file is about the edges
of chunks and tiles.  The kernel's own arithmetic is held in tests/test_gpu_search_bounds.py, per element.  The
selection is checked against the kernel's own heat-map, so pass 2 is seen reading what the shared store wrote."""
import pytest
import torch

import search_fp8_reference as f8
import search_reference as sr

pytestmark = pytest.mark.gpu

TOL = 2e-3
NS = (1, 129, 300)
QS = (1, 32, 33, 65)
K = 4


def dev():
    return torch.device("cuda", 0)


def rows_with_edges(n, d, gen):
    """-> (float32 rows, the all-zero rows, the NaN-holding rows); a single row stays an ordinary one"""
    x = sr.unit_rows(n, d, gen)
    zero = [r for r in (2, 299) if r < n and n > 1]
    nan = [r for r in (5, 200) if r < n]
    if zero:
        x[zero] = 0
    for r in nan:
        x[r, r % d] = float("nan")
    return x, zero, nan


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("kind,d", [("fp16", 8), ("fp16", 136), ("fp16", 384), ("fp8", 128), ("fp8", 272), ("fp8", 384), ("fp8", 512)])
def test_heat_and_selection_at_the_chunk_and_tile_edges(kind, d, normalize):
    from openscene_amd.search import FeatureBank, search
    g = torch.Generator().manual_seed(100 * d + 10 * int(normalize) + (kind == "fp8"))
    done = 0
    for n in NS:
        x, zero, nan = rows_with_edges(n, d, g)
        if kind == "fp16":
            x = x.half()
        ok = torch.ones(n, dtype=torch.bool)
        ok[nan] = False
        bank = FeatureBank(d, dev(), capacity_rows=8, dtype=kind)
        cut = n // 2                                          # two scenes (an empty first one when n = 1)
        bank.add_scene("a", x[:cut].to(dev()))
        bank.add_scene("b", x[cut:].to(dev()))
        assert bank.offsets == [0, cut, n]
        for q in QS:
            t = sr.text(q, d, g)
            thr = torch.zeros(q)
            res = search(bank, t.to(dev()), k=K, thresholds=thr, normalize=normalize, return_heat=True)
            heat = res.heat.cpu()
            assert heat.shape == (n, q) and heat.dtype == torch.float16
            assert torch.isnan(heat[nan]).all() and not torch.isnan(heat[ok]).any()
            assert (heat[zero] == 0).all()                    # exactly zero: 0 / (0 + 1e-5)
            if kind == "fp16":
                refs = [sr.scores_f64(x, t, normalize, round_normalised=r) for r in (False, True)]
            else:
                refs = [f8.scores_f64(bank.codes.cpu(), bank.exponents.cpu(), t, normalize)]
            worst = max((heat.double() - ref)[ok].abs().max().item() for ref in refs)
            print("%s heat-map normalize=%d d=%d n=%d q=%d: max abs deviation %.3e" % (kind, normalize, d, n, q, worst))
            assert worst <= TOL, (n, q)
            sr.check_selection(res, res.heat, bank.offsets, K, thr.to(dev()))
            done += 1
    assert done == len(NS) * len(QS)
