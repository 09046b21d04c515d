"""The two halves of the pair-array weight gradient as every executor backward runs them -- osn_spconv_wgrad_tl_partial per
convolution, then osn_wgrad_tl_reduce_batch over all of them -- against the single entry osn_spconv_wgrad_tl, whose summation order
the header promises: bit for bit the same gradient.

conv_bounds.batch_plan(): the pair-array weight-gradient cases of conv_bounds.CASES in turn (32 -> 32 up to 384 -> 256 channels, K = 27, 8
and identity maps, swap launches) with the five operand kinds in turn, NaN-padded operands -- 33 live jobs in ONE call.  A launch takes 32
jobs, so the second launch and a ragged last batch (one job) are reached; that last job is a map with rows on both sides and not one
pair, whose gradient is exactly zero.  A 34th entry has no rows: its job is skipped and gW is zeroed by the first call.  Every gW is
pre-filled with NaN, so an element the reduction does not write shows.  The single-entry results are the ones test_gpu_conv_bounds.py
holds to the per-element abs-sum bound.
"""
import pytest
import torch

import conv_bounds as cb
from test_gpu_conv_bounds import dev, launch_of, padded

pytestmark = pytest.mark.gpu


def _launch_of(case):
    if case in cb.CASES:
        return launch_of(case)                       # the launches of test_gpu_conv_bounds.py, tile lists and pair arrays built once
    rc, nbr = cb.resolve(case)
    return rc, nbr, cb.Launch(rc, nbr, dev())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_batched_reduction_gives_the_bits_of_the_single_entry():
    d = dev()
    plan = cb.batch_plan()
    assert len(plan) == cb.BATCH_JOBS + 1 and cb.BATCH_JOBS > 32
    assert len({(c.cin, c.cout, c.K) for c, _k in plan}) >= 12
    entries = cb.batch_entries(_launch_of, lambda t: padded(t, d))
    got, jobs = cb.batched_wgrad(entries, d)
    torch.cuda.synchronize(d)
    live = [i for i in range(len(entries)) if jobs[i].gW]
    assert live == list(range(cb.BATCH_JOBS)), "every entry with rows is a pending job, the one without rows is not"
    for i, ((case, kind), (run, feats, gout)) in enumerate(zip(plan, entries)):
        label = "job %d %s %s" % (i, case.id, kind)
        if feats.shape[0] == 0:
            assert got[i].shape == (case.K, case.cin, case.cout) and float(got[i].abs().max()) == 0.0, label + ": not zeroed"
            continue
        want = run.wgrad(feats, gout)
        assert bool(torch.isfinite(got[i]).all()), label + ": elements the batched reduction did not write"
        assert _same_bits(got[i], want), "%s: %d elements differ from osn_spconv_wgrad_tl" % (label, int((got[i] != want).sum()))
        if case.id == cb.EMPTY_MAP.id:
            assert float(want.abs().max()) == 0.0, label + ": a map without pairs has a zero gradient"
    # again: the jobs' partial buffers and pair arrays are left as they were, so the same call gives the same bits
    again, _ = cb.batched_wgrad(entries, d)
    assert all(_same_bits(a, b) for a, b in zip(got, again)), "not bitwise reproducible"
