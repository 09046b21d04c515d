"""The launch plan of the batch-norm apply kernels (csrc/bn.hip, plan_apply; osn_bn_apply_plan in include/openscene_amd.h), asked of
the real host code through the dry-run library (tools/dryrun: a null HIP runtime, no GPU).

The column-keeping kernels are only right on a grid whose stride (grid x 256 quads) is a multiple of c4: a thread's quads then all
lie in the column quad it took its constants for.  The plan is the smallest such grid at or above the grid the flat kernels use,
min(2048, ceil(total4 / 256)), and at most 127 workgroups above it; where none exists it says `flat` and keeps that grid.  Here the
answer is compared with a search over the candidates, for c4 = 1 .. 1024 and totals from one quad to past the 2048-workgroup cap.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BLOCK, MAX_GRID, SLACK = 256, 2048, 127
ROWS = (1, 2, 15, 17, 63, 208, 1000, 4097, 33000, 70001, 100999, 3000000)


def _wanted(total4):
    return max(1, min(MAX_GRID, -(-total4 // BLOCK)))


@pytest.fixture(scope="module")
def plan():
    sys.path.insert(0, os.path.join(ROOT, "tools", "dryrun"))
    import dry_step
    mp = pytest.MonkeyPatch()
    dry_step.install(dry_step.build_dry_lib(), mp.setattr)
    from openscene_amd import ops
    yield ops.bn_apply_plan
    mp.undo()


def test_the_plan_keeps_columns_exactly_where_a_grid_under_the_cap_fits(plan):
    kept = flat = 0
    for c4 in range(1, 1025):
        for n in ROWS:
            total4 = n * c4
            g = _wanted(total4)
            grid, is_flat = plan(total4, c4)
            label = "c4 %d, %d rows (wanted grid %d): plan (%d, flat %d)" % (c4, n, g, grid, is_flat)
            fits = [k for k in range(g, g + SLACK + 1) if (k * BLOCK) % c4 == 0]
            assert 1 <= grid <= g + SLACK <= MAX_GRID + SLACK, label
            assert is_flat == (not fits), label
            if is_flat:
                assert grid == g, label                  # the flat kernels' own grid
                flat += 1
            else:
                assert (grid * BLOCK) % c4 == 0 and grid == fits[0], label
                kept += 1
    assert kept > 0 and flat > 0


def test_the_plan_of_the_network_widths_and_of_the_gpu_tests_widths(plan):
    # every width of the U-Nets (c4 = 8 .. 64, and 24, 48: period 3) keeps its columns at every size
    for c in (32, 64, 96, 128, 192, 256, 384):
        for n in ROWS:
            grid, is_flat = plan(n * (c // 4), c // 4)
            assert not is_flat and (grid * BLOCK) % (c // 4) == 0 and grid - _wanted(n * (c // 4)) < 3
    # c = 260 (c4 = 65: a grid every 65) always fits; c = 772 (c4 = 193) fits only where the wanted grid lies within 127 of a multiple
    assert not any(plan(n * 65, 65)[1] for n in ROWS)
    assert [n for n in (1, 15, 16, 17, 207, 208, 209, 4097, 70001) if plan(n * 193, 193)[1]] == [1, 15, 16, 17]
    assert plan(70001 * 193, 193) == (2123, False)


def test_the_plan_rejects_what_is_not_a_shape(plan):
    from openscene_amd._lib import OpenSceneAmdError
    for total4, c4 in ((-1, 4), (10, 0), (10, -3)):
        with pytest.raises(OpenSceneAmdError):
            plan(total4, c4)
