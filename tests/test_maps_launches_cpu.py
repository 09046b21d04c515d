"""The launch sequence of osn_maps_build without a GPU (null HIP runtime of tools/dryrun: every launch becomes a log line).
MinkUNet's job list on the S100k level sizes:
  * the 3^3 map of a level that follows the level's 5^3 map is one copy launch (kmap_derive_self_kernel) on the 5^3 job's stream
    instead of a probing build;
  * a level with an occupancy buffer gets one occ_fill_kernel launch in front of its self map, which runs the occupancy builder;
  * a pair list is two launches (prefix, fill): no pair_plan launch of its own and no memset;
  * ops.maps_set_legacy(1): the sequence of the earlier rounds -- six probing self-map builds, pair_plan in front of every fill."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [100999, 47618, 12868, 3052, 700]            # S100k
MAIN, SIDE, AUX = 0x100, 0x200, 0x300               # stream handles (never dereferenced by the null runtime)


@pytest.fixture(scope="module")
def dry():
    sys.path.insert(0, os.path.join(ROOT, "tools", "dryrun"))
    import dry_step
    from openscene_amd import _lib
    lib = ctypes.CDLL(dry_step.build_dry_lib())
    for name, (res, args) in _lib.PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    lib.osn_dry_log.restype = ctypes.c_char_p
    return lib, dry_step


def _jobs(lib, n_occ):
    """MinkUNet's maps as CoordinateManager._prebuild_fast lays them out (pairs=True), over made-up device addresses -- without the
    tile-ordered copies: the sort asks the device for its scratch size."""
    from openscene_amd import ops
    ldt, jdt = ops._map_dtypes()
    cursor = [1 << 32]

    def take(nbytes=1 << 26):
        cursor[0] += nbytes
        return cursor[0]
    levels = np.zeros(len(ROWS), dtype=ldt)
    for i, r in enumerate(ROWS):
        levels[i] = (take(), take(), take(), 1 << 18, r)
    lane = {(0, 0, 5): 1, (0, 0, 3): 2, (2, 2, 3): 2, (0, 1, 2): 2}
    specs = [(0, 0, 5)] + [(l, l, 3) for l in range(5)] + [(l, l + 1, 2) for l in range(4)]
    jobs = np.zeros(len(specs), dtype=jdt)
    n_pl = 0
    for j, (li, lo, k) in enumerate(specs):
        q = dict(lvl_in=li, lvl_out=lo, ksize=k, scale=1 << li, self_map=int(li == lo), stream=lane.get((li, lo, k), 0),
                 nbr_fwd=take(), counts=take())
        if li != lo:
            q["nbr_bwd"] = take()
        if k ** 3 <= 32:
            q["bm_fwd"], q["tl_fwd"], q["pl_fwd"] = lib.osn_tile_rows(ROWS[lo]), take(), take()
            n_pl += 1
            if li != lo:
                q["bm_bwd"], q["tl_bwd"] = lib.osn_tile_rows(ROWS[li]), take()
        jobs[j] = tuple(q.get(n, 0) for n in jdt.names)
    occ = (ctypes.c_void_p * len(ROWS))(*[take() if i < n_occ else None for i in range(len(ROWS))])
    return levels, jobs, occ, n_pl


def _log(dry, legacy, n_occ=2, streams=(MAIN, SIDE, AUX)):
    lib, dry_step = dry
    levels, jobs, occ, n_pl = _jobs(lib, n_occ)
    ns = len(streams)
    st = (ctypes.c_void_p * ns)(*streams)
    ws = (ctypes.c_void_p * ns)(*[(7 + i) << 40 for i in range(ns)])
    wb = (ctypes.c_uint64 * ns)(*[256] * ns)
    ev = lib.osn_events_create(8)
    prev = lib.osn_maps_set_legacy(int(legacy))
    try:
        lib.osn_dry_reset()
        rc = lib.osn_maps_build_occ(levels.ctypes.data, len(levels), jobs.ctypes.data, len(jobs), st, ws, wb, ns, ev, occ)
        log = dry_step.demangle(lib.osn_dry_log().decode())
    finally:
        lib.osn_maps_set_legacy(prev)
        lib.osn_events_destroy(ev)
    assert rc == 0, lib.osn_last_error().decode()
    lines = log.split("\n")
    launches = []                                   # (kernel, grid, stream) in issue order
    for i, l in enumerate(lines):
        m = re.match(r"K (\S+?)(?:<.*>)? grid=(\S+) block=\d+", l)
        if m:
            launches.append((m.group(1), m.group(2), int(lines[i + 1][2:], 16)))
    return launches, [l for l in lines if l.startswith("MEMSET")], n_pl


def _count(launches, kernel):
    return sum(1 for k, _, _ in launches if k == kernel)


def test_derived_table_occupancy_and_pair_plan(dry):
    new, memsets, n_pl = _log(dry, legacy=False)
    old, old_memsets, _ = _log(dry, legacy=True)
    assert n_pl == 9 and not memsets and not old_memsets
    # the earlier sequence: a probing build per self map, a plan launch per pair list, nothing of the new kernels
    assert _count(old, "kmap_build_self_kernel") == 6
    assert _count(old, "pair_plan_kernel") == _count(old, "pair_fill_kernel") == _count(old, "pair_prefix_kernel") == n_pl
    assert not [k for k, _, _ in old if k in ("kmap_derive_self_kernel", "occ_fill_kernel", "kmap_build_self_occ_kernel")]
    # now: level 0's 3^3 map is a copy of its 5^3 map -- one probing build fewer -- and levels 0, 1 probe occupied cells only
    assert _count(new, "kmap_derive_self_kernel") == 1
    assert _count(new, "kmap_build_self_kernel") + _count(new, "kmap_build_self_occ_kernel") == 5
    assert _count(new, "occ_fill_kernel") == _count(new, "kmap_build_self_occ_kernel") == 2
    assert _count(new, "pair_plan_kernel") == 0 and _count(new, "pair_fill_kernel") == _count(new, "pair_prefix_kernel") == n_pl
    assert len(new) == len(old) - n_pl + 2                             # - 9 plans, + 2 occupancy tables; the copy replaces a build
    # everything else is the same launch, in the same order
    changed = ("kmap_build_self_kernel", "kmap_build_self_occ_kernel", "kmap_derive_self_kernel", "occ_fill_kernel", "pair_plan_kernel",
               "fill_batch_kernel")
    assert [(k, g) for k, g, _ in new if k not in changed] == [(k, g) for k, g, _ in old if k not in changed]
    # the copy runs on the 5^3 job's stream, right behind it, with the occupancy table in front
    names = [k for k, _, s in new if s == SIDE]
    assert names[:3] == ["occ_fill_kernel", "kmap_build_self_occ_kernel", "kmap_derive_self_kernel"]
    grid = dict((k, g) for k, g, _ in new)
    assert grid["kmap_derive_self_kernel"] == "%d,27,1" % ((ROWS[0] + 255) // 256)
    assert [g for k, g, _ in new if k == "kmap_build_self_occ_kernel"] == ["%d,3,1" % ((ROWS[0] + 255) // 256), "%d,2,1" % ((ROWS[1] + 255) // 256)]


def test_without_occupancy_buffers_and_on_one_stream(dry):
    new, memsets, n_pl = _log(dry, legacy=False, n_occ=0, streams=(MAIN,))
    old, _, _ = _log(dry, legacy=True, n_occ=0, streams=(MAIN,))
    assert not memsets
    assert _count(new, "occ_fill_kernel") == _count(new, "kmap_build_self_occ_kernel") == 0
    assert _count(new, "kmap_build_self_kernel") == 5 and _count(new, "kmap_derive_self_kernel") == 1
    assert len(new) == len(old) - n_pl
    assert {s for _, _, s in new} == {MAIN}
