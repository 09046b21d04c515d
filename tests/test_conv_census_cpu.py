"""A convolution kernel instance that a shipped network can launch has a case in conv_bounds.CASES -- checked without a GPU.

The per-element abs-sum bound (conv_bounds, test_gpu_conv_bounds.py, test_gpu_conv_pieces.py) is asked of CASES.  Every family is a grid
of compile-time instances, and which one runs is decided by host code from the channel counts, the row counts and the tile height; so a
case list chosen by family can miss every instance the networks use.  Here both sides are listed with the library linked against the
null HIP runtime of tools/dryrun (conv_census.py: keys, normalisation):

  * network side: every variant of mink_unet._ARCHS on the ROOMS below -- one training step and the evaluation forward in the three
    precisions, through the module path and through the executor.  The rooms' level rows lie on both sides of every row count that
    selects a kernel or a tile height (ROW_THRESHOLDS; asserted), the largest ones have the benchmark's level-0 sizes (above 100 000
    and above 200 000 rows);
  * case side: every entry of CASES through the Launch / PiecesLaunch object the GPU tests run, and the batched weight-gradient
    reduction through the helper test_gpu_wgrad_batch.py calls.

Every network-side key must be on the case side or in EXEMPT; an EXEMPT entry that no network launches any more fails as well.
The two sets are printed (pytest -s).
"""
import os
import sys

import pytest
import torch

import conv_bounds as cb
import conv_census as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (surface samples, voxel size, room dimensions) -> level rows, measured:
ROOMS = {
    "3k":   (2500, 0.05, (4.8, 3.6, 2.4)),       # level 0 below 4096
    "11k":  (12000, 0.04, (4.8, 3.6, 2.4)),      # [11083, 7730, 2992, 700, 137]
    "35k":  (40000, 0.03, (4.8, 3.6, 2.4)),      # [34960, 18772, 5609, 1348, 304]
    "100k": (120000, 0.02, (4.8, 3.6, 2.4)),     # [100999, 47618, 12868, 3052, 700]: the benchmark's S100k
    "hall": (400000, 0.02, (9.6, 7.2, 2.4)),     # [316128, 108632, 27634, 6757, 1602]: level 0 beyond L235k, level 1 above 65 536
}
# row counts that select a kernel or a tile height: stem (4096, 32768), first-generation plan (4096, 32768), weight-stationary limit and
# the tile-list kernel's mid limit (8192), the tile-list kernel's limit (65536), osn_tile_rows' 32-row tiles end at 49152 and its
# 64-row tiles begin at 86016
ROW_THRESHOLDS = (4096, 8192, 32768, 49152, 65536, 86016, 100000, 200000)
OUT_DIM = 768                                    # the distillation head (openseg features); the benchmark's

# key -> one-line reason.  May not name an instance of the tile-list, pair-array, weight-stationary, register-gather, dense, stem,
# first-generation weight-gradient or batched-reduction families: those have cases.
EXEMPT = {
}


@pytest.fixture(scope="module")
def dry(request):
    sys.path.insert(0, os.path.join(ROOT, "tools", "dryrun"))
    import dry_step
    mp = pytest.MonkeyPatch()
    request.addfinalizer(mp.undo)
    lib = dry_step.install(dry_step.build_dry_lib(), mp.setattr)
    return lib, mp


_NETWORK = {}           # (arch, room) -> {pass: keys}
_ROWS = {}              # room -> level rows
_BUILT = {}             # room -> (coordinate manager with every map built, features)


def network_side(dry, archs=None, make_model=None, rooms=None):
    """{(arch, room): {pass: keys}}; the rooms' maps and each (arch, room) log are built once per module."""
    from openscene_amd.mink_unet import _ARCHS, mink_unet
    from openscene_amd.sparse import CoordinateManager
    lib, mp = dry
    archs, rooms = list(archs or _ARCHS), list(rooms or ROOMS)
    for room in rooms:
        if room not in _BUILT:
            coords, feats = cc.room(*ROOMS[room])
            cm = CoordinateManager(coords)
            cm.prebuild()
            _BUILT[room] = (cm, feats)
            _ROWS[room] = [cm.size(s) for s in (1, 2, 4, 8, 16)]
        cm, feats = _BUILT[room]
        for arch in archs:
            if (arch, room) not in _NETWORK:
                torch.manual_seed(0)
                model = (make_model or mink_unet)(3, OUT_DIM, 3, arch)
                _NETWORK[(arch, room)] = cc.network_instances(lib, model, cm, feats, mp.setattr)
    return {(a, r): _NETWORK[(a, r)] for a in archs for r in rooms}


_CASES = {}


def case_side(dry, cases=None):
    lib, _mp = dry
    for case in cb.CASES:
        if case.id not in _CASES:
            _CASES[case.id] = cc.case_instances(lib, case)
    if "batch" not in _CASES:
        _CASES["batch"] = cc.batched_instances(lib)
    ids = [c.id for c in (cb.CASES if cases is None else cases)] + ["batch"]
    return {i: _CASES[i] for i in ids}


def _union(d):
    out = set()
    for v in d.values():
        for w in (v.values() if isinstance(v, dict) else [v]):
            out |= w
    return out


def _missing(net, cases):
    have = _union(cases)
    return {k: sorted("%s/%s/%s" % (a, r, p) for (a, r), passes in net.items() for p, keys in passes.items() if k in keys)
            for k in sorted(_union(net) - have - set(EXEMPT))}


def test_rooms_lie_on_both_sides_of_every_row_threshold(dry):
    network_side(dry, ["MinkUNet14A"])
    assert set(_ROWS) == set(ROOMS)
    rows = sorted(r for v in _ROWS.values() for r in v)
    print("level rows:", _ROWS)
    for t in ROW_THRESHOLDS:
        assert rows[0] < t <= rows[-1], t
    # per level: the thresholds inside the range that level can reach at all lie strictly inside what the rooms cover
    for lvl in range(5):
        lo, hi = min(v[lvl] for v in _ROWS.values()), max(v[lvl] for v in _ROWS.values())
        print("level %d rows %d .. %d" % (lvl, lo, hi))
    assert max(v[0] for v in _ROWS.values()) > 200000 and sorted(v[0] for v in _ROWS.values())[-2] > 100000
    assert min(v[0] for v in _ROWS.values()) < 4096 and max(v[1] for v in _ROWS.values()) > 65536


def test_every_instance_a_network_launches_has_a_case(dry):
    from openscene_amd.mink_unet import _ARCHS
    net, cases = network_side(dry), case_side(dry)
    assert set(a for a, _r in net) == set(_ARCHS) and set(r for _a, r in net) == set(ROOMS)
    assert all(set(p) == {"%s/%s" % (m, path) for m in ("train", "eval-bf16x6", "eval-bf16x3", "eval-bf16x1")
                          for path in ("modules", "executor")} for p in net.values())
    net_keys, case_keys = _union(net), _union(cases)
    print("NETWORK SIDE (%d instances):" % len(net_keys))
    for k in sorted(net_keys):
        print("    %-70s %s" % (k, "" if k in case_keys else ("EXEMPT" if k in EXEMPT else "NO CASE")))
    print("CASE SIDE (%d instances):" % len(case_keys))
    for k in sorted(case_keys):
        print("    %-70s %s" % (k, "" if k in net_keys else "(no network)"))
    missing = _missing(net, cases)
    assert not missing, "instances without a case in conv_bounds.CASES:\n" + "\n".join(
        "  %s   launched by %s" % (k, ", ".join(v[:3]) + (" ... (%d)" % len(v) if len(v) > 3 else "")) for k, v in missing.items())
    # a reduced-precision instance comes from the same case as its three-piece twin, never from an exemption of its own
    stale = sorted(k for k in EXEMPT if k not in net_keys)
    assert not stale, "exempt instances that no network launches any more: %s" % stale
    covered = sorted(k for k in EXEMPT if k in case_keys)
    assert not covered, "exempt instances that have a case: %s" % covered
    assert all(isinstance(v, str) and v.strip() and "\n" not in v for v in EXEMPT.values())


def test_the_executor_and_the_module_path_launch_the_same_instances_but_for_the_epilogues(dry):
    """(EPI is dropped from the key, so the two paths must agree per pass -- except for what only one of them has: the batched
    reduction and the elementwise kernels are the executor's / the module path's own.)"""
    net = network_side(dry, ["MinkUNet18A", "MinkUNet34C"])
    own = {"wgrad_tl_reduce_batch_kernel<>", "wgrad_tl_reduce_kernel<>"}
    for (arch, room), passes in net.items():
        for mode in ("train", "eval-bf16x6", "eval-bf16x3", "eval-bf16x1"):
            a, b = passes[mode + "/modules"] - own, passes[mode + "/executor"] - own
            assert a == b, "%s %s %s: %s" % (arch, room, mode, sorted(a ^ b))


def test_the_census_sees_a_removed_case_and_an_unknown_width(dry):
    """The census' own teeth.  For every instance the networks launch: without the cases that reach it, it is reported (and only it and
    the instances those cases were alone to reach).  A variant with a 160-channel decoder launches instances no case reaches."""
    net, cases = network_side(dry), case_side(dry)
    net_keys = _union(net)
    alone = set()
    for k in sorted(net_keys):
        reach = [i for i, keys in cases.items() if k in keys]
        assert reach, k
        fewer = [c for c in cb.CASES if c.id not in reach]
        left = _union({i: _CASES[i] for i in [c.id for c in fewer] + ([] if "batch" in reach else ["batch"])})
        assert k not in left and k in net_keys - left - set(EXEMPT)
        if len(reach) == 1:
            alone.add(reach[0])
    print("%d of %d cases are the only one to reach some network instance; removing one of them alone fails the census" % (
        len(alone), len(cb.CASES)))
    one = next(c for c in cb.CASES if c.id in alone and c.family == "dense" and (c.cin, c.cout) == (64, 128))
    missing = _missing(net, case_side(dry, [c for c in cb.CASES if c.id != one.id]))
    assert list(missing) == ["dense_kernel<KS=2> pieces=%d" % p for p in (1, 2, 3)], missing

    from openscene_amd import mink_unet as mu
    scratch = mu._variant("MinkUNet18Scratch", mu.BasicBlock, (2,) * 8, (32, 64, 128, 256, 128, 128, 160, 160))
    try:
        net = network_side(dry, ["MinkUNet18Scratch"], make_model=lambda i, o, d, arch: scratch(i, o, d), rooms=["11k", "100k"])
    finally:
        for k in [k for k in _NETWORK if k[0] == "MinkUNet18Scratch"]:
            del _NETWORK[k]
    missing = _missing(net, cases)
    print("the 160-channel decoder's instances without a case:", sorted(missing))
    assert any(k.startswith("spconv_tl_kernel<NW=1,KS=4,RAGGED=1,OCC=2,BUFG=0>") for k in missing), missing
