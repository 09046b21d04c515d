"""The C-ABI library loads (no GPU needed) and exports exactly what include/openscene_amd.h declares."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "openscene_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(osn_[a-z0-9_]+)\s*\(", src))


def test_library_builds_loads_and_exports_header_symbols():
    import __graft_entry__ as ge
    ge.build()
    from openscene_amd import _lib
    lib = _lib.load()
    names = declared_functions()
    assert len(names) >= 25
    assert names == set(_lib.PROTOTYPES), (names ^ set(_lib.PROTOTYPES))
    for n in names:
        assert hasattr(lib, n), "missing export " + n
    # ... and nothing else under the library's prefix: a leftover export of a retired name fails here
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split("\n")
    exported = {f[-1] for f in (l.split() for l in syms) if f and f[-1].startswith("osn_")}
    assert exported == names, (exported ^ names)
    assert lib.osn_version() == 3
    assert lib.osn_hash_capacity(1000) == 2048 and lib.osn_hash_capacity(0) == 1024
    assert lib.osn_bn_ws_bytes(10, 32) > 0 and lib.osn_coords_unique_ws_bytes(1000) > 0
    # big maps: room for the (K/8 - 1) partial buffers of the units mode; 1x1 convs need no scratch
    assert lib.osn_spconv_fwd_ws_bytes(100999, 27, 96, 96) >= 3 * 100999 * 96 * 4
    assert lib.osn_spconv_fwd_ws_bytes(100999, 1, 96, 768) == 0
    assert lib.osn_spconv_fwd_ws_bytes(700, 27, 256, 256) > 0            # deep level: split + reduce buffer
    assert lib.osn_weight_prep_x6_bytes(27, 96, 128, 0) == 3 * 27 * 128 * 96 * 2
    # second-generation kernels: tile rows between 32 and 64 (round 4: three workgroups per CU), fragment images of 1 KB blocks, pair-list buffers
    assert lib.osn_tile_rows(100999) == 64 and lib.osn_tile_rows(3052) == 32 and lib.osn_tile_rows(47618) == 32
    assert lib.osn_weight_prep_tl_bytes(27, 96, 96, 0) == 3 * 27 * 3 * 6 * 1024
    assert lib.osn_tile_lists_bytes(1000, 27, 32) > 27 * 1000 * 8 and lib.osn_pair_lists_bytes(1000, 27, 32) > 2 * 27 * 1000 * 4
    assert lib.osn_spconv_fwd_tl_ws_bytes(100999, 27, 96, 64) == 512                 # big table: no offset split
    assert lib.osn_spconv_fwd_tl_ws_bytes(700, 27, 256, 32) > 256                    # small table: partial tiles


def test_header_cites_reference_lines():
    src = open(os.path.join(ROOT, "include", "openscene_amd.h")).read()
    for cite in ("run/evaluate.py:290-292", "dataset/voxelizer.py:117-129", "models/mink_unet.py", "run/distill.py:316-317"):
        assert cite in src


# ---- one name per operation (ABI 3): the argument checks of the folded entries.  No kernel is launched: every call returns before
# it touches the device, and the message names the entry that was called.
def test_folded_entries_argument_errors():
    import __graft_entry__ as ge
    ge.build()
    from openscene_amd import _lib
    h = _lib.load()
    n, c = 8, 16
    ws_bytes = h.osn_bn_ws_bytes(n, c)
    buf = (ctypes.c_char * (4096 + ws_bytes + 16))()
    p = (ctypes.addressof(buf) + 15) & ~15
    gys = (ctypes.c_void_p * 4)(p + 1024, p + 1024, p + 1024, p + 1024)
    lds = (ctypes.c_int64 * 4)(c, c, c, c)

    def backward(y=p + 512, n_gy=1, beta=None, relu=1, gres=None):
        return h.osn_bn_backward(p, y, gys, lds, n_gy, p + 2048, p + 2112, p + 2176, beta, 1e-5, relu, 1, p + 2560, gres, p + 2240,
                                 p + 2304, n, c, p + 4096, ws_bytes, None)
    for bad in (dict(y=None), dict(y=None, beta=p + 2368, gres=p + 3072), dict(n_gy=0), dict(n_gy=4)):
        assert backward(**bad) == -1, bad                     # OSN_E_ARG
        assert _lib.last_error().startswith("osn_bn_backward:"), _lib.last_error()
    # a second destination whose row stride is below the width
    rc = h.osn_bn_apply(p, p + 2048, p + 2112, p + 2176, p + 2368, 1e-5, None, 0, p + 512, p + 1024, c - 4, n, c, None)
    assert rc == -1 and _lib.last_error().startswith("osn_bn_apply:"), _lib.last_error()
