"""The shapes each convolution kernel family is routed to are stated three times on purpose -- the library's own export beside the
kernel (osn_*_ok: the one statement the executor and openscene_amd.ops both ask), ops.*_eligible (a memoised call of it) and
tests/cpu_backend.py (the independent spec, used where no device exists) -- and held together here, WITHOUT a GPU: the exports
are host arithmetic."""
import itertools

import pytest

import cpu_backend

K_GRID = [1, 2, 8, 27, 32, 33, 64, 125, 126, 128, 129]
C_GRID = [1, 3, 4, 5, 8, 12, 30, 32, 64, 96, 128, 256, 512, 516, 768, 1024]
N_GRID = [0, 1, 31, 4095, 4096, 32767, 32768, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 31) - 1]
# The stem kernels take one output width and the register-gather kernel two widths per side: on the grid above they say yes to 0.75 %
# and 0.87 % of the tuples.  Their own neighbourhoods, added to the sweep:
STEM_NEAR = list(itertools.product([1, 2, 3, 27, 124, 125, 126], [1, 2, 3, 4, 5], [31, 32, 33]))
RG_NEAR = list(itertools.product([1, 2, 8, 27, 125, 128, 129], [32, 64, 96], [32, 64, 96],
                                 [1, 4096, 100000, (1 << 23) - 1, 1 << 23, (1 << 24) - 1, 1 << 24]))
KCC = list(itertools.product(K_GRID, C_GRID, C_GRID))
KCCN = list(itertools.product(K_GRID, C_GRID, C_GRID, N_GRID))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from openscene_amd import _lib
    return _lib.load()


@pytest.fixture()
def ops(monkeypatch):
    from openscene_amd import ops
    monkeypatch.setattr(ops, "_size_cache", {})          # the sweep's 100 k answers do not stay in the process
    return ops


def families(lib):
    """name -> (tuples in the argument order of ops.X, the export called as both of its callers call it)."""
    return {
        "stem_eligible": (KCC + STEM_NEAR, lambda K, cin, cout: lib.osn_stem_conv_ok(K, cin, cout)),
        "tl_eligible": (KCCN, lambda K, cin, cout, n=0: lib.osn_spconv_fwd_tl_ok(n, K, cin, cout)),
        "dense_eligible": (list(itertools.product(C_GRID, C_GRID)), lambda cin, cout: lib.osn_dense_fwd_ok(cin, cout)),
        # (csrc/net.hip and ops.rg_eligible both ask about at least one row: the export itself refuses an empty matrix)
        "rg_eligible": (KCCN + RG_NEAR, lambda K, cin, cout, n: lib.osn_spconv_fwd_rg_ok(max(n, 1), K, cin, cout)),
        "x6_eligible": (KCCN, lambda K, cin, cout, n: lib.osn_spconv_fwd_x6_ok(n, K, cin, cout)),
    }


@pytest.mark.parametrize("name", ["stem_eligible", "tl_eligible", "dense_eligible", "rg_eligible", "x6_eligible"])
def test_library_ops_and_spec_agree_on_the_grid(lib, ops, name):
    tuples, export = families(lib)[name]
    in_ops, spec = getattr(ops, name), getattr(cpu_backend, name)
    yes = 0
    for t in tuples:
        got = export(*t)
        assert got in (0, 1), (name, t, got)
        a, b = in_ops(*t), spec(*t)
        assert a is bool(got) and bool(b) == a, "%s%r: library %d, ops %r, cpu_backend %r" % (name, t, got, a, b)
        yes += got
    share = yes / len(tuples)
    print("%s: yes on %d of %d tuples (%.2f %%)" % (name, yes, len(tuples), 100 * share))
    assert 0.01 <= share <= 0.99, "%s answers the same on (almost) the whole sweep: %.2f %% yes" % (name, 100 * share)


# one tuple just inside and one just outside every clause; arguments in the order of ops.X
EDGES = {
    "stem_eligible": [
        ((125, 3, 32), True), ((126, 3, 32), False),                       # K: 5^3 at most
        ((2, 3, 32), True), ((1, 3, 32), False),                           # a table, not a 1x1 conv
        ((27, 4, 32), True), ((27, 5, 32), False), ((27, 1, 32), True),    # cin <= 4
        ((27, 3, 31), False), ((27, 3, 33), False),                        # cout == 32
    ],
    "tl_eligible": [
        ((27, 64, 64, 1 << 24), True), ((27, 64, 64, (1 << 24) + 1), False),        # input rows packed into 24 bits
        ((27, 64, 64, 0), True), ((27, 64, 64), True),                              # asked before the rows are known
        ((27, 512, 64, 1000), True), ((27, 516, 64, 1000), False),                  # four 128-channel chunks
        ((27, 8, 64, 1000), True), ((27, 4, 64, 1000), False), ((27, 10, 64, 1000), False),
        ((27, 64, 4, 1000), True), ((27, 64, 66, 1000), False),
        ((128, 64, 64, 1000), True), ((129, 64, 64, 1000), False), ((1, 64, 64, 1000), True),
    ],
    "dense_eligible": [
        ((8, 4), True), ((4, 4), False), ((10, 8), False), ((12, 8), True), ((8, 6), False), ((512, 768), True), ((1024, 4), True),
    ],
    "rg_eligible": [
        ((27, 64, 64, (1 << 23) - 1), True), ((27, 64, 64, 1 << 23), False),        # the feature matrix below 2 GB: 64 channels x 4 bytes
        ((27, 32, 32, (1 << 24) - 1), True), ((27, 32, 32, 1 << 24), False),        # rows below 2^24
        ((27, 32, 64, 0), True),                                                    # an empty matrix is asked about as one row
        ((2, 32, 32, 1000), True), ((1, 32, 32, 1000), False), ((128, 32, 32, 1000), True), ((129, 32, 32, 1000), False),
        ((27, 96, 32, 1000), False), ((27, 32, 96, 1000), False), ((27, 64, 32, 1000), True),
    ],
    "x6_eligible": [
        # the weight image, 3 planes of K x cout x (cin padded to 32) bf16, below 2^30 elements: 3 x 349525 x 1024 = 2^30 - 1024
        ((1, 1024, 349525, 100000), True), ((1, 1024, 349526, 100000), False),
        ((1, 1000, 349525, 100000), True), ((1, 1000, 349526, 100000), False),      # (the padded width counts)
        # at most 32 offsets per block.  K = 125, 32 -> 32 (tiles of 128 rows): up to 255 tiles the plan brings the launch to 768
        # blocks with 4 offset groups of 32; from 256 tiles on with 3 groups of 42
        ((125, 32, 32, 255 * 128), True), ((125, 32, 32, 255 * 128 + 1), False),
        # a big map is not split at all; a small one of the same conv into groups of 3 offsets
        ((32, 32, 32, 100000), True), ((33, 32, 32, 100000), False), ((33, 32, 32, 1000), True),
        ((27, 8, 32, 1000), True), ((27, 4, 32, 1000), False), ((27, 10, 32, 1000), False),
        ((27, 32, 32, 0), True), ((27, 32, 32, -5), True),                          # no rows: planned as one row
    ],
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_every_clause_has_a_tuple_on_each_side(lib, ops, name):
    _, export = families(lib)[name]
    for t, want in EDGES[name]:
        got = (bool(export(*t)), getattr(ops, name)(*t), bool(getattr(cpu_backend, name)(*t)))
        assert all(g is want for g in got), "%s%r: want %r, (library, ops, cpu_backend) say %r" % (name, t, want, got)
