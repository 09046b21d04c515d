"""coords_edges.py on the CPU: the unmutated model of the integer pipeline reproduces the oracle (tests/cpu_backend.py) on every
edge case, every mutant is caught by the cases named for it (coords_edges.CATCHES), the scan's carry was out of reach of the sizes
the suite had before, and the generators really reach what they claim: wrap_cloud wraps, range_cloud hits and leaves every face.

Case  x  mutant (x = the mutated model differs from the reference on that case; asserted and printed by test_mutant_is_caught_by_its_cases):

                      scan_carry  scan_carry  scan_total_without  scan_block  probe_    floor_div_  range_inclusive  sort_     mask_bit
                      _lost       _once       _last_block         _edge       no_wrap   truncates   _off_by_one      unstable  _order
  big_cloud           x           .  (a)      x                                         x
  big_duplicates      x           x
  boundary                                    x                   x
  range_cloud                                                                           x
  range_raises                                                                                      x
  wrap_cloud                                                                  x
  sort_wrap_cloud                                                                                                    x         x
  sort_big_cloud                                                                                                     x         x
  legacy_cloud (b)    .           .

  (a) big_cloud has two chunks of block sums; the one carry there is goes to the second chunk, which scan_carry_once still does.
  (b) about 800 k rows with duplicates, the largest the suite fed the unique pipeline before: one chunk, no carry to lose.
"""
import numpy as np
import pytest
import torch

from oracle import coords as oc

import coords_edges as ce
import cpu_backend

_CACHE = {}             # one construction of every 2^20 case and of its reference per module


def _cached(name, fn):
    if name not in _CACHE:
        _CACHE[name] = fn()
    return _CACHE[name]


def _t(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy())          # the cached clouds are read-only


def _ref_unique(c, stride=1):
    u, inv, first, table = cpu_backend.coords_unique(_t(c), stride)
    return u.numpy(), inv.numpy(), first.numpy(), table


def _ref_pyramid(name, c):
    return _cached(("ref_pyramid", name), lambda: [(u.numpy(), i.numpy(), f.numpy(), t) for u, i, f, t in cpu_backend.coords_pyramid(_t(c))])


def _same_unique(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))


def _same_pyramid(got, want):
    return len(got) == len(want) and all(_same_unique(g, w) for g, w in zip(got, want))


def _ref_sort(nbr, counts):
    o, t, g = cpu_backend.kmap_sort(_t(nbr), None if counts is None else _t(counts))
    return o.numpy(), t.numpy(), g.numpy()


def _same_sort(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


SUB = 1 << 17           # level-1 rows the big strided map is built for: kmap_build has no path that depends on the row count


def _big_up_table():
    """the 2^3 map level 0 -> level 1 of big_cloud for the first SUB level-1 rows, transposed (K = 8, N_BIG columns, one offset per
    row or none), from the model's pyramid, with its counts."""
    def make():
        pyr = _cached("model_pyramid_big", lambda: ce.model_pyramid(ce.big_cloud()))
        down, cnt = ce.model_kmap_build(pyr[0][3], pyr[1][0][:SUB], 2, 1)
        return cpu_backend.kmap_transpose(_t(down), pyr[0][0].shape[0]).numpy(), cnt, down
    return _cached("big_up_table", make)[:2]


def _wrap_map():
    def make():
        w = ce.wrap_cloud()
        u, _, _, t = ce.model_unique(w.rows)
        return ce.model_kmap_build(t, u, 3, 1)
    return _cached("wrap_map", make)


# ------------------------------------------------------------------------------------------------ the model is right
def test_model_scan_is_a_prefix_sum_at_every_block_and_chunk_edge():
    rng = np.random.default_rng(0)
    for n in ce.BOUNDARY_SIZES + (2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 20 + 1024, 2 ** 21 + 7):
        f = rng.random(n) < 0.4
        out, total = ce.model_scan(f)
        assert np.array_equal(out, np.cumsum(f) - f) and total == int(f.sum()), n


def test_pack_and_hash_known_answers():
    """common.h by hand: (b, x, y, z) = (1, -32768 + 2, 0, 32767) -> fields 0001 0002 8000 FFFF."""
    assert int(ce.pack_key(np.array([[1, -32766, 0, 32767]]))[0]) == 0x000100028000FFFF
    M = (1 << 64) - 1
    for k in (0, 1, 0x000100028000FFFF, M - 1):                 # the finaliser again, in Python integers
        h = k
        h = ((h ^ (h >> 30)) * 0xBF58476D1CE4E5B9) & M
        h = ((h ^ (h >> 27)) * 0x94D049BB133111EB) & M
        h ^= h >> 31
        assert int(ce.hash_key(np.array([k], dtype=np.uint64))[0]) == h & 0xFFFFFFFF
    assert [ce.hash_capacity(n) for n in (0, 512, 513, 1024, 1025)] == [1024, 1024, 2048, 2048, 4096]


@pytest.mark.parametrize("name", ["big_cloud", "big_duplicates"])
def test_model_equals_the_oracle_past_2_20_rows(name):
    c = getattr(ce, name)()
    assert c.shape[0] > 2 ** 20 and c.dtype == np.int32
    if name == "big_cloud":
        assert c.shape[0] == ce.N_BIG and np.unique(ce.pack_key(c)).shape[0] == ce.N_BIG and set(np.unique(c[:, 0])) == {0, 1, 2, 3}
        want = _ref_pyramid(name, c)
        got = _cached("model_pyramid_big", lambda: ce.model_pyramid(c))
        sizes = [w[0].shape[0] for w in want]
        print("big_cloud level sizes", sizes)
        assert sizes[0] == ce.N_BIG and 2 ** 19 < sizes[1] < 2 ** 20 and sizes[1] > sizes[2] > sizes[3] > sizes[4] > 1000
        assert _same_pyramid(got, want)
        # the strided 2^3 map level 0 -> level 1 and its transposed table (K = 8), and the tile order of the latter
        down = cpu_backend.kmap_build(want[0][3], _t(want[1][0][:SUB]), 2, 1).numpy()
        up, cnt = _big_up_table()
        assert up.shape == (8, ce.N_BIG) and int(cnt.sum()) > SUB
        assert np.array_equal(_CACHE["big_up_table"][2], down)
        for counts in (None, cnt):
            assert _same_sort(ce.model_kmap_sort(up, counts), _ref_sort(up, counts))
    else:
        assert c.shape[0] == ce.N_DUP
        want = _cached("ref_unique_dup", lambda: _ref_unique(c))
        got = ce.model_unique(c)
        n_u = want[0].shape[0]
        assert 0.99 * ce.N_DUP_DISTINCT < n_u <= ce.N_DUP_DISTINCT and _same_unique(got, want)     # e^-7 of the pool is never drawn
        nbr = ce.model_kmap_build(got[3], got[0], 1, 1)[0]
        assert np.array_equal(nbr[0], np.arange(n_u))
        assert np.array_equal(nbr, cpu_backend.kmap_build(want[3], _t(want[0]), 1, 1).numpy())


def test_model_equals_the_oracle_at_the_block_boundaries():
    for n, last in ce.boundary_cases():
        c = ce.boundary_cloud(n, last)
        assert c.shape == (n, 4)
        want = _ref_unique(c)
        dup = n - want[0].shape[0]
        assert n < 8 or 0.2 * n < dup < 0.5 * n, (n, last, dup)                  # about a third of the rows are duplicates
        assert (int(want[2][-1]) == n - 1) == (last == "first")                # the last row is / is not a first occurrence
        for s in (1, 2):
            assert _same_unique(ce.model_unique(c, s), _ref_unique(c, s)), (n, last, s)
        if n >= 1023:
            pyr = ce.model_pyramid(c)
            assert _same_pyramid(pyr, [(u.numpy(), i.numpy(), f.numpy()) for u, i, f, _ in cpu_backend.coords_pyramid(_t(c))]), (n, last)
            assert np.array_equal(ce.model_kmap_build(pyr[0][3], pyr[0][0], 3, 1)[0],
                                  cpu_backend.kmap_build(cpu_backend.HashTable(pyr[0][0]), _t(pyr[0][0]), 3, 1).numpy())


def _range_levels():
    def make():
        c = ce.range_cloud()
        return [(u.numpy(), i.numpy(), f.numpy()) for u, i, f, _ in cpu_backend.coords_pyramid(_t(c), (1, 2))]
    return _cached("range_levels", make)


def test_model_equals_the_masked_oracle_on_the_range_cloud():
    c = ce.range_cloud()
    assert ce.in_range(c, ce.DOC_LIM).all() and set(c[:, 0]) == {0, ce.BATCH_MAX}
    want = _range_levels()
    got = ce.model_pyramid(c, (1, 2))
    assert _same_pyramid(got, want)
    for lvl, scale in enumerate((1, 2)):
        for k in ce.KSIZES:
            nbr = ce.model_kmap_build(got[lvl][3], got[lvl][0], k, scale)[0]
            assert np.array_equal(nbr, ce.masked_kernel_map(want[lvl][0], want[lvl][0], k, scale)), (k, scale)
    down = ce.model_kmap_build(got[0][3], got[1][0], 2, 1)[0]                     # the strided map level 0 -> level 1
    assert np.array_equal(down, ce.masked_kernel_map(want[0][0], want[1][0], 2, 1))
    for counts in (None, (down >= 0).sum(1)):
        assert _same_sort(ce.model_kmap_sort(down, counts), _ref_sort(down, counts))


def test_the_unmasked_oracle_aliases_past_the_range():
    """Why masked_kernel_map exists: oracle.coords.pack ORs its fields together unmasked, so z = 32766 + 4 sets the lowest bit of the
    y field and leaves z = -32766 behind: with an odd biased y the probe of voxel 0 finds voxel 1 at the opposite face."""
    c = np.array([[0, 5, 1, 32766], [0, 5, 1, -32766]], dtype=np.int32)
    k = 4 * 25 + 2 * 5 + 2                                                      # offset (0, 0, +2) of a 5^3 kernel, times scale 2
    assert oc.kernel_map(c, c, oc.kernel_offsets(5, 2))[k, 0] == 1
    assert ce.probe_out_of_range(c, 5, 2)[k, 0] and ce.masked_kernel_map(c, c, 5, 2)[k, 0] == -1
    assert ce.model_kmap_build(ce.model_unique(c)[3], c, 5, 2)[0][k, 0] == -1


def test_range_cloud_hits_and_leaves_every_face():
    """For every kernel size: a hit whose target lies within three cells of each of the six faces, and a probe with a component outside
    [-32767, 32767] through each face an offset of that size can point through -- all six for the centred odd sizes; an even size spans
    [0, k), so it leaves through the three positive faces only, and size 2 does so at scale 2 (32766 + 1 is still packable)."""
    lv = _range_levels()
    for k in ce.KSIZES:
        hit_faces, out_faces = set(), set()
        for lvl, scale in enumerate((1, 2)):
            c = lv[lvl][0].astype(np.int64)
            nbr = ce.masked_kernel_map(c, c, k, scale)
            off = oc.kernel_offsets(k, scale).astype(np.int64)
            tgt = c[None, :, 1:] + off[:, None, :]
            for axis in range(3):
                for sign in (-1, 1):
                    near = sign * tgt[:, :, axis] >= ce.DOC_LIM - 3 * scale
                    moved = off[:, axis][:, None] != 0                     # a neighbour along this axis, not the voxel itself
                    if ((nbr >= 0) & near & moved).any():
                        hit_faces.add((axis, sign))
                    if (sign * tgt[:, :, axis] > ce.LIM).any():
                        out_faces.add((axis, sign))
        assert len(hit_faces) == 6, (k, hit_faces)
        want_out = {(a, s) for a in range(3) for s in ((-1, 1) if k & 1 else (1,))}
        assert out_faces == want_out, (k, out_faces)


def test_range_rows_raise_in_the_model():
    for name, c, strides in ce.range_raises():
        for s in strides:
            with pytest.raises(ce.ModelRangeError):
                ce.model_unique(c, s)
            if s == 2:
                with pytest.raises(ce.ModelRangeError):
                    ce.model_pyramid(c, (1, 2))
        if strides == (2,):
            ce.model_unique(c, 1)                                               # in range until it is quantised


def test_wrap_cloud_really_wraps():
    w = ce.wrap_cloud()
    cap = w.cap
    assert cap == ce.hash_capacity(w.rows.shape[0]) == 1024 and np.unique(w.rows, axis=0).shape[0] == w.rows.shape[0]
    assert int((w.home >= cap - 3).sum()) >= 12 and int(((w.home >= 1) & (w.home <= 7)).sum()) >= 6 and w.rows.shape[0] >= 300
    assert not (w.home == 0).any() and not w.occupied[cap - 4]
    home_of_slot = ce.hash_key(w.keys) & (cap - 1)
    assert w.occupied[cap - 1] and w.occupied[0] and home_of_slot[cap - 1] >= cap - 3 and home_of_slot[0] >= cap - 3
    spilled = int((w.occupied[:32] & (home_of_slot[:32] >= cap - 3)).sum())
    assert spilled >= 11                                                        # 14 keys for three slots
    displaced = w.occupied & (home_of_slot <= 7) & (np.arange(cap) > home_of_slot)
    assert int(displaced.sum()) >= 6                                            # the keys homed in slots 1 .. 7 moved on
    assert int(w.occupied.sum()) == w.rows.shape[0]
    # the occupied set does not depend on the insertion order
    rev = ce.ModelTable.insert(ce.pack_key(w.rows[::-1]), cap)
    assert np.array_equal(rev.keys != ce.KEY_EMPTY, w.occupied)
    # model = oracle on it, the wrapped probes included
    u, inv, first, t = ce.model_unique(w.rows)
    assert _same_unique((u, inv, first), _ref_unique(w.rows))
    assert np.array_equal(t.keys != ce.KEY_EMPTY, w.occupied)
    nbr, cnt = _wrap_map()
    assert np.array_equal(nbr, cpu_backend.kmap_build(cpu_backend.HashTable(u), _t(u), 3, 1).numpy())
    for counts in (None, cnt):
        assert _same_sort(ce.model_kmap_sort(nbr, counts), _ref_sort(nbr, counts))


# ------------------------------------------------------------------------------------------------ every mutant is caught
def _caught(case, mutant):
    """True when the mutated model's output differs from the reference on the named case."""
    if case == "big_cloud":
        c = ce.big_cloud()
        return not _same_pyramid(ce.model_pyramid(c, mutant=mutant), _ref_pyramid(case, c))
    if case == "big_duplicates":
        c = ce.big_duplicates()
        return not _same_unique(ce.model_unique(c, mutant=mutant), _cached("ref_unique_dup", lambda: _ref_unique(c)))
    if case == "legacy_cloud":
        c = ce.legacy_cloud()
        return not _same_unique(ce.model_unique(c, mutant=mutant), _ref_unique(c))
    if case == "boundary":
        hits = [(n, last) for n, last in ce.boundary_cases()
                if not _same_unique(ce.model_unique(ce.boundary_cloud(n, last), mutant=mutant), _ref_unique(ce.boundary_cloud(n, last)))]
        if mutant == "scan_block_edge":             # exactly the sizes with a first occurrence at an index 1024 j
            assert hits == [(n, "first") for n in ce.BOUNDARY_SIZES if n > 1024], hits
        if mutant == "scan_total_without_last_block":       # every cloud whose last scan block holds a first occurrence
            want = [(n, last) for n, last in ce.boundary_cases()
                    if _ref_unique(ce.boundary_cloud(n, last))[2][-1] >= (n - 1) // ce.SCAN_BLOCK * ce.SCAN_BLOCK]
            assert hits == want and len(want) >= len(ce.boundary_cases()) - 2, hits
        return bool(hits)
    if case == "range_cloud":
        return not _same_pyramid(ce.model_pyramid(ce.range_cloud(), (1, 2), mutant=mutant), _range_levels())
    if case == "range_raises":
        n_missed = 0
        for _, c, strides in ce.range_raises():
            for s in strides:
                try:
                    ce.model_unique(c, s, mutant=mutant)
                    n_missed += 1                   # the reference behaviour is to raise
                except ce.ModelRangeError:
                    pass
        return n_missed > 0
    if case == "wrap_cloud":
        w = ce.wrap_cloud()
        u, _, _, t = ce.model_unique(w.rows, mutant=mutant)
        return not np.array_equal(ce.model_kmap_build(t, u, 3, 1, mutant=mutant)[0], _wrap_map()[0])
    if case in ("sort_wrap_cloud", "sort_big_cloud"):
        nbr, cnt = _wrap_map() if case == "sort_wrap_cloud" else _big_up_table()
        return not _same_sort(ce.model_kmap_sort(nbr, cnt, mutant=mutant), _ref_sort(nbr, cnt))
    raise KeyError(case)


def test_catch_table_names_every_mutant():
    assert set(ce.CATCHES) == set(ce.MUTANTS) and all(ce.CATCHES[m] for m in ce.MUTANTS)


@pytest.mark.parametrize("mutant", ce.MUTANTS)
def test_mutant_is_caught_by_its_cases(mutant):
    for case in ce.CATCHES[mutant]:
        assert _caught(case, mutant), "%s is not caught by %s" % (mutant, case)
        print("%-32s caught by %s" % (mutant, case))


@pytest.mark.parametrize("mutant", ce.NOT_CAUGHT_BEFORE)
def test_the_carry_was_out_of_reach_of_the_sizes_the_suite_had(mutant):
    assert not _caught("legacy_cloud", mutant)
    assert ce.legacy_cloud().shape[0] <= ce.SCAN_BLOCK * ce.SCAN_CHUNK
    f = np.random.default_rng(1).random(2 ** 20) < 0.5              # 1024 blocks exactly: still one chunk
    out, total = ce.model_scan(f, mutant)
    assert np.array_equal(out, np.cumsum(f) - f) and total == int(f.sum())


def test_scan_carry_once_needs_three_chunks():
    """Footnote (a) of the table: big_cloud cannot see scan_carry_once, big_duplicates can."""
    assert not _caught("big_cloud", "scan_carry_once")
