"""Edge cases of the integer pipeline in one place (plain helper module; imported by test_coords_edges_cpu.py and
test_gpu_coords_edges.py): seeded case generators for the regimes no other test reaches, and a numpy model of the index
arithmetic of csrc/coords.hip and csrc/kmap_sort.hip, with one defect at a time (MUTANTS).

The model is not the kernel.  It restates WHERE the kernels put an index -- the three-launch scan with its 1024-element blocks and
its 1024-block chunks of block sums, the range checks in front of pack_key, the linear probe with its wrap, the rank of a key bit --
so that the CPU test can prove that the inputs below tell a right pipeline from a subtly wrong one.  The GPU test then holds the
kernels to the oracle (oracle/coords.py through tests/cpu_backend.py) on the same inputs, bit for bit.

Regimes (each generator's docstring says what it reaches):
  big_cloud, big_duplicates   more than 2^20 rows: scan_sums_kernel's second / third chunk and its carry (coords.hip, `carry_s`),
                              the pyramid's grid of more than 1024 blocks with the count read from device memory, rocPRIM's sort
                              path above 1 M items (kmap_sort.hip)
  boundary_cloud              row counts at and beside the multiples of 64 (wave), 256 (workgroup), 1024 (scan block)
  range_cloud, range_raises   voxels at the documented limit |c| <= 32766, scene 65534; probes and quantisation steps across it
  wrap_cloud                  a hash cluster that spills from the last slots of the table to slot 0

Which case catches which mutant: CATCHES (asserted by test_coords_edges_cpu.py).

The oracle's trap.  oracle.coords.pack does not range-check and ORs its 16-bit fields together without masking, so a probe with a
component outside [-32767, 32767] spills into the neighbouring field and can alias a voxel near the OPPOSITE face
(test_coords_edges_cpu.py has a two-voxel example).  The kernels refuse those probes (kmap_build_kernel's range check), so the range reference
(masked_kernel_map) turns every such probe into a miss: it drops the oracle's answer for it, whatever the aliased key found -- the
same table as masking the probe before the lookup.
"""
import functools
import types

import numpy as np

from oracle import coords as oc

# ------------------------------------------------------------------------------------------------ constants of the kernels
SCAN_BLOCK = 1024                       # coords.hip: SCAN_TPB * SCAN_IPT elements per block of scan_block_kernel
SCAN_CHUNK = 1024                       # scan_sums_kernel scans the block sums 1024 at a time
COORD_BIAS = 1 << 15                    # common.h
LIM = COORD_BIAS - 1                    # the range checks accept |c| <= LIM; the documents promise |c| < 32767
DOC_LIM = 32766                         # the documented cube: |c| <= 32766, batch <= 65534
BATCH_MAX = 65534
KEY_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
VAL_EMPTY = 0x7F7F7F7F

N_BIG = 2 ** 20 + 3 * 1024 + 5          # 1 051 653: two chunks of block sums, 1028 blocks, the last one partial
N_DUP = 2 ** 21 + 7                     # 2 097 159: three chunks
N_DUP_DISTINCT = 300000
BOUNDARY_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 4097)
boundary_sizes = BOUNDARY_SIZES
KSIZES = (2, 3, 5, 7)

MUTANTS = ("scan_carry_lost", "scan_carry_once", "scan_total_without_last_block", "scan_block_edge", "probe_no_wrap",
           "floor_div_truncates", "range_inclusive_off_by_one", "sort_unstable", "mask_bit_order")

# mutant -> the named cases whose model output must differ from the reference (test_coords_edges_cpu.py runs exactly these)
#   scan_carry_once needs THREE chunks of block sums: with two, the only carry there is goes to the second chunk, which is what the
#   mutant still does -- so big_duplicates (2049 blocks) sees it and big_cloud (1028 blocks) cannot; scan_carry_lost is seen by both.
CATCHES = {
    "scan_carry_lost": ("big_cloud", "big_duplicates"),
    "scan_carry_once": ("big_duplicates",),
    "scan_total_without_last_block": ("boundary", "big_cloud"),
    "scan_block_edge": ("boundary",),
    "probe_no_wrap": ("wrap_cloud",),
    "floor_div_truncates": ("range_cloud", "big_cloud"),
    "range_inclusive_off_by_one": ("range_raises",),
    "sort_unstable": ("sort_wrap_cloud", "sort_big_cloud"),
    "mask_bit_order": ("sort_wrap_cloud", "sort_big_cloud"),
}
# the scan's carry is out of reach of every size the suite had before (all at most 1024 blocks): asserted on legacy_cloud
NOT_CAUGHT_BEFORE = ("scan_carry_lost", "scan_carry_once")


class ModelRangeError(Exception):
    """The model's OpenSceneAmdError: a coordinate outside the packable range."""


# ------------------------------------------------------------------------------------------------ common.h in numpy
def hash_capacity(n):
    """osn_hash_capacity"""
    cap = 1024
    while cap < 2 * n:
        cap <<= 1
    return cap


def pack_key(c4):
    """common.h pack_key: four 16-bit fields, each masked (uint64)."""
    c = np.asarray(c4).astype(np.int64)
    f = lambda v: (v & 0xFFFF).astype(np.uint64)
    return (f(c[:, 0]) << np.uint64(48)) | (f(c[:, 1] + COORD_BIAS) << np.uint64(32)) | \
           (f(c[:, 2] + COORD_BIAS) << np.uint64(16)) | f(c[:, 3] + COORD_BIAS)


def hash_key(k):
    """common.h hash_key: the splitmix64 finaliser, low 32 bits."""
    k = np.asarray(k, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(30)
        k *= np.uint64(0xBF58476D1CE4E5B9)
        k ^= k >> np.uint64(27)
        k *= np.uint64(0x94D049BB133111EB)
        k ^= k >> np.uint64(31)
    return (k & np.uint64(0xFFFFFFFF)).astype(np.int64)


def home_slot(c4, cap):
    return hash_key(pack_key(c4)) & (cap - 1)


def in_range(c4, lim=LIM):
    c = np.asarray(c4).astype(np.int64)
    return (c[:, 0] >= 0) & (c[:, 0] < 0xFFFF) & (np.abs(c[:, 1:]) <= lim).all(1)


# ------------------------------------------------------------------------------------------------ generators
def _rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _cells(rng, n, lo, hi):
    """n distinct (x, y, z) int rows of the box lo <= c < hi, in random order."""
    lo, hi = np.asarray(lo), np.asarray(hi)
    ext = hi - lo
    flat = rng.choice(int(ext.prod()), n, replace=False)
    x, r = np.divmod(flat, ext[1] * ext[2])
    y, z = np.divmod(r, ext[2])
    return np.stack([x, y, z], 1) + lo


@functools.lru_cache(maxsize=None)
def big_cloud():
    """N_BIG unique rows in four scenes, thin slabs (x, y in [-300, 300), z in [-3, 3)), shuffled: level 0 is above 2^20 rows (1028
    scan blocks, the last one partial, two chunks of block sums), level 1 below it with the grid still sized for level 0, and the
    deeper levels shrink the way a room does.  Negative coordinates throughout."""
    rng = _rng("big_cloud")
    per = [N_BIG // 4 + (1 if b < N_BIG % 4 else 0) for b in range(4)]
    rows = [np.concatenate([np.full((m, 1), b), _cells(rng, m, (-300, -300, -3), (300, 300, 3))], 1) for b, m in enumerate(per)]
    c = np.concatenate(rows).astype(np.int32)
    c = c[rng.permutation(c.shape[0])]
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def big_duplicates():
    """N_DUP rows drawn with replacement from 300 000 distinct rows: three chunks of block sums, most flags zero."""
    rng = _rng("big_duplicates")
    half = N_DUP_DISTINCT // 2
    pool = np.concatenate([np.concatenate([np.full((half, 1), b), _cells(rng, half, (-120, -120, -8), (120, 120, 8))], 1)
                           for b in range(2)]).astype(np.int32)
    c = pool[rng.integers(0, pool.shape[0], N_DUP)]
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def legacy_cloud():
    """The largest shape the suite fed the unique pipeline before: about 800 k rows (782 scan blocks, one chunk), with duplicates."""
    rng = _rng("legacy_cloud")
    pool = np.concatenate([np.full((500000, 1), 0), _cells(rng, 500000, (-150, -150, -10), (150, 150, 10))], 1).astype(np.int32)
    c = pool[rng.integers(0, pool.shape[0], 800000)]
    c.setflags(write=False)
    return c


def boundary_cloud(n, last):
    """n rows in two scenes, about a third of them duplicates, negative coordinates included.  last = "first": the last row and every
    row at an index 1024 j are first occurrences; last = "dup": they repeat row 0 (n = 1 has only "first")."""
    assert last in ("first", "dup") and (n > 1 or last == "first")
    rng = _rng("boundary", n, last)
    u = max(1, n - n // 3)
    pool = np.concatenate([rng.integers(0, 2, (u + 8, 1)), _cells(rng, u + 8, (-40, -40, -40), (40, 40, 40))], 1).astype(np.int32)
    idx = np.concatenate([np.arange(u), rng.integers(0, u, n - u)])
    idx[1:] = idx[1:][rng.permutation(n - 1)]                          # row 0 stays pool row 0
    marks = sorted(set(range(SCAN_BLOCK, n, SCAN_BLOCK)) | ({n - 1} if n > 1 else set()))
    for j, i in enumerate(marks):
        idx[i] = u + j if last == "first" else 0                     # pool rows u .. u + 7 occur nowhere else
    return pool[idx]


def boundary_cases():
    return [(n, last) for n in BOUNDARY_SIZES for last in ("first", "dup") if n > 1 or last == "first"]


@functools.lru_cache(maxsize=None)
def range_cloud():
    """540 voxels: 27 clusters -- one per face, edge and corner of the documented cube |c| <= 32766 and one interior -- in scene 0 and
    in scene 65534.  A cluster is its anchor and, along each axis, three more voxels 1, 2 and 3 cells inward, so it holds real
    neighbours at distance 1, 2 and 3 along each axis; after stride-2 quantisation at distance 2 and 4."""
    inner = (100, -201, 302)
    rows = []
    for b in (0, BATCH_MAX):
        for sx in (-1, 0, 1):
            for sy in (-1, 0, 1):
                for sz in (-1, 0, 1):
                    s = np.array([sx, sy, sz])
                    anchor = np.where(s != 0, s * DOC_LIM, inner)
                    step = np.where(s != 0, -s, 1)
                    pts = [anchor] + [anchor + d * step * np.eye(3, dtype=np.int64)[a] for a in range(3) for d in (1, 2, 3)]
                    rows += [np.concatenate([[b], p]) for p in pts]
    c = np.array(rows, dtype=np.int32)
    c = c[_rng("range_cloud").permutation(c.shape[0])]
    assert np.unique(c, axis=0).shape[0] == c.shape[0] == 540
    c.setflags(write=False)
    return c


def range_raises():
    """(name, rows, strides that must raise).  A row at |c| = 32768 in any column, a row stride quantisation pushes there
    (floor(-32767 / 2) * 2 = -32768), a row of scene 65535."""
    base = np.array([[0, 1, 2, 3], [1, -4, 5, -6], [2, 7, -8, 9]], dtype=np.int32)
    out = []
    for col in (1, 2, 3):
        for v in (32768, -32768):
            c = base.copy()
            c[1, col] = v
            out.append(("c%d=%d" % (col, v), c, (1, 2)))
        c = base.copy()
        c[2, col] = -32767
        out.append(("c%d=-32767 at stride 2" % col, c, (2,)))
    c = base.copy()
    c[0, 0] = 65535
    out.append(("batch=65535", c, (1, 2)))
    return out


def wrap_cloud(cap=1024):
    """Rows whose hash cluster wraps in a table of `cap` slots (cap = osn_hash_capacity(n) of the returned n rows):
      * 14 rows whose home slot is one of the last three: at least eleven of them spill past slot 0;
      * 8 rows homed in slots 1 .. 7, which the wrapped keys displace;
      * ordinary rows up to n = 3 cap / 8, none of them homed in the last 64 slots.
    No row is homed in slot 0 and slot cap - 4 stays empty, so in EVERY insertion order slot cap - 1 and slot 0 end up with keys
    homed at >= cap - 3 (a key only moves forward from its home, and cannot pass an empty slot).  The set of occupied slots of a
    linear-probing table does not depend on the insertion order either; which key sits where does.
    -> rows, home [n], occupied bool [cap] and keys uint64 [cap] of a sequential insert."""
    assert cap >= 1024 and cap & (cap - 1) == 0
    rng = _rng("wrap_cloud", cap)
    n = 3 * cap // 8
    m = max(200000, 400 * cap)
    side = int(np.ceil((m / 2) ** (1 / 3))) + 1
    pool = np.concatenate([np.concatenate([np.full((side ** 3, 1), b), _cells(rng, side ** 3, (-(side // 2),) * 3, (side - side // 2,) * 3)], 1)
                           for b in range(2)]).astype(np.int32)
    home = home_slot(pool, cap)
    tail = np.nonzero(home >= cap - 3)[0][:14]
    head = np.nonzero((home >= 1) & (home <= 7))[0][:8]
    rest = np.nonzero((home >= 8) & (home < cap - 64))[0][:n - 22]
    assert tail.size == 14 and head.size == 8 and rest.size == n - 22 and hash_capacity(n) == cap
    pick = np.concatenate([tail, head, rest])
    pick = pick[rng.permutation(pick.size)]
    rows = pool[pick]
    t = ModelTable.insert(pack_key(rows), cap)
    return types.SimpleNamespace(rows=rows, home=home[pick], occupied=t.keys != KEY_EMPTY, keys=t.keys, cap=cap)


# ------------------------------------------------------------------------------------------------ the model
def model_scan(flags, mutant=None):
    """exclusive_scan_i32_dev: scan_block_kernel (1024 elements per block, block sums), scan_sums_kernel (one workgroup, the block
    sums in chunks of 1024 with a carry), scan_add_kernel.  -> (exclusive scan, total)."""
    v = np.asarray(flags).astype(np.int64)
    n = v.shape[0]
    nb = max(1, -(-n // SCAN_BLOCK))
    pad = np.zeros(nb * SCAN_BLOCK, np.int64)
    pad[:n] = v
    blk = pad.reshape(nb, SCAN_BLOCK)
    local = np.cumsum(blk, 1) - blk
    sums = blk.sum(1)
    if mutant == "scan_block_edge":                    # the element at 1024 j belongs to block j - 1's sum, not to block j: only out[1024 j] moves
        edge = blk[1:, 0].copy()
        sums[:-1] += edge
        sums[1:] -= edge
        local[1:, 1:] -= edge[:, None]
    offs = np.zeros(nb, np.int64)
    carry = 0
    for ci, b0 in enumerate(range(0, nb, SCAN_CHUNK)):
        s = sums[b0:b0 + SCAN_CHUNK]
        use = carry
        if mutant == "scan_carry_lost" or (mutant == "scan_carry_once" and ci != 1):
            use = 0
        offs[b0:b0 + SCAN_CHUNK] = use + np.cumsum(s) - s
        carry = use + int(s.sum())
    total = carry
    if mutant == "scan_total_without_last_block":
        total = int(offs[-1])
    return (local + offs[:, None]).reshape(-1)[:n], total


def quantise(c4, stride, mutant=None):
    c = np.asarray(c4).astype(np.int64).copy()
    if stride > 1:
        if mutant == "floor_div_truncates":
            c[:, 1:] = np.trunc(c[:, 1:] / stride).astype(np.int64) * stride
        else:
            c[:, 1:] = np.floor_divide(c[:, 1:], stride) * stride
    return c


class ModelTable:
    """keys uint64 [cap] / vals int32 [cap], open addressing with linear probing, as common.h reads it."""
    PROBE_MAX = 1 << 16             # above this many rows the table is a sorted key list (the probe sequence is not what those cases test)

    def __init__(self, keys, vals, cap, sorted_keys=None, sorted_vals=None):
        self.keys, self.vals, self.cap, self.sorted_keys, self.sorted_vals = keys, vals, cap, sorted_keys, sorted_vals

    @classmethod
    def insert(cls, ukeys, cap):
        """hash_insert_kernel, one row after the other: the distinct keys `ukeys` in this order; value = position in ukeys."""
        keys = np.full(cap, KEY_EMPTY, np.uint64)
        vals = np.full(cap, VAL_EMPTY, np.int32)
        home = hash_key(ukeys) & (cap - 1)
        for j in range(ukeys.shape[0]):
            s = int(home[j])
            while keys[s] != KEY_EMPTY:
                s = (s + 1) & (cap - 1)
            keys[s], vals[s] = ukeys[j], j
        return cls(keys, vals, cap)

    @classmethod
    def build(cls, ukeys, cap):
        if ukeys.shape[0] <= cls.PROBE_MAX:
            return cls.insert(ukeys, cap)
        order = np.argsort(ukeys, kind="stable")
        return cls(None, None, cap, ukeys[order], order.astype(np.int32))

    def find(self, q, mutant=None):
        """table_find for every key of q -> value or -1."""
        q = np.asarray(q, dtype=np.uint64)
        res = np.full(q.shape[0], -1, np.int32)
        if self.keys is None:
            pos = np.minimum(np.searchsorted(self.sorted_keys, q), self.sorted_keys.shape[0] - 1)
            hit = self.sorted_keys[pos] == q
            res[hit] = self.sorted_vals[pos[hit]]
            return res
        slot = hash_key(q) & (self.cap - 1)
        live = np.arange(q.shape[0])
        while live.size:
            k = self.keys[slot[live]]
            hit = k == q[live]
            res[live[hit]] = self.vals[slot[live[hit]]]
            go = ~hit & (k != KEY_EMPTY)
            live = live[go]
            nxt = slot[live] + 1
            if mutant == "probe_no_wrap":
                live, nxt = live[nxt < self.cap], nxt[nxt < self.cap]       # a probe that reaches cap reports a miss
            slot[live] = nxt & (self.cap - 1)
        return res


def model_unique(coords4, stride=1, mutant=None):
    """queue_unique: quantise, range check, insert (the table keeps the lowest row of a key), flag the first occurrences, scan, emit,
    renumber.  -> (unique rows int32, inverse int32, first int32, ModelTable); ModelRangeError where the kernels set their flag."""
    n = np.asarray(coords4).shape[0]
    if n == 0:
        return np.zeros((0, 4), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), ModelTable.build(np.zeros(0, np.uint64), 1024)
    q = quantise(coords4, stride, mutant)
    if not in_range(q, LIM + 1 if mutant == "range_inclusive_off_by_one" else LIM).all():
        raise ModelRangeError("coordinate outside the packable range")
    key = pack_key(q)
    ukeys, head_of, inv = np.unique(key, return_index=True, return_inverse=True)
    head = head_of[inv.reshape(-1)]                                      # lowest row holding this row's key (atomicMin)
    flag = head == np.arange(n)
    rank, total = model_scan(flag, mutant)
    out = np.full((n + 2, 4), -1, np.int64)
    first = np.full(n + 2, -1, np.int64)
    rows = np.nonzero(flag)[0]
    out[np.minimum(rank[rows], n + 1)] = q[rows]
    first[np.minimum(rank[rows], n + 1)] = rows
    t = ModelTable.build(key[rows], hash_capacity(n))                    # keys in first-occurrence order ...
    ranks = rank[rows].astype(np.int32)                                  # ... renumbered to the unique row number
    if t.keys is None:
        t.sorted_vals = ranks[t.sorted_vals]
    else:
        occ = t.keys != KEY_EMPTY
        t.vals[occ] = ranks[t.vals[occ]]
    return out[:total].astype(np.int32), rank[head].astype(np.int32), first[:total].astype(np.int32), t


def model_pyramid(coords4, strides=(1, 2, 4, 8, 16), mutant=None):
    res, cur = [], coords4
    for s in strides:
        r = model_unique(cur, s, mutant)
        res.append(r)
        cur = r[0]
    return res


def model_kmap_build(table, out_coords4, ksize, scale, mutant=None):
    """kmap_build_kernel -> (nbr int32 [K, n_out], counts int64 [K]); offsets with x fastest, odd kernels centred, even ones [0, k)."""
    lim = LIM + 1 if mutant == "range_inclusive_off_by_one" else LIM
    out = np.asarray(out_coords4).astype(np.int64)
    K = ksize ** 3
    c = ksize // 2 if ksize & 1 else 0
    nbr = np.full((K, out.shape[0]), -1, np.int32)
    for k in range(K):
        off = np.array([0, k % ksize - c, (k // ksize) % ksize - c, k // (ksize * ksize) - c]) * scale
        p = out + off
        ok = (np.abs(p[:, 1:]) <= lim).all(1)
        nbr[k, ok] = table.find(pack_key(p[ok]), mutant)
    return nbr, (nbr >= 0).sum(1).astype(np.int64)


def model_kmap_sort(nbr, counts=None, mutant=None):
    """osn_kmap_sort -> (order int32, table in that order, group masks int32)."""
    nbr = np.asarray(nbr)
    K, n = nbr.shape
    bitpos = np.arange(K)
    if counts is not None and mutant != "mask_bit_order":
        c = np.asarray(counts).astype(np.int64)
        j, k = np.meshgrid(np.arange(K), np.arange(K))                   # bitpos[k] = offsets in front of k: more pairs, or as many and a lower index
        bitpos = ((j != k) & ((c[j] > c[k]) | ((c[j] == c[k]) & (j < k)))).sum(1)
    occ = (nbr >= 0).astype(np.int64)
    key = (occ << bitpos.reshape(K, 1)).sum(0)
    if mutant == "sort_unstable":
        order = (n - 1 - np.argsort(key[::-1], kind="stable")).astype(np.int32)
    else:
        order = np.argsort(key, kind="stable").astype(np.int32)
    srt = nbr[:, order]
    mask = ((srt >= 0).astype(np.int64) << np.arange(K).reshape(K, 1)).sum(0)
    pad = np.zeros((-n) % 32, np.int64)
    gmask = np.bitwise_or.reduce(np.concatenate([mask, pad]).reshape(-1, 32), 1)
    return order, np.ascontiguousarray(srt), gmask.astype(np.uint32).view(np.int32)


# ------------------------------------------------------------------------------------------------ the range reference
def probe_out_of_range(out_coords4, ksize, scale):
    """bool [K, n_out]: the probe of offset k at row o has a component outside [-32767, 32767]."""
    off = oc.kernel_offsets(ksize, scale).astype(np.int64)
    p = np.asarray(out_coords4).astype(np.int64)[None, :, 1:] + off[:, None, :]
    return (np.abs(p) > LIM).any(2)


def masked_kernel_map(in_coords4, out_coords4, ksize, scale):
    """oracle.coords.kernel_map with every probe that leaves [-32767, 32767] a miss (module docstring: the oracle's pack would alias)."""
    nbr = oc.kernel_map(np.asarray(in_coords4), np.asarray(out_coords4), oc.kernel_offsets(ksize, scale)).copy()
    nbr[probe_out_of_range(out_coords4, ksize, scale)] = -1
    return nbr


def synthetic_table(K, n, fill, seed):
    """A neighbour table of random occupancy: entry = some input row where occupied, else -1."""
    rng = _rng("synthetic_table", K, n, seed)
    t = rng.integers(0, n, (K, n), dtype=np.int32)
    t[rng.random((K, n), dtype=np.float32) >= fill] = -1
    return t
