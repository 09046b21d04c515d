"""Tensor-level wrappers over the C ABI: allocate outputs / scratch with torch,
pass raw device pointers and the current HIP stream.  No autograd here (see
functional.py) and no CPU fallback."""
import collections
import ctypes
import os
import threading
import weakref

import torch

from . import _lib
from ._lib import check

_vp = ctypes.c_void_p

# Optional launch profiler (bench.py): an object with start(kind, dev, **meta) -> token and
# stop(token); brackets the C-ABI call with HIP events on the stream the kernels run on.
_profiler = None


def set_profiler(p):
    global _profiler
    _profiler = p


# Host-side cost matters: a training step is ~1200 launches and the deep U-Net levels run kernels of a few
# microseconds, so every microsecond spent here is a microsecond the GPU may sit idle
# (tools/host_profile.py measures this layer against a mock library).  Hence raw ints instead of
# ctypes / torch.cuda.Stream objects and one raw-stream query per helper.
_raw_stream_of = torch._C._cuda_getCurrentRawStream      # device index -> current hipStream_t as int
_current_device = torch._C._cuda_getDevice


def _prof_start(kind, dev, **meta):
    # the profiler brackets torch's current stream: launches redirected by on_stream() are not bracketed
    if _profiler is None or getattr(_tls, "stream", None) is not None:
        return None
    return _profiler.start(kind, dev, **meta)


def _p(t):
    return t.data_ptr() if t is not None else None       # ctypes converts the int to void* (argtypes are set)


def _idx(dev):
    i = dev.index
    return i if i is not None else _current_device()


_tls = threading.local()


def _stream(dev):
    s = getattr(_tls, "stream", None)
    return s if s is not None else _raw_stream_of(_idx(dev))


class on_stream:
    """Context: the C-ABI calls of this thread launch on `stream` (a torch.cuda.Stream) instead of torch's current
    stream -- without touching torch's stream state, so tensors are still allocated from the current stream's pool.
    The caller orders the two streams (functional.py forks / joins around the weight gradient)."""
    __slots__ = ("raw", "prev", "torch_stream", "prev_torch")

    def __init__(self, stream):
        self.raw = stream.cuda_stream
        self.torch_stream = stream

    def __enter__(self):
        self.prev = getattr(_tls, "stream", None)
        self.prev_torch = getattr(_tls, "torch_stream", None)
        _tls.stream = self.raw
        _tls.torch_stream = self.torch_stream

    def __exit__(self, *a):
        _tls.stream = self.prev
        _tls.torch_stream = self.prev_torch


_side_streams = {}


def side_stream(dev):
    """One auxiliary HIP stream per device (created on first use), default priority.  (The weight gradients queued here crowd
    the main stream's memory-bound kernels; a LOW-priority stream was measured twice -- round 3, and round 5 with the executor,
    profiles/r05_s1_knobs_ab.txt -- as no change: the hardware's priorities do not pre-empt resident workgroups.)"""
    i = _idx(dev)
    s = _side_streams.get(i)
    if s is None:
        s = torch.cuda.Stream(device=i)
        _side_streams[i] = s
    return s


_aux_streams = {}


def aux_stream(dev):
    """The THIRD stream of the process (per device, high priority, created on first use): the map prefetcher's stream, and the third
    lane of an inference pass's map build.  The library never creates a fourth: the process is held to three hardware queues
    (openscene_amd.configure_hw_queues), and a stream beyond them shares a queue with one that matters (round 6: two extra map
    streams moved a LATER prefetcher onto the main stream's queue and the scene-stream inference went from 2.85 to 4.85 ms per scene)."""
    i = _idx(dev)
    s = _aux_streams.get(i)
    if s is None:
        _lo, hi = torch.cuda.Stream.priority_range()
        s = _aux_streams[i] = torch.cuda.Stream(device=i, priority=hi)
    return s


# Scratch for the C-ABI calls: ONE growing buffer per (device, stream).  Every call's scratch is only
# live while that call's kernels run, and calls on one stream execute in order (autograd's backward
# thread launches on the same stream), so sharing is safe and saves a torch.empty per launch.
_ws_pool = {}


def _ws(nbytes, dev):
    return ws_on(nbytes, dev, _stream(dev))


def ws_on(nbytes, dev, raw_stream):
    """The growing scratch buffer of (device, the given raw stream) -- for launches a C call places on another stream."""
    nbytes = max(int(nbytes), 16)
    key = (_idx(dev), raw_stream)
    buf = _ws_pool.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=dev)
        _ws_pool[key] = buf
    return buf


_size_cache = {}


def _cached(fn_name, *args):
    """ws-size / plan helpers are pure functions of their integer arguments: memoise the ctypes call."""
    key = (fn_name,) + args
    v = _size_cache.get(key)
    if v is None:
        v = getattr(_lib.load(), fn_name)(*args)
        _size_cache[key] = v
    return v


_dev_ok = {}


def _prep(dev):
    if dev not in _dev_ok:
        _lib.require_device(dev)          # raises for CPU tensors / other architectures
        _dev_ok[dev] = True
    return _lib.load()


class _Dev:
    """Make `dev` the current HIP device for the duration of a call if it is not already."""
    __slots__ = ("ctx",)

    def __init__(self, dev):
        idx = dev.index
        self.ctx = None if (idx is None or idx == _current_device()) else torch.cuda.device(idx)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def _f32c(t, name):
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (got %s)" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _query_feats(t, name):
    """Query features: float32 (network output) or float16 (fused 2-D features as the reference stores them,
    scripts/feature_fusion/fusion_util.py:87).  The kernel reads fp32 rows; an fp16 matrix is widened once here
    (half -> float -> half is the identity, so `feats.half() @ text` is unchanged; costs one pass over it)."""
    if t.dtype == torch.float16:
        t = t.float()
    return _f32c(t, name)


# ----------------------------------------------------------------- coordinates
class HashTable:
    """Open-addressing table keys[cap] u64 / vals[cap] i32 living in HBM."""
    __slots__ = ("keys", "vals", "cap")

    def __init__(self, n, dev):
        self.cap = int(_lib.load().osn_hash_capacity(int(n)))
        self.keys = torch.empty(self.cap, dtype=torch.int64, device=dev)
        self.vals = torch.empty(self.cap, dtype=torch.int32, device=dev)


def coords_unique(coords4, stride=1):
    """-> (unique coords [U,4] int32 in first-occurrence order, inverse [N] int32,
    first [U] int32, HashTable mapping packed key -> unique row)."""
    if coords4.dtype != torch.int32 or coords4.dim() != 2 or coords4.shape[1] != 4:
        raise TypeError("coordinates must be int32 [N, 4] rows (batch, x, y, z)")
    dev = coords4.device
    lib = _prep(dev)
    coords4 = coords4.contiguous()
    n = coords4.shape[0]
    table = HashTable(n, dev)
    out = torch.empty((max(n, 1), 4), dtype=torch.int32, device=dev)
    inverse = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    first = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    wsb = _cached("osn_coords_unique_ws_bytes", n)
    ws = _ws(wsb, dev)
    nu = ctypes.c_int64(0)
    with _Dev(dev):
        check(lib.osn_coords_unique(_p(coords4), n, int(stride), _p(table.keys), _p(table.vals), table.cap,
                                    _p(out), _p(inverse), _p(first), ctypes.byref(nu), _p(ws), ws.numel(),
                                    _stream(dev)), "osn_coords_unique")
    u = int(nu.value)
    return out[:u], inverse[:n], first[:u], table


def coords_pyramid(coords4, strides=(1, 2, 4, 8, 16)):
    """coords_unique for a chain of strides (level i is the unique set of level i-1 quantised to strides[i]) with ONE
    host synchronisation for the whole chain instead of one per level: every level is queued with its row count still
    in device memory (osn_coords_unique_async) and sized for the input's row count; the counts come back together.
    -> [(coords [U_i, 4], inverse [U_{i-1}] (parent map), first [U_i], HashTable)] -- the tuples coords_unique returns."""
    if coords4.dtype != torch.int32 or coords4.dim() != 2 or coords4.shape[1] != 4:
        raise TypeError("coordinates must be int32 [N, 4] rows (batch, x, y, z)")
    n0 = coords4.shape[0]
    if n0 == 0 or len(strides) == 1:
        res, cur = [], coords4
        for s in strides:
            r = coords_unique(cur, s)
            res.append(r)
            cur = r[0]
        return res
    dev = coords4.device
    lib = _prep(dev)
    coords4 = coords4.contiguous()
    L = len(strides)
    counts = torch.empty(L + 1, dtype=torch.int32, device=dev)        # [0 .. L-1] unique rows per level, [L] range error (zeroed by the call)
    ws = _ws(_cached("osn_coords_unique_ws_bytes", n0), dev)
    st = _stream(dev)
    bufs = []
    for _ in strides:
        bufs.append((torch.empty((n0, 4), dtype=torch.int32, device=dev), torch.empty(n0, dtype=torch.int32, device=dev),
                     torch.empty(n0, dtype=torch.int32, device=dev), HashTable(n0, dev)))
    arr = lambda ts: (ctypes.c_void_p * L)(*[t.data_ptr() for t in ts])
    with _Dev(dev):
        # one call, one preset launch for every table (round 6; was one osn_coords_unique_async per level)
        check(lib.osn_coords_pyramid_async(_p(coords4), n0, (ctypes.c_int32 * L)(*[int(s) for s in strides]), L,
                                           arr([b[3].keys for b in bufs]), arr([b[3].vals for b in bufs]), bufs[0][3].cap,
                                           arr([b[0] for b in bufs]), arr([b[1] for b in bufs]), arr([b[2] for b in bufs]),
                                           _p(counts), _p(ws), ws.numel(), st), "osn_coords_pyramid_async")
    host = counts.tolist()                                             # the one synchronisation
    if host[L]:
        raise _lib.OpenSceneAmdError("osn_coords_pyramid_async: coordinate outside the packable range "
                                     "(|x|,|y|,|z| < 32767, 0 <= batch < 65535)")
    res, u_prev = [], n0
    for (out, inverse, first, table), u in zip(bufs, host[:L]):
        res.append((out[:u], inverse[:u_prev], first[:u], table))
        u_prev = u
    return res


def kmap_build(table, out_coords4, ksize, offset_scale, with_counts=False, self_map=False):
    """nbr int32 [K, n_out] (and, with_counts, int64 [K] pairs per offset from the same pass).  self_map: out_coords4 are
    the rows the table was built from, in row order, and ksize is odd (stride-1 convolution): the half-probe builder."""
    dev = out_coords4.device
    lib = _prep(dev)
    out_coords4 = out_coords4.contiguous()
    n_out = out_coords4.shape[0]
    K = ksize ** 3
    nbr = torch.empty((K, n_out), dtype=torch.int32, device=dev)
    counts = torch.empty(K, dtype=torch.int64, device=dev) if with_counts else None
    fn, what = (lib.osn_kmap_build_self, "osn_kmap_build_self") if (self_map and ksize % 2 == 1) else \
        (lib.osn_kmap_build, "osn_kmap_build")
    with _Dev(dev):
        check(fn(_p(table.keys), _p(table.vals), table.cap, _p(out_coords4), n_out, int(ksize),
                 int(offset_scale), _p(nbr), _p(counts), _stream(dev)), what)
    return (nbr, counts) if with_counts else nbr


def kmap_transpose(nbr, n_in):
    dev = nbr.device
    lib = _prep(dev)
    K, n_out = nbr.shape
    tbl = torch.empty((K, int(n_in)), dtype=torch.int32, device=dev)
    with _Dev(dev):
        check(lib.osn_kmap_transpose(_p(nbr), n_out, K, int(n_in), _p(tbl), _stream(dev)), "osn_kmap_transpose")
    return tbl


def kmap_sort(nbr, counts=None):
    """-> (order int32 [n_out], nbr_sorted int32 [K, n_out], gmask int32 [ceil(n_out/32)]): rows ordered by
    offset-occupancy mask (key bits ordered by rarity when the per-offset pair `counts` are given);
    gmask = OR of the masks (bit k = offset k) of each 32-row group of the sorted table."""
    dev = nbr.device
    lib = _prep(dev)
    nbr = nbr.contiguous()
    K, n_out = nbr.shape
    order = torch.empty(n_out, dtype=torch.int32, device=dev)
    out = torch.empty_like(nbr)
    gmask = torch.empty((n_out + 31) // 32, dtype=torch.int32, device=dev)
    with _Dev(dev):
        wsb = _cached("osn_kmap_sort_ws_bytes", n_out)
        ws = _ws(wsb, dev)
        check(lib.osn_kmap_sort(_p(nbr), n_out, K, _p(counts), _p(order), _p(out), _p(gmask), _p(ws), ws.numel(),
                                _stream(dev)), "osn_kmap_sort")
    return order, out, gmask


def kmap_count(nbr):
    dev = nbr.device
    lib = _prep(dev)
    K, n_out = nbr.shape
    counts = torch.empty(K, dtype=torch.int64, device=dev)
    with _Dev(dev):
        check(lib.osn_kmap_count(_p(nbr), n_out, K, _p(counts), _stream(dev)), "osn_kmap_count")
    return counts


# ------------------------------------------------- every kernel map of a scene from one call, on several streams
_MAP_LEVEL = None
_MAP_JOB = None
_map_events = {}
# streams the jobs of one maps_build call are dealt to.  Measured on MI355X (profiles/r03_s5..s7): 2 - 4 streams do not
# shorten the step (12.5 - 12.7 ms either way: the 5^3 stem map is the long pole and the first thing the forward pass
# needs), and every extra stream counts against the runtime's four hardware queues -- with the executor's side stream
# and the input prefetcher's stream in flight as well, streams start to share queues and the step DOUBLES (26 ms).
MAPS_STREAMS = int(os.environ.get("OSN_MAPS_STREAMS", "1"))        # 1 = everything on the caller's stream


def _map_dtypes():
    global _MAP_LEVEL, _MAP_JOB
    if _MAP_LEVEL is None:
        import numpy as np
        _MAP_LEVEL = np.dtype([("coords4", "<u8"), ("keys", "<u8"), ("vals", "<u8"), ("cap", "<i8"), ("rows", "<i8")])
        _MAP_JOB = np.dtype([(n, "<i4") for n in ("lvl_in", "lvl_out", "ksize", "scale", "self_map", "stream", "bm_fwd", "bm_bwd")] +
                            [(n, "<u8") for n in ("nbr_fwd", "nbr_bwd", "counts", "order_fwd", "sorted_fwd", "gmask_fwd", "order_bwd",
                                                  "sorted_bwd", "gmask_bwd", "tl_fwd", "tl_bwd", "pl_fwd")])
        assert _MAP_LEVEL.itemsize == 40 and _MAP_JOB.itemsize == 128
    return _MAP_LEVEL, _MAP_JOB


def _addr(v):
    return 0 if v is None else (int(v) if isinstance(v, int) else v.data_ptr())


def maps_build(levels, jobs, dev, sort_rows, streams=None, occ=None):
    """levels: [(coords4, HashTable, rows)]; jobs: list of dicts with the fields of osn_map_job (tensors, device addresses
    or None for the pointers, `stream` = 0 .. MAPS_STREAMS - 1); sort_rows: rows of the largest table that gets tile-ordered (scratch
    size).  One C call; the maps of different levels run side by side on MAPS_STREAMS streams (fork / join inside).
    occ: per level a buffer of maps_occupancy_bytes(rows) bytes (tensor, device address) or None -- the level's 3^3 / 5^3 self maps
    then probe occupied cells only (osn_maps_build_occ)."""
    import numpy as np
    lib = _prep(dev)
    ldt, jdt = _map_dtypes()
    la = np.zeros(len(levels), dtype=ldt)
    for i, (c, t, rows) in enumerate(levels):
        la[i] = (c.data_ptr(), t.keys.data_ptr(), t.vals.data_ptr(), t.cap, rows)
    ja = np.zeros(max(len(jobs), 1), dtype=jdt)
    for i, q in enumerate(jobs):
        ja[i] = tuple((_addr(q.get(n)) if jdt[n].kind == "u" else int(q.get(n, 0))) for n in jdt.names)
    ns = max(1, min(int(streams) if streams else MAPS_STREAMS, 3))      # (streams: the caller's choice -- the executor's inference pass)
    idx = _idx(dev)
    main = _stream(dev)
    raws = [main]
    if ns > 1:
        # lanes 1, 2: the two auxiliary streams the process has anyway (the executor's side stream, the prefetcher's) -- never new ones
        pool = [s for s in (side_stream(dev), aux_stream(dev)) if s.cuda_stream != main]
        ns = min(ns, 1 + len(pool))
        raws += [s.cuda_stream for s in pool[:ns - 1]]
        ev = _map_events.get(idx)
        if ev is None:
            with _Dev(dev):
                ev = _map_events[idx] = lib.osn_events_create(8)
        if not ev:
            ns, raws, ev = 1, [main], None
    else:
        ev = None
    wsb = int(_cached("osn_kmap_sort_ws_bytes", int(sort_rows))) if sort_rows else 256
    wss = [_ws(wsb, dev)] + [ws_on(wsb, dev, r) for r in raws[1:]]
    st_arr = (ctypes.c_void_p * ns)(*raws)
    ws_arr = (ctypes.c_void_p * ns)(*[w.data_ptr() for w in wss])
    wb_arr = (ctypes.c_uint64 * ns)(*[w.numel() for w in wss])
    occ_arr = (ctypes.c_void_p * len(levels))(*[_addr(o) or None for o in occ]) if occ is not None else None
    with _Dev(dev):
        check(lib.osn_maps_build_occ(la.ctypes.data, len(levels), ja.ctypes.data, len(jobs), st_arr, ws_arr, wb_arr, ns, ev, occ_arr),
              "osn_maps_build")


def maps_occupancy_bytes(rows):
    """Bytes of a level's block-occupancy buffer (maps_build's occ)."""
    return int(_cached("osn_maps_occupancy_bytes", int(rows)))


def maps_set_legacy(on):
    """Tests and A/B: run the kernel-map launches of the earlier rounds (every self map probed, the pair lists' work items planned
    by a launch of their own), process-wide; every product is bitwise the same.  Returns the previous setting."""
    return bool(_lib.load().osn_maps_set_legacy(int(bool(on))))


# ----------------------------------------------------------------- convolution
def _w3(weight):
    return weight.unsqueeze(0) if weight.dim() == 2 else weight


def _table_conv(kind, lib, feats, wptr, nbr, n_out, out_rows, gmask, K, cin, cout):
    """What both table kernels share: table check, output, workspace, profiler bracket and the call of osn_<kind>."""
    dev = feats.device
    if nbr is not None:
        if nbr.dtype != torch.int32 or nbr.shape != (K, n_out):
            raise ValueError("nbr must be int32 [%d, %d], got %s %s" % (K, n_out, nbr.dtype, tuple(nbr.shape)))
        nbr = nbr.contiguous()
    elif K != 1 or feats.shape[0] != n_out:
        raise ValueError("nbr=None is the identity map and needs K == 1 and n_in == n_out")
    out = torch.empty((n_out, cout), dtype=torch.float32, device=dev)
    wsb = _cached("osn_spconv_fwd_ws_bytes", n_out, K, cin, cout)
    ws = _ws(wsb, dev) if wsb else None
    tok = _prof_start(kind, dev, n_in=feats.shape[0], n_out=n_out, K=K, cin=cin, cout=cout)
    with _Dev(dev):
        check(getattr(lib, "osn_" + kind)(_p(feats), wptr, _p(nbr), _p(out_rows), _p(gmask), _p(out), n_out, K, cin, cout,
                                          _p(ws), int(wsb), _stream(dev)), "osn_" + kind)
    if tok is not None:
        _profiler.stop(tok)
    return out


def spconv_fwd(feats, weight, nbr, n_out, out_rows=None, gmask=None):
    """out[o] = sum_k feats[nbr[k,o]] @ weight[k].  nbr None <=> K == 1 identity map.
    (out_rows, gmask) come with a tile-ordered table from kmap_sort."""
    lib = _prep(feats.device)
    feats = _f32c(feats, "features")
    w = _f32c(_w3(weight), "weight")
    K, cin, cout = w.shape
    if feats.shape[1] != cin:
        raise ValueError("features have %d channels, kernel expects %d" % (feats.shape[1], cin))
    return _table_conv("spconv_fwd", lib, feats, _p(w), nbr, n_out, out_rows, gmask, K, cin, cout)


def weight_prep_x6(weight, flip=False, for_dgrad=False):
    """bf16 [3, K, n, c_pad] pre-split weights for spconv_fwd_x6 (n = output channels of the conv that will run)."""
    dev = weight.device
    lib = _prep(dev)
    w = _f32c(_w3(weight), "weight")
    K, cin, cout = w.shape
    nn, nc = (cin, cout) if for_dgrad else (cout, cin)
    cp = (nc + 31) // 32 * 32
    wp = torch.empty((3, K, nn, cp), dtype=torch.bfloat16, device=dev)
    with _Dev(dev):
        check(lib.osn_weight_prep_x6(_p(w), K, cin, cout, int(bool(flip)), int(bool(for_dgrad)), _p(wp), _stream(dev)),
              "osn_weight_prep_x6")
    return wp


def weight_prep_x6_pair(weight, flip=False):
    """(forward planes, input-gradient planes) of one weight from a single launch."""
    dev = weight.device
    lib = _prep(dev)
    w = _f32c(_w3(weight), "weight")
    K, cin, cout = w.shape
    wf = torch.empty((3, K, cout, (cin + 31) // 32 * 32), dtype=torch.bfloat16, device=dev)
    wb = torch.empty((3, K, cin, (cout + 31) // 32 * 32), dtype=torch.bfloat16, device=dev)
    with _Dev(dev):
        check(lib.osn_weight_prep_x6_pair(_p(w), K, cin, cout, int(bool(flip)), _p(wf), _p(wb), _stream(dev)),
              "osn_weight_prep_x6_pair")
    return wf, wb


def spconv_fwd_x6(feats, wp, nbr, n_out, out_rows=None, gmask=None):
    """Split-bf16 convolution: out[o] = sum_k feats[nbr[k,o]] @ B[k], B given as weight_prep_x6 planes."""
    lib = _prep(feats.device)
    feats = _f32c(feats, "features")
    _three, K, cout, cp = wp.shape
    cin = feats.shape[1]
    if (cin + 31) // 32 * 32 != cp:
        raise ValueError("features have %d channels, prepared weights expect <= %d" % (cin, cp))
    return _table_conv("spconv_fwd_x6", lib, feats, _p(wp), nbr, n_out, out_rows, gmask, K, cin, cout)


# ------------------------------------------------- second-generation convolution (tile lists)
class TileLists:
    """Per-tile compacted pair lists of one neighbour table (osn_tile_lists_build): `buf` holds
    cnt int32 [n_tiles, K] and lst int2 [n_tiles, K, bm]; `out_rows` is the row permutation of a
    tile-ordered table (None = table rows are tensor rows)."""
    __slots__ = ("buf", "bm", "n_out", "K", "out_rows", "pairs")

    def __init__(self, buf, bm, n_out, K, out_rows):
        self.buf, self.bm, self.n_out, self.K, self.out_rows = buf, bm, n_out, K, out_rows
        self.pairs = None                  # per-offset pair arrays for the weight gradient, built on first use

    @property
    def n_tiles(self):
        return -(-self.n_out // self.bm)

    def counts(self):
        """int32 [n_tiles, K] view of the pair counts."""
        return self.buf[:self.n_tiles * self.K * 4].view(torch.int32).view(self.n_tiles, self.K)

    def lists(self):
        """int32 [n_tiles, K, bm, 2] view: (input row, local output row); only the first cnt entries are defined."""
        off = (self.n_tiles * self.K * 4 + 255) // 256 * 256
        return self.buf[off:off + self.n_tiles * self.K * self.bm * 8].view(torch.int32).view(self.n_tiles, self.K, self.bm, 2)


def tile_rows(n_out):
    return int(_cached("osn_tile_rows", int(n_out)))


def tile_lists(nbr, out_rows=None, bm=None):
    """TileLists of an int32 [K, n_out] table (rows possibly tile-ordered; then pass its `out_rows`)."""
    dev = nbr.device
    lib = _prep(dev)
    nbr = nbr.contiguous()
    K, n_out = nbr.shape
    bm = tile_rows(n_out) if bm is None else int(bm)
    nbytes = int(_cached("osn_tile_lists_bytes", n_out, K, bm))
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with _Dev(dev):
        check(lib.osn_tile_lists_build(_p(nbr), n_out, K, bm, _p(buf), _stream(dev)), "osn_tile_lists_build")
    return TileLists(buf, bm, n_out, K, out_rows)


def tl_eligible(K, cin, cout, n_in=0):
    """Shapes the tile-list kernel takes (everything of the U-Net but the 3-channel stem; up to 2^24 input rows; up to 512
    input channels = four 128-channel chunks in the kernel's step table: wider 1x1 convs are the dense kernel's)."""
    return bool(_cached("osn_spconv_fwd_tl_ok", int(n_in), int(K), int(cin), int(cout)))


def weight_prep_tl(weight, flip=False, want_fwd=True, want_dgrad=True):
    """(forward image, input-gradient image) of one weight, MFMA-fragment layout, one launch."""
    dev = weight.device
    lib = _prep(dev)
    w = _f32c(_w3(weight), "weight")
    K, cin, cout = w.shape
    wf = torch.empty(_cached("osn_weight_prep_tl_bytes", K, cin, cout, 0), dtype=torch.uint8, device=dev) if want_fwd else None
    wb = torch.empty(_cached("osn_weight_prep_tl_bytes", K, cin, cout, 1), dtype=torch.uint8, device=dev) if want_dgrad else None
    with _Dev(dev):
        check(lib.osn_weight_prep_tl(_p(w), K, cin, cout, int(bool(flip)), _p(wf), _p(wb), _stream(dev)),
              "osn_weight_prep_tl")
    return wf, wb


# ------------------------------------------------- weight images of model parameters: one launch per optimizer step
# A convolution weight that is an nn.Parameter keeps its images (forward / input gradient, plane or fragment layout)
# between calls, keyed on the parameter's version counter: an optimizer step bumps every version, the first
# convolution of the next forward then refreshes ALL images of the device in one osn_weight_prep_batch launch (the job
# table lives in device memory and is reused while the set of stale images is the same); in eval mode nothing is
# launched.  Anything that changes a parameter without bumping its version (writes through `.data` / raw pointers)
# must call clear_weight_cache().  OSN_WEIGHT_CACHE=0 switches the cache off (one prep launch per convolution).
WEIGHT_CACHE = os.environ.get("OSN_WEIGHT_CACHE", "1") != "0"
PREP_X6, PREP_TL = 0, 1


class _Image:
    __slots__ = ("ref", "ptr", "version", "image", "K", "cin", "cout", "flip", "for_dgrad", "layout", "blocks")


class _WeightImages:
    def __init__(self):
        self.entries = {}          # (id(param), flip, for_dgrad, layout) -> _Image
        self.table = None          # (tuple of entry keys, job table on the device, total blocks)
        self.keep = []             # recent job tables (their launches may still be queued)
        self.lock = threading.Lock()


_weight_images = {}


WEIGHT_CACHE_GENERATION = 0          # moves when the cache is emptied (the executor's descriptor cache keys on it)


def clear_weight_cache():
    global WEIGHT_CACHE_GENERATION
    WEIGHT_CACHE_GENERATION += 1
    _weight_images.clear()


def _alloc_image(K, cin, cout, for_dgrad, layout, dev):
    if layout == PREP_TL:
        return torch.empty(_cached("osn_weight_prep_tl_bytes", K, cin, cout, int(for_dgrad)), dtype=torch.uint8, device=dev)
    nn, nc = (cin, cout) if for_dgrad else (cout, cin)
    return torch.empty((3, K, nn, (nc + 31) // 32 * 32), dtype=torch.bfloat16, device=dev)


def _refresh_images(imgs, lib, dev):
    import numpy as np
    stale, keys = [], []
    for key, e in list(imgs.entries.items()):
        p = e.ref()
        if p is None:
            del imgs.entries[key]
            continue
        if e.version != p._version or e.ptr != p.data_ptr():
            stale.append((e, p))
            keys.append(key)
    if not stale:
        return
    keys = tuple(keys)
    tbl = imgs.table
    if tbl is None or tbl[0] != keys or any(e.ptr != p.data_ptr() for e, p in stale):
        jobs = np.zeros(len(stale), dtype=[("W", "<u8"), ("out", "<u8"), ("first", "<i8"), ("K", "<i4"), ("cin", "<i4"),
                                           ("cout", "<i4"), ("flip", "<i4"), ("dg", "<i4"), ("layout", "<i4")])
        first = 0
        for i, (e, p) in enumerate(stale):
            e.ptr = p.data_ptr()
            jobs[i] = (e.ptr, e.image.data_ptr(), first, e.K, e.cin, e.cout, e.flip, e.for_dgrad, e.layout)
            first += e.blocks
        # (under ops.on_stream the launch below goes to that stream: the table's upload has to be in ITS past, not in torch's
        # current stream's)
        ts = getattr(_tls, "torch_stream", None)
        if ts is not None:
            with torch.cuda.stream(ts):
                tbl = (keys, torch.from_numpy(jobs.view(np.uint8)).to(dev), first)
        else:
            tbl = (keys, torch.from_numpy(jobs.view(np.uint8)).to(dev), first)
        imgs.table = tbl
        imgs.keep = (imgs.keep + [tbl[1]])[-8:]
    with _Dev(dev):
        check(lib.osn_weight_prep_batch(_p(tbl[1]), len(stale), tbl[2], _stream(dev)), "osn_weight_prep_batch")
    for e, p in stale:
        e.version = p._version


def weight_image(weight, flip=False, for_dgrad=False, layout=PREP_X6):
    """Image of `weight` for spconv_fwd_x6 (layout PREP_X6) or spconv_fwd_tl (PREP_TL); for_dgrad: the image the input
    gradient multiplies with (transposed, offsets mirrored if flip).  Parameters are served from the per-device cache
    (see above), other tensors are prepared on the spot."""
    flip, for_dgrad = bool(flip), bool(for_dgrad)
    cacheable = (WEIGHT_CACHE and isinstance(weight, torch.nn.Parameter) and weight.dtype == torch.float32
                 and weight.is_contiguous())
    if not cacheable:
        if layout == PREP_TL:
            wf, wb = weight_prep_tl(weight, flip, want_fwd=not for_dgrad, want_dgrad=for_dgrad)
            return wb if for_dgrad else wf
        return weight_prep_x6(weight, flip=flip, for_dgrad=for_dgrad)
    dev = weight.device
    lib = _prep(dev)
    imgs = _weight_images.get(dev)
    if imgs is None:
        imgs = _weight_images[dev] = _WeightImages()
    key = (id(weight), flip, for_dgrad, layout)
    with imgs.lock:
        e = imgs.entries.get(key)
        if e is None or e.ref() is not weight:
            K, cin, cout = _w3(weight).shape
            e = _Image()
            e.ref, e.ptr, e.version = weakref.ref(weight), 0, -1
            e.K, e.cin, e.cout, e.flip, e.for_dgrad, e.layout = K, cin, cout, int(flip), int(for_dgrad), layout
            e.blocks = _cached("osn_weight_prep_job_blocks", K, cin, cout, int(for_dgrad), layout)
            e.image = _alloc_image(K, cin, cout, for_dgrad, layout, dev)
            imgs.entries[key] = e
        if e.version != weight._version or e.ptr != weight.data_ptr():
            _refresh_images(imgs, lib, dev)
        return e.image


_tl_counters = {}


def tl_counters(dev):
    """The 128 persistent tile counters of (device, current stream): zero once, the tile-list kernel leaves them zero."""
    ck = (_idx(dev), _stream(dev))
    c = _tl_counters.get(ck)
    if c is None:
        c = _tl_counters[ck] = torch.zeros(128, dtype=torch.int32, device=dev)
    return c


def _pieces_ok(pieces):
    """pieces = 3: the six-product arithmetic through the entry it always went through; 2 / 1: the reduced inference modes
    (openscene_amd.precision, csrc/split.h) through the entry's `_pieces` sibling."""
    if pieces not in (1, 2, 3):
        raise ValueError("pieces must be 1, 2 or 3, got %r" % (pieces,))
    return int(pieces)


def spconv_fwd_tl(feats, wp, tl, n_out, K, cout, bn_partial=None, pieces=3):
    """out[o] = sum_k feats[list rows] @ B[k] with B given as a weight_prep_tl image; tl None <=> K == 1 identity.
    bn_partial: optional float64 [n_tiles, 2, cout] receiving per-tile column sums / sums of squares.
    pieces: operand pieces (_pieces_ok)."""
    pieces = _pieces_ok(pieces)
    dev = feats.device
    lib = _prep(dev)
    feats = _f32c(feats, "features")
    cin = feats.shape[1]
    if tl is not None:
        if tl.n_out != n_out or tl.K != K:
            raise ValueError("tile lists are for a [%d, %d] table, conv wants [%d, %d]" % (tl.K, tl.n_out, K, n_out))
        bm, buf, rows = tl.bm, tl.buf, tl.out_rows
    else:
        if K != 1 or feats.shape[0] != n_out:
            raise ValueError("tl=None is the identity map and needs K == 1 and n_in == n_out")
        bm, buf, rows = tile_rows(n_out), None, None
    need = _cached("osn_weight_prep_tl_bytes", K, cin, cout, 0)
    if wp.numel() != need:
        raise ValueError("prepared weight has %d bytes, a [%d, %d, %d] conv needs %d" % (wp.numel(), K, cin, cout, need))
    out = torch.empty((n_out, cout), dtype=torch.float32, device=dev)
    ws = _ws(_cached("osn_spconv_fwd_tl_ws_bytes", n_out, K if tl is not None else 1, cout, bm), dev)
    tok = _prof_start("spconv_fwd_tl", dev, n_in=feats.shape[0], n_out=n_out, K=K, cin=cin, cout=cout)
    counters = tl_counters(dev)
    with _Dev(dev):
        try:
            args = (_p(feats), feats.shape[0], _p(wp), _p(buf), _p(rows), _p(out), _p(bn_partial), n_out, K, cin, cout, bm, _p(ws),
                    ws.numel(), _p(counters), _stream(dev))
            if pieces == 3:
                check(lib.osn_spconv_fwd_tl(*args), "osn_spconv_fwd_tl")
            else:
                check(lib.osn_spconv_fwd_tl_pieces(*args, pieces), "osn_spconv_fwd_tl_pieces")
        except Exception:
            _tl_counters.pop((_idx(dev), _stream(dev)), None)   # a failed launch leaves the counters undefined: start from a fresh zero buffer
            raise
    if tok is not None:
        _profiler.stop(tok)
    return out


def pair_lists(tl):
    """Per-offset pair arrays + weight-gradient work items of a TileLists (built once, cached on it)."""
    if tl.pairs is None:
        dev = tl.buf.device
        lib = _prep(dev)
        nbytes = int(_cached("osn_pair_lists_bytes", tl.n_out, tl.K, tl.bm))
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with _Dev(dev):
            check(lib.osn_pair_lists_build(_p(tl.buf), _p(tl.out_rows), tl.n_out, tl.K, tl.bm, _p(buf), _stream(dev)),
                  "osn_pair_lists_build")
        tl.pairs = buf
    return tl.pairs


def pair_arrays(tl):
    """(poff int32 [K+1], pin int32 [P], pout int32 [P]) host-readable views of pair_lists(tl) (tests / tools)."""
    buf = pair_lists(tl)
    poff = buf[:(tl.K + 1) * 4].view(torch.int32)
    cap = tl.K * max(tl.n_out, 1)
    P = int(poff[tl.K])
    pin = buf[16384:16384 + cap * 4].view(torch.int32)[:P]
    pout = buf[16384 + cap * 4:16384 + 2 * cap * 4].view(torch.int32)[:P]
    return poff, pin, pout


def spconv_wgrad_tl(feats, gout, tl, K, swap=False, pieces=3):
    """gW [K, cin, cout] from the pair arrays of `tl` (None <=> K == 1 identity).  swap: `tl` belongs to the strided
    convolution that this transposed convolution mirrors.  pieces: operand pieces (_pieces_ok; below 3: the reduced training modes)."""
    pieces = _pieces_ok(pieces)
    dev = feats.device
    lib = _prep(dev)
    feats = _f32c(feats, "features")
    gout = _f32c(gout, "grad_output")
    n_in, cin = feats.shape
    n_out, cout = gout.shape
    if tl is not None:
        table_rows = n_in if swap else n_out
        if tl.K != K or tl.n_out != table_rows:
            raise ValueError("pair lists are for a [%d, %d] table, the weight gradient wants [%d, %d]" % (
                tl.K, tl.n_out, K, table_rows))
        pl = pair_lists(tl)
    else:
        if K != 1 or n_in != n_out:
            raise ValueError("tl=None is the identity map and needs K == 1 and n_in == n_out")
        pl = None
    gw = torch.empty((K, cin, cout), dtype=torch.float32, device=dev)
    wsb = _cached("osn_spconv_wgrad_tl_ws_bytes", K, cin, cout)
    ws = _ws(wsb, dev)
    tok = _prof_start("spconv_wgrad_tl", dev, n_in=n_in, n_out=n_out, K=K, cin=cin, cout=cout)
    with _Dev(dev):
        args = (_p(feats), _p(gout), _p(pl), int(bool(swap)), _p(gw), n_in, n_out, K, cin, cout, _p(ws), ws.numel(), _stream(dev))
        if pieces == 3:
            check(lib.osn_spconv_wgrad_tl(*args), "osn_spconv_wgrad_tl")
        else:
            check(lib.osn_spconv_wgrad_tl_pieces(*args, pieces), "osn_spconv_wgrad_tl_pieces")
    if tok is not None:
        _profiler.stop(tok)
    return gw


def rows_argmax(scores, gather=None):
    """int64 labels [len(gather) or N] = argmax over the columns of float32 `scores` [N, c] (a column slice of a wider
    contiguous matrix is fine), row gather[p] for point p: argmax + point -> voxel gather in one launch."""
    dev = scores.device
    lib = _prep(dev)
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1:
        raise ValueError("scores must be a float32 matrix with unit column stride")
    n, c = scores.shape
    ld = scores.stride(0) if n > 1 else max(c, scores.stride(0))
    if gather is not None:
        if gather.dtype != torch.int64 or gather.device != dev:
            raise ValueError("gather must be an int64 vector on the scores' device")
        gather = gather.contiguous()
    n_pts = n if gather is None else gather.shape[0]
    labels = torch.empty(n_pts, dtype=torch.int64, device=dev)
    with _Dev(dev):
        check(lib.osn_rows_argmax(_p(scores), ld, c, _p(gather), n_pts, n, _p(labels), _stream(dev)), "osn_rows_argmax")
    return labels


def dense_eligible(cin, cout):
    """Shapes the 1x1-convolution kernel takes (everything of the U-Net family; odd widths stay on the generic kernel)."""
    return bool(_cached("osn_dense_fwd_ok", int(cin), int(cout)))


def dense_fwd(feats, wp, cout, pieces=3):
    """out = feats @ B, B a weight_prep_tl image of a K = 1 weight (forward image, or the input-gradient image).
    pieces: operand pieces (_pieces_ok)."""
    pieces = _pieces_ok(pieces)
    dev = feats.device
    lib = _prep(dev)
    feats = _f32c(feats, "features")
    n, cin = feats.shape
    need = _cached("osn_weight_prep_tl_bytes", 1, cin, cout, 0)
    if wp.numel() != need:
        raise ValueError("prepared weight has %d bytes, a [%d, %d] 1x1 conv needs %d" % (wp.numel(), cin, cout, need))
    out = torch.empty((n, cout), dtype=torch.float32, device=dev)
    tok = _prof_start("dense_fwd", dev, n_in=n, n_out=n, K=1, cin=cin, cout=cout)
    with _Dev(dev):
        if pieces == 3:
            check(lib.osn_dense_fwd(_p(feats), _p(wp), _p(out), n, cin, cout, _stream(dev)), "osn_dense_fwd")
        else:
            check(lib.osn_dense_fwd_pieces(_p(feats), _p(wp), _p(out), n, cin, cout, _stream(dev), pieces), "osn_dense_fwd_pieces")
    if tok is not None:
        _profiler.stop(tok)
    return out


def stem_conv_wgrad(feats, gout, nbr, K):
    """gW [K, cin, 32] of the stem convolution (stem_eligible shapes) from the plain neighbour table."""
    dev = feats.device
    lib = _prep(dev)
    feats = _f32c(feats, "features")
    gout = _f32c(gout, "grad_output")
    cin, (n_out, cout) = feats.shape[1], gout.shape
    if nbr.dtype != torch.int32 or tuple(nbr.shape) != (K, n_out):
        raise ValueError("nbr must be int32 [%d, %d], got %s %s" % (K, n_out, nbr.dtype, tuple(nbr.shape)))
    gw = torch.empty((K, cin, cout), dtype=torch.float32, device=dev)
    ws = _ws(_cached("osn_stem_conv_wgrad_ws_bytes", K, cin), dev)
    tok = _prof_start("stem_wgrad", dev, n_in=feats.shape[0], n_out=n_out, K=K, cin=cin, cout=cout)
    with _Dev(dev):
        check(lib.osn_stem_conv_wgrad(_p(feats), _p(gout), _p(nbr.contiguous()), _p(gw), n_out, K, cin, cout, _p(ws), ws.numel(),
                                      _stream(dev)), "osn_stem_conv_wgrad")
    if tok is not None:
        _profiler.stop(tok)
    return gw


def spconv_fwd_ws(feats, wp, tl, nbr_dst, n_dst, K, cout, swap=False, direct=False, pieces=3):
    """Convolution of a small map from the pair arrays of `tl` (weight-stationary workgroups + ordered sum over the
    offsets): out[r] = sum_k feats[src of (k, r)] @ B[k], B a weight_prep_tl image.  nbr_dst int32 [K, n_dst]: the
    neighbour table of the destination side, plain row order.  swap: `tl` belongs to the map's transposed direction.
    direct: every destination row has exactly one pair in the map (fine side of a 2^3 stride-2 map): rows are written
    straight to the output, nbr_dst may be None.  pieces: operand pieces (_pieces_ok)."""
    pieces = _pieces_ok(pieces)
    dev = feats.device
    lib = _prep(dev)
    feats = _f32c(feats, "features")
    n_in, cin = feats.shape
    table_rows = n_in if swap else n_dst
    if tl.K != K or tl.n_out != table_rows:
        raise ValueError("pair lists are for a [%d, %d] table, the convolution wants [%d, %d]" % (tl.K, tl.n_out, K, table_rows))
    if not (direct and nbr_dst is None) and (nbr_dst.dtype != torch.int32 or tuple(nbr_dst.shape) != (K, n_dst)):
        raise ValueError("nbr_dst must be int32 [%d, %d], got %s %s" % (K, n_dst, nbr_dst.dtype, tuple(nbr_dst.shape)))
    need = _cached("osn_weight_prep_tl_bytes", K, cin, cout, 0)
    if wp.numel() != need:
        raise ValueError("prepared weight has %d bytes, a [%d, %d, %d] conv needs %d" % (wp.numel(), K, cin, cout, need))
    pl = pair_lists(tl)
    out = torch.empty((n_dst, cout), dtype=torch.float32, device=dev)
    ws = _ws(_cached("osn_spconv_fwd_ws_ws_bytes", n_dst, K, cout, int(bool(direct))), dev)
    tok = _prof_start("spconv_fwd_ws", dev, n_in=n_in, n_out=n_dst, K=K, cin=cin, cout=cout)
    with _Dev(dev):
        args = (_p(feats), n_in, _p(wp), _p(pl), table_rows, int(bool(swap)), int(bool(direct)),
                _p(nbr_dst.contiguous() if nbr_dst is not None else None), _p(out), n_dst, K, cin, cout, _p(ws), ws.numel(), _stream(dev))
        if pieces == 3:
            check(lib.osn_spconv_fwd_ws(*args), "osn_spconv_fwd_ws")
        else:
            check(lib.osn_spconv_fwd_ws_pieces(*args, pieces), "osn_spconv_fwd_ws_pieces")
    if tok is not None:
        _profiler.stop(tok)
    return out


def rg_eligible(K, cin, cout, n_in):
    """Shapes the register-gather kernel takes (csrc/spconv_rg.hip): 32 / 64 channels on both sides, K > 1."""
    return bool(_cached("osn_spconv_fwd_rg_ok", int(max(n_in, 1)), int(K), int(cin), int(cout)))


def spconv_fwd_rg(feats, wp, nbr, n_out, cout, out_rows=None, pieces=3):
    """out[o] = sum_k feats[nbr[k, o]] @ B[k], B given as a weight_prep_tl image (forward or input-gradient image); nbr plain or
    tile-ordered (then out_rows = its permutation).  pieces: operand pieces (_pieces_ok)."""
    pieces = _pieces_ok(pieces)
    dev = feats.device
    lib = _prep(dev)
    feats = _f32c(feats, "features")
    nbr = nbr.contiguous()
    K = nbr.shape[0]
    if nbr.shape[1] != n_out:
        raise ValueError("table is [%d, %d], conv wants %d output rows" % (K, nbr.shape[1], n_out))
    out = torch.empty((n_out, cout), dtype=torch.float32, device=dev)
    with _Dev(dev):
        args = (_p(feats), feats.shape[0], _p(wp), _p(nbr), _p(out_rows), _p(out), n_out, K, feats.shape[1], cout, _stream(dev))
        if pieces == 3:
            check(lib.osn_spconv_fwd_rg(*args), "osn_spconv_fwd_rg")
        else:
            check(lib.osn_spconv_fwd_rg_pieces(*args, pieces), "osn_spconv_fwd_rg_pieces")
    return out


def stem_eligible(K, cin, cout):
    """The dedicated kernels of the U-Net's 3-channel stem conv (any conv with <= 4 input and 32 output channels)."""
    return bool(_cached("osn_stem_conv_ok", int(K), int(cin), int(cout)))


def stem_conv_fwd(feats, weight, nbr, n_out):
    dev = feats.device
    lib = _prep(dev)
    feats = _f32c(feats, "features")
    w = _f32c(_w3(weight), "weight")
    K, cin, cout = w.shape
    if nbr.dtype != torch.int32 or nbr.shape != (K, n_out):
        raise ValueError("nbr must be int32 [%d, %d], got %s %s" % (K, n_out, nbr.dtype, tuple(nbr.shape)))
    out = torch.empty((n_out, cout), dtype=torch.float32, device=dev)
    tok = _prof_start("stem_fwd", dev, n_in=feats.shape[0], n_out=n_out, K=K, cin=cin, cout=cout)
    with _Dev(dev):
        check(lib.osn_stem_conv_fwd(_p(feats), _p(w), _p(nbr.contiguous()), _p(out), n_out, K, cin, cout, _stream(dev)),
              "osn_stem_conv_fwd")
    if tok is not None:
        _profiler.stop(tok)
    return out


def x6_eligible(K, cin, cout, n_out):
    """The split-bf16 kernel handles every conv of the U-Net except the 3-channel stem."""
    return bool(_cached("osn_spconv_fwd_x6_ok", int(n_out), int(K), int(cin), int(cout)))


def weight_transpose(weight, flip):
    dev = weight.device
    lib = _prep(dev)
    w = _f32c(_w3(weight), "weight")
    K, cin, cout = w.shape
    wt = torch.empty((K, cout, cin), dtype=torch.float32, device=dev)
    with _Dev(dev):
        check(lib.osn_weight_transpose(_p(w), K, cin, cout, int(bool(flip)), _p(wt), _stream(dev)),
              "osn_weight_transpose")
    return wt


_wgrad_items = {}      # id(counts tensor of a map) -> (weakref to it, {items_bytes: work-item table})


def _wgrad_plan_items(lib, counts, n_out, K, cin, cout, dev):
    """Work-item table of a map, built once per (map, table size) and shared by every conv on that map."""
    nbytes = _cached("osn_spconv_wgrad_items_bytes", n_out, K, cin, cout)
    key = id(counts)
    hit = _wgrad_items.get(key)
    if hit is None or hit[0]() is not counts:
        # entry dies with the map's counts tensor (tensors compare elementwise, so no WeakKeyDictionary)
        hit = _wgrad_items[key] = (weakref.ref(counts, lambda _r, k=key: _wgrad_items.pop(k, None)), {})
    per_map = hit[1]
    # a transposed conv shares its counts tensor with the strided conv it mirrors but has another n_out
    sub = (int(n_out), int(K), int(cin), int(cout))         # the plan depends on the channel tiling, not only on its size
    items = per_map.get(sub)
    if items is None:
        items = per_map[sub] = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        with _Dev(dev):
            check(lib.osn_spconv_wgrad_plan(_p(counts), n_out, K, cin, cout, _p(items), _stream(dev)),
                  "osn_spconv_wgrad_plan")
    return items


def spconv_wgrad(feats, gout, nbr, K, counts=None):
    dev = feats.device
    lib = _prep(dev)
    feats = _f32c(feats, "features")
    gout = _f32c(gout, "grad_output")
    n_out, cout = gout.shape
    cin = feats.shape[1]
    if nbr is not None:
        nbr = nbr.contiguous()
        if nbr.shape != (K, n_out):
            raise ValueError("nbr shape %s does not match (K=%d, n_out=%d)" % (tuple(nbr.shape), K, n_out))
    gw = torch.empty((K, cin, cout), dtype=torch.float32, device=dev)
    wsb = _cached("osn_spconv_wgrad_ws_bytes", n_out, K, cin, cout)
    ws = _ws(wsb, dev) if wsb else None
    tok = _prof_start("spconv_wgrad", dev, n_in=feats.shape[0], n_out=n_out, K=K, cin=cin, cout=cout)
    items = _wgrad_plan_items(lib, counts, n_out, K, cin, cout, dev) if (counts is not None and n_out > 0) else None
    with _Dev(dev):
        check(lib.osn_spconv_wgrad(_p(feats), _p(gout), _p(nbr), _p(counts), _p(items), _p(gw), n_out, K, cin, cout,
                                   _p(ws), int(wsb), _stream(dev)), "osn_spconv_wgrad")
    if tok is not None:
        _profiler.stop(tok)
    return gw


_plan_cache = {}


def spconv_fwd_plan(n_out, K, cin, cout):
    """(WM, WN, TN, BK, S, workgroups) of the kernel instance osn_spconv_fwd picks."""
    key = (int(n_out), int(K), int(cin), int(cout))
    v = _plan_cache.get(key)
    if v is None:
        plan = (ctypes.c_int32 * 6)()
        check(_lib.load().osn_spconv_fwd_plan(key[0], key[1], key[2], key[3], plan), "osn_spconv_fwd_plan")
        v = _plan_cache[key] = tuple(plan)
    return v


# ------------------------------------------------------------------ batch norm
def bn_stats(x, running_mean=None, running_var=None, momentum=0.1):
    dev = x.device
    lib = _prep(dev)
    x = _f32c(x, "x")
    n, c = x.shape
    mean = torch.empty(c, dtype=torch.float32, device=dev)
    var = torch.empty(c, dtype=torch.float32, device=dev)
    wsb = _cached("osn_bn_ws_bytes", n, c)
    ws = _ws(wsb, dev)
    with _Dev(dev):
        check(lib.osn_bn_stats(_p(x), n, c, _p(mean), _p(var), _p(running_mean), _p(running_var), float(momentum),
                               _p(ws), ws.numel(), _stream(dev)), "osn_bn_stats")
    return mean, var


def _bn_fwd_args(x, residual):
    """(x, residual, n, c) of a forward pass: contiguous float32, the residual (or None) shaped like x."""
    x = _f32c(x, "x")
    if residual is not None:
        residual = _f32c(residual, "residual")
        if residual.shape != x.shape:
            raise ValueError("residual shape %s != %s" % (tuple(residual.shape), tuple(x.shape)))
    return x, residual, x.shape[0], x.shape[1]


def bn_apply(x, mean, var, gamma, beta, eps, residual=None, relu=False, y2=None, out=None):
    """y2: a second destination (a [n, c] column window of a wider matrix: ME.cat written in place by its producer), or None.
    out: a caller's destination (contiguous float32 shaped like x; x itself normalises in place: every element is read before it
    is written), or None for a new tensor.  -> y"""
    dev = x.device
    lib = _prep(dev)
    x, residual, n, c = _bn_fwd_args(x, residual)
    if out is not None and (out.dtype != torch.float32 or out.shape != x.shape or out.device != dev or not out.is_contiguous()):
        raise ValueError("out must be a contiguous float32 tensor shaped like x, on its device")
    p2, ld2 = _row_view(y2, c, "y2") if y2 is not None else (None, 0)
    y = out if out is not None else torch.empty_like(x)
    with _Dev(dev):
        check(lib.osn_bn_apply(_p(x), _p(mean), _p(var), _p(gamma), _p(beta), float(eps), _p(residual), int(bool(relu)),
                               _p(y), p2, ld2, n, c, _stream(dev)), "osn_bn_apply")
    return y


def bn_forward_train(x, gamma, beta, eps, residual, relu, running_mean, running_var, momentum, y2=None):
    """(y, mean, var): batch statistics (running buffers updated in place) + normalise (+ residual) (+ ReLU), one C call.
    y2: a second destination as in bn_apply, or None."""
    dev = x.device
    lib = _prep(dev)
    x, residual, n, c = _bn_fwd_args(x, residual)
    p2, ld2 = _row_view(y2, c, "y2") if y2 is not None else (None, 0)
    mv = torch.empty((2, c), dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    ws = _ws(_cached("osn_bn_ws_bytes", n, c), dev)
    with _Dev(dev):
        check(lib.osn_bn_forward_train(_p(x), n, c, _p(gamma), _p(beta), float(eps), _p(residual), int(bool(relu)),
                                       float(momentum), _p(mv[0]), _p(mv[1]), _p(running_mean), _p(running_var), _p(y), p2, ld2,
                                       _p(ws), ws.numel(), _stream(dev)), "osn_bn_forward_train")
    return y, mv[0], mv[1]


# The names these two had while y2 / out were separate wrappers (the C entries behind them are gone): same functions, same
# argument order, so that code written against them keeps running.  New code uses the plain names.
bn_apply2 = bn_apply
bn_forward_train2 = bn_forward_train


def bn_backward(x, y, gy, mean, var, gamma, eps, relu, training, want_gres, beta=None):
    """beta given and y None (batch norm + ReLU without a residual): the ReLU mask is recomputed from x, y is not read."""
    return bn_backward_multi(x, y, [_f32c(gy, "grad_output")], mean, var, gamma, eps, relu, training, want_gres, beta=beta)


def _row_view(t, c, name):
    """(pointer, row stride in floats) of a float32 [n, c] matrix that may be a column window of a wider one."""
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != c or (t.shape[0] > 1 and t.stride(1) != 1):
        raise TypeError("%s must be a float32 [n, %d] matrix with unit column stride" % (name, c))
    ld = t.stride(0) if t.shape[0] > 1 else max(c, t.stride(0))
    if ld % 4 or t.data_ptr() % 16:
        raise ValueError("%s: row stride and first element must be 16-byte aligned" % name)
    return t.data_ptr(), ld


def bn_backward_multi(x, y, gys, mean, var, gamma, eps, relu, training, want_gres, beta=None, gres_out=None):
    """bn_backward whose incoming gradient is the SUM of the matrices in `gys` (1 .. 3, each possibly a column window of a
    wider matrix): the sum is formed while reading.  y None with relu needs beta (mask recomputed from x; no residual).
    gres_out: a contiguous float32 [n, c] destination for gres (with want_gres) instead of a new tensor; it may be one of the
    contiguous sources itself (include/openscene_amd.h, osn_bn_backward: the aliasing rule)."""
    dev = x.device
    lib = _prep(dev)
    n, c = x.shape
    if relu and y is None and (beta is None or want_gres):
        raise ValueError("batch-norm backward with ReLU needs y, or beta and no residual")
    views = [_row_view(g, c, "grad_output[%d]" % i) for i, g in enumerate(gys)]
    ptrs = (ctypes.c_void_p * len(views))(*[v[0] for v in views])
    lds = (ctypes.c_int64 * len(views))(*[v[1] for v in views])
    gx = torch.empty_like(x)
    if gres_out is not None and (not want_gres or gres_out.dtype != torch.float32 or gres_out.shape != x.shape or
                                 gres_out.device != dev or not gres_out.is_contiguous()):
        raise ValueError("gres_out must be a contiguous float32 tensor shaped like x, on its device, and needs want_gres")
    gres = (gres_out if gres_out is not None else torch.empty_like(x)) if want_gres else None
    ggamma = torch.empty(c, dtype=torch.float32, device=dev)
    gbeta = torch.empty(c, dtype=torch.float32, device=dev)
    ws = _ws(_cached("osn_bn_ws_bytes", n, c), dev)
    with _Dev(dev):
        check(lib.osn_bn_backward(_p(x), _p(y), ptrs, lds, len(views), _p(mean), _p(var), _p(gamma),
                                  _p(beta) if (relu and y is None) else None, float(eps),
                                  int(bool(relu)), int(bool(training)), _p(gx), _p(gres), _p(ggamma), _p(gbeta), n, c,
                                  _p(ws), ws.numel(), _stream(dev)), "osn_bn_backward")
    return gx, gres, ggamma, gbeta


def bn_apply_plan(total4, c4):
    """(grid, flat) of the apply kernels' launch plan for total4 = n * c / 4 quads in c4 = c / 4 column quads (osn_bn_apply_plan:
    flat = the grid-stride kernels run because no grid near the wanted one keeps a thread on its columns).  Needs no device."""
    grid, flat = ctypes.c_int32(), ctypes.c_int32()
    check(_lib.load().osn_bn_apply_plan(int(total4), int(c4), ctypes.byref(grid), ctypes.byref(flat)), "osn_bn_apply_plan")
    return grid.value, bool(flat.value)


def bn_set_flat_kernels(on):
    """Tests and A/B: run the batch-norm kernels of the earlier rounds (flat apply kernels, one row in flight in the column sums),
    process-wide; results are bitwise the same.  Returns the previous setting."""
    return bool(_lib.load().osn_bn_set_flat_kernels(int(bool(on))))


def bn_set_separate_finalize(on):
    """Tests and A/B: keep the backward pass's finalize kernel a launch of its own on the small maps too (by default the apply pass
    of a map of at most 4096 rows, with batch statistics, adds the partial sums itself), process-wide; results are bitwise the same.
    Returns the previous setting."""
    return bool(_lib.load().osn_bn_set_separate_finalize(int(bool(on))))


# ------------------------------------------------------- elementwise (a11)
def relu_fwd(x):
    dev = x.device
    lib = _prep(dev)
    x = _f32c(x, "x")
    y = torch.empty_like(x)
    with _Dev(dev):
        check(lib.osn_relu_fwd(_p(x), _p(y), x.numel(), _stream(dev)), "osn_relu_fwd")
    return y


def relu_bwd(y, gy):
    dev = y.device
    lib = _prep(dev)
    gy = _f32c(gy, "grad_output")
    gx = torch.empty_like(y)
    with _Dev(dev):
        check(lib.osn_relu_bwd(_p(y), _p(gy), _p(gx), y.numel(), _stream(dev)), "osn_relu_bwd")
    return gx


def add(a, b):
    dev = a.device
    lib = _prep(dev)
    a, b = _f32c(a, "a"), _f32c(b, "b")
    if a.shape != b.shape:
        raise ValueError("add: shapes %s and %s differ" % (tuple(a.shape), tuple(b.shape)))
    out = torch.empty_like(a)
    with _Dev(dev):
        check(lib.osn_add(_p(a), _p(b), _p(out), a.numel(), _stream(dev)), "osn_add")
    return out


def cat2(a, b):
    """[n, ca] ++ [n, cb] -> [n, ca + cb] in one launch (channel counts multiples of 4)."""
    dev = a.device
    lib = _prep(dev)
    a, b = _f32c(a, "a"), _f32c(b, "b")
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0]:
        raise ValueError("cat2: need two [n, c] matrices with equal n")
    n, ca, cb = a.shape[0], a.shape[1], b.shape[1]
    out = torch.empty((n, ca + cb), dtype=torch.float32, device=dev)
    with _Dev(dev):
        check(lib.osn_cat2(_p(a), ca, _p(b), cb, _p(out), n, _stream(dev)), "osn_cat2")
    return out


def cat2_bwd(gout, ca, cb):
    dev = gout.device
    lib = _prep(dev)
    gout = _f32c(gout, "grad_output")
    n = gout.shape[0]
    ga = torch.empty((n, ca), dtype=torch.float32, device=dev)
    gb = torch.empty((n, cb), dtype=torch.float32, device=dev)
    with _Dev(dev):
        check(lib.osn_cat2_bwd(_p(gout), _p(ga), ca, _p(gb), cb, n, _stream(dev)), "osn_cat2_bwd")
    return ga, gb


# ----------------------------------------------------------------------- query
def cosine_query(feats, text_half, gather=None, want_scores=True):
    """(scores fp16 [n, C] or None, argmax int64 [n]) of feats[gather].half() @ text.t()."""
    dev = feats.device
    lib = _prep(dev)
    feats = _query_feats(feats, "features")
    if text_half.dtype != torch.float16:
        raise TypeError("text features must be float16 (util/util.py:41-44 produces fp16)")
    text_half = text_half.contiguous()
    c, d = text_half.shape
    if feats.shape[1] != d:
        raise ValueError("feature dim %d != text dim %d" % (feats.shape[1], d))
    if gather is not None:
        if gather.dtype != torch.int64:
            gather = gather.long()
        gather = gather.contiguous()
        n = gather.shape[0]
    else:
        n = feats.shape[0]
    scores = torch.empty((n, c), dtype=torch.float16, device=dev) if want_scores else None
    amax = torch.empty(n, dtype=torch.int64, device=dev)
    with _Dev(dev):
        check(lib.osn_cosine_query(_p(feats), _p(gather), _p(text_half), _p(scores), _p(amax), n, d, c, _stream(dev)),
              "osn_cosine_query")
    return scores, amax


def query_ensemble(feat_distill, feat_fusion, text_half, gather_distill=None, gather_fusion=None, want_scores=True):
    dev = feat_distill.device
    lib = _prep(dev)
    fd = _query_feats(feat_distill, "distill features")
    ff = _query_feats(feat_fusion, "fusion features")
    text_half = text_half.contiguous()
    c, d = text_half.shape

    def _g(g):
        if g is None:
            return None
        return (g if g.dtype == torch.int64 else g.long()).contiguous()

    gd, gf = _g(gather_distill), _g(gather_fusion)
    n = gd.shape[0] if gd is not None else fd.shape[0]
    nf = gf.shape[0] if gf is not None else ff.shape[0]
    if n != nf:
        raise ValueError("the two feature sources address %d vs %d points" % (n, nf))
    scores = torch.empty((n, c), dtype=torch.float16, device=dev) if want_scores else None
    amax = torch.empty(n, dtype=torch.int64, device=dev)
    sel = torch.empty(n, dtype=torch.uint8, device=dev)
    wsb = lib.osn_query_ensemble_ws_bytes(n)
    ws = _ws(wsb, dev)
    with _Dev(dev):
        check(lib.osn_query_ensemble(_p(fd), _p(gd), _p(ff), _p(gf), _p(text_half), _p(scores), _p(amax), _p(sel), n,
                                     d, c, _p(ws), ws.numel(), _stream(dev)), "osn_query_ensemble")
    return scores, amax, sel.bool()


def _vote_matrix(votes, n, c, dev):
    if (votes.dtype != torch.float16 or votes.dim() != 2 or tuple(votes.shape) != (n, c) or votes.device != dev
            or not votes.is_contiguous()):
        raise ValueError("votes must be a contiguous float16 [%d, %d] matrix on the features' device" % (n, c))
    if votes.data_ptr() % (16 if c % 8 == 0 else 2):
        raise ValueError("votes must start 16-byte aligned when the label count is a multiple of 8")


def cosine_query_vote(feats, text_half, votes, gather=None, want_labels=False):
    """votes [n, C] (fp16, in place) += feats[gather].half() @ text.t() with torch's CPU half rounding (fp32 add, one
    rounding): run/evaluate.py:397,416 `store = pred + store` fused into the query.  -> argmax int64 [n] of this call's
    scores, or None."""
    dev = feats.device
    lib = _prep(dev)
    feats = _query_feats(feats, "features")
    if text_half.dtype != torch.float16:
        raise TypeError("text features must be float16 (util/util.py:41-44 produces fp16)")
    text_half = text_half.contiguous()
    c, d = text_half.shape
    if feats.shape[1] != d:
        raise ValueError("feature dim %d != text dim %d" % (feats.shape[1], d))
    if gather is not None:
        gather = (gather if gather.dtype == torch.int64 else gather.long()).contiguous()
    n = gather.shape[0] if gather is not None else feats.shape[0]
    _vote_matrix(votes, n, c, dev)
    amax = torch.empty(n, dtype=torch.int64, device=dev) if want_labels else None
    with _Dev(dev):
        check(lib.osn_cosine_query_vote(_p(feats), _p(gather), _p(text_half), _p(votes), _p(amax), n, d, c, _stream(dev)),
              "osn_cosine_query_vote")
    return amax


def query_ensemble_vote(feat_distill, feat_fusion, text_half, votes, gather_distill=None, gather_fusion=None, want_labels=False):
    """query_ensemble with the vote epilogue: votes [n, C] += the selected source's fp16 scores.  -> (argmax or None,
    used_fusion bool [n])."""
    dev = feat_distill.device
    lib = _prep(dev)
    fd = _query_feats(feat_distill, "distill features")
    ff = _query_feats(feat_fusion, "fusion features")
    if text_half.dtype != torch.float16:
        raise TypeError("text features must be float16 (util/util.py:41-44 produces fp16)")
    text_half = text_half.contiguous()
    c, d = text_half.shape

    def _g(g):
        if g is None:
            return None
        return (g if g.dtype == torch.int64 else g.long()).contiguous()

    gd, gf = _g(gather_distill), _g(gather_fusion)
    n = gd.shape[0] if gd is not None else fd.shape[0]
    nf = gf.shape[0] if gf is not None else ff.shape[0]
    if n != nf:
        raise ValueError("the two feature sources address %d vs %d points" % (n, nf))
    _vote_matrix(votes, n, c, dev)
    amax = torch.empty(n, dtype=torch.int64, device=dev) if want_labels else None
    sel = torch.empty(n, dtype=torch.uint8, device=dev)
    ws = _ws(lib.osn_query_ensemble_ws_bytes(n), dev)
    with _Dev(dev):
        check(lib.osn_query_ensemble_vote(_p(fd), _p(gd), _p(ff), _p(gf), _p(text_half), _p(votes), _p(amax), _p(sel), n,
                                          d, c, _p(ws), ws.numel(), _stream(dev)), "osn_query_ensemble_vote")
    return amax, sel.bool()


def eval_confusion(labels, confusion, err, votes=None, ids=None, mapper=None, has_feature=None, hist=-1):
    """confusion int64 [C + 1, C] += the counts of (prediction, gt) over the points whose gt is not 255: prediction =
    Tensor.max(1)[1] of the fp16 `votes` [n, c_in] (or the int64 `ids` [n]), then mapper[prediction], then 256 where
    has_feature is False; row C counts the no-feature points.  `err` (int32 [1], device) collects bad mapper ids, gt and
    predictions without a synchronisation; eval_check raises on them.  hist: -1 auto (LDS up to 90 classes), 1 LDS histogram
    (up to 160 classes), 0 global atomics."""
    dev = labels.device
    lib = _prep(dev)
    if (votes is None) == (ids is None):
        raise ValueError("give exactly one of votes and ids")
    if labels.dtype != torch.int64 or labels.dim() != 1:
        raise ValueError("labels must be an int64 vector")
    labels = labels.contiguous()
    n = labels.shape[0]
    c_in = 0
    if votes is not None:
        if votes.dtype != torch.float16 or votes.dim() != 2 or votes.shape[0] != n or votes.device != dev:
            raise ValueError("votes must be a float16 [%d, c] matrix on the labels' device" % n)
        votes = votes.contiguous()
        c_in = votes.shape[1]
    else:
        if ids.dtype != torch.int64 or tuple(ids.shape) != (n,) or ids.device != dev:
            raise ValueError("ids must be an int64 vector of %d entries on the labels' device" % n)
        ids = ids.contiguous()
    n_map = 0
    if mapper is not None:
        if mapper.dtype != torch.int64 or mapper.dim() != 1 or mapper.device != dev:
            raise ValueError("mapper must be an int64 vector on the labels' device")
        mapper = mapper.contiguous()
        n_map = mapper.shape[0]
    if has_feature is not None:
        if has_feature.dim() != 1 or has_feature.shape[0] != n or has_feature.device != dev:
            raise ValueError("has_feature must be a vector of %d entries on the labels' device" % n)
        has_feature = has_feature.to(torch.uint8).contiguous()
    if (confusion.dtype != torch.int64 or confusion.dim() != 2 or confusion.shape[0] != confusion.shape[1] + 1
            or confusion.device != dev or not confusion.is_contiguous()):
        raise ValueError("confusion must be a contiguous int64 [C + 1, C] matrix on the labels' device")
    if err.dtype != torch.int32 or err.numel() != 1 or err.device != dev:
        raise ValueError("err must be an int32 [1] tensor on the labels' device")
    with _Dev(dev):
        check(lib.osn_eval_confusion(_p(votes), _p(ids), n, c_in, _p(labels), _p(mapper), n_map, _p(has_feature),
                                     confusion.shape[1], _p(confusion), _p(err), int(hist), _stream(dev)), "osn_eval_confusion")
    return confusion


def eval_check(err):
    """Raise on what eval_confusion recorded in `err` (synchronises)."""
    dev = err.device
    lib = _prep(dev)
    with _Dev(dev):
        check(lib.osn_eval_check(_p(err), _stream(dev)), "osn_eval_check")


# ---------------------------------------------------------------------- search
BANK_MAX_K = 128
BANK_MAX_Q = 1024
BANK_ENSEMBLE_MODES = ("vocabulary", "query")    # the `mode` word of osn_bank_search_ensemble: the position in this tuple


def _bank_append_args(feats, rows, row0, err, gather):
    """What bank_append and bank_append_fp8 check alike; `rows` is the matrix the rows go to.  -> (gather, n, row0)"""
    dev = feats.device
    if gather is not None:
        if gather.dim() != 1 or gather.device != dev:
            raise ValueError("gather must be a vector on the features' device")
        gather = (gather if gather.dtype == torch.int64 else gather.long()).contiguous()
    n = gather.shape[0] if gather is not None else feats.shape[0]
    row0 = int(row0)
    if row0 < 0 or row0 + n > rows.shape[0]:
        raise ValueError("rows [%d, %d) do not fit a bank of %d rows" % (row0, row0 + n, rows.shape[0]))
    if err.dtype != torch.int32 or err.numel() != 1 or err.device != dev:
        raise ValueError("err must be an int32 [1] tensor on the features' device")
    return gather, n, row0


def bank_append(bank, row0, feats, err, gather=None):
    """bank[row0 : row0 + n] = feats[gather].half() (fp16 rows of a caller-owned matrix, no float32 intermediate):
    the rows `run/evaluate.py:290` forms.  A gather index outside the feature matrix writes nothing for its row and is
    recorded in `err` (int32 [1], device) without a synchronisation; bank_check raises on it.  -> n."""
    dev = feats.device
    lib = _prep(dev)
    feats = _f32c(feats, "features")
    if feats.dim() != 2:
        raise ValueError("features must be [rows, dim]")
    if (bank.dtype != torch.float16 or bank.dim() != 2 or bank.device != dev or not bank.is_contiguous()
            or bank.shape[1] != feats.shape[1]):
        raise ValueError("the bank must be a contiguous float16 [rows, %d] matrix on the features' device" % feats.shape[1])
    gather, n, row0 = _bank_append_args(feats, bank, row0, err, gather)
    with _Dev(dev):
        check(lib.osn_bank_append(_p(feats), feats.shape[0], _p(gather), n, feats.shape[1], _p(bank), row0, _p(err),
                                  _stream(dev)), "osn_bank_append")
    return n


def bank_check(err):
    """Raise on what bank_append / bank_search recorded in `err` (synchronises)."""
    dev = err.device
    lib = _prep(dev)
    with _Dev(dev):
        check(lib.osn_bank_check(_p(err), _stream(dev)), "osn_bank_check")


def _bank_search(entries, bank_ptrs, n, d, d_multiple, dev, scene_offsets, queries, k, thresholds, normalize, want_heat,
                 max_scene_rows, err, negatives=None, temperature=0.1, ensemble_mode=None, want_source=True):
    """bank_search and bank_search_fp8 behind their own checks of the bank: `entries` are the C entries (plain, contrast)
    that take `bank_ptrs` (the fp16 rows, or the codes and the exponents) ahead of the arguments the two share; the
    contrast entry is called when `negatives` are given.  ensemble_mode ("vocabulary" / "query"): `entries` is the one
    ensemble entry, `bank_ptrs` hold both banks, and the choice of source is returned after the four results."""
    entry, tail = entries[0], ()
    if ensemble_mode is not None and ensemble_mode not in BANK_ENSEMBLE_MODES:
        raise ValueError('ensemble_mode must be "vocabulary" or "query" (got %r)' % (ensemble_mode,))
    if negatives is not None:
        if not isinstance(negatives, torch.Tensor) or negatives.dtype != torch.float16:
            raise TypeError("negatives must be a float16 tensor")
        if negatives.dim() != 2 or negatives.shape[1] != d:
            raise ValueError("negatives must be [M, %d] (got %s)" % (d, tuple(negatives.shape)))
        if negatives.device != dev:
            raise ValueError("negatives must be on the bank's device")
        if not 1 <= negatives.shape[0] <= BANK_MAX_Q:
            raise ValueError("1 .. %d negatives per call (got %d)" % (BANK_MAX_Q, negatives.shape[0]))
        temperature = float(temperature)
        if not 0.0 < temperature < float("inf"):
            raise ValueError("the temperature must be finite and > 0 (got %r)" % (temperature,))
        negatives = negatives.contiguous()
        entry, tail = entries[-1], (_p(negatives), negatives.shape[0], temperature)
    elif ensemble_mode is not None:
        tail = (None, 0, 0.0)                               # m = 0 with null negatives: plain scores
    if queries.dtype != torch.float16:
        raise TypeError("queries must be float16 (util/util.py:41-44 produces fp16)")
    if queries.dim() != 2 or queries.shape[1] != d:
        raise ValueError("queries must be [Q, %d] (got %s)" % (d, tuple(queries.shape)))
    if queries.device != dev:
        raise ValueError("queries must be on the bank's device")
    queries = queries.contiguous()
    q = queries.shape[0]
    k = int(k)
    if not 1 <= k <= BANK_MAX_K:
        raise ValueError("k must be in 1 .. %d (got %d)" % (BANK_MAX_K, k))
    if not 1 <= q <= BANK_MAX_Q:
        raise ValueError("1 .. %d queries per call (got %d)" % (BANK_MAX_Q, q))
    if d < d_multiple or d % d_multiple:
        raise ValueError("the feature dim must be a multiple of %d (got %d)" % (d_multiple, d))
    if scene_offsets.dtype != torch.int64 or scene_offsets.dim() != 1 or scene_offsets.shape[0] < 1 or scene_offsets.device != dev:
        raise ValueError("scene_offsets must be an int64 [S + 1] vector on the bank's device")
    scene_offsets = scene_offsets.contiguous()
    s = scene_offsets.shape[0] - 1
    if thresholds is not None:
        if thresholds.dtype != torch.float32 or tuple(thresholds.shape) != (q,) or thresholds.device != dev:
            raise ValueError("thresholds must be a float32 [%d] vector on the bank's device" % q)
        thresholds = thresholds.contiguous()
    if max_scene_rows is None:
        max_scene_rows = int((scene_offsets[1:] - scene_offsets[:-1]).max().item()) if s > 0 else 0
        max_scene_rows = min(max(max_scene_rows, 0), n)
    max_scene_rows = int(max_scene_rows)
    own_err = err is None
    if own_err:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    elif err.dtype != torch.int32 or err.numel() != 1 or err.device != dev:
        raise ValueError("err must be an int32 [1] tensor on the bank's device")
    heat = torch.empty((n, q), dtype=torch.float16, device=dev) if want_heat else None
    top_s = torch.empty((s, q, k), dtype=torch.float16, device=dev)
    top_p = torch.empty((s, q, k), dtype=torch.int64, device=dev)
    counts = torch.empty((s, q), dtype=torch.int64, device=dev) if thresholds is not None else None
    source = None
    if ensemble_mode is not None:
        mode = BANK_ENSEMBLE_MODES.index(ensemble_mode)
        if mode == 0:
            source = torch.empty((n,), dtype=torch.bool, device=dev)
        elif want_source:
            source = torch.empty((n, q), dtype=torch.bool, device=dev)
        tail = tail + (mode, _p(source))
    wsb = _cached("osn_bank_search_ws_bytes", n, s, q, k, max_scene_rows)
    ws = _ws(wsb, dev)
    with _Dev(dev):
        check(entry(*bank_ptrs, n, d, _p(scene_offsets), s, max_scene_rows, _p(queries), q, int(bool(normalize)), k, _p(thresholds),
                    _p(heat), _p(top_s), _p(top_p), _p(counts), _p(err), _p(ws), ws.numel(), _stream(dev), *tail), entry.__name__)
    if own_err and s > 0:
        bank_check(err)
    if ensemble_mode is not None:
        return heat, top_s, top_p, counts, source
    return heat, top_s, top_p, counts


def bank_search(bank, scene_offsets, queries, k=16, thresholds=None, normalize=True, want_heat=False, max_scene_rows=None,
                err=None, negatives=None, temperature=0.1):
    """Scores of every bank row against every query and the k best rows of every scene.
    bank fp16 [N, d]; scene_offsets int64 [S + 1] on the device (ascending from 0; S = 0 computes the heat-map only);
    queries fp16 [Q, d], L2-normalised; thresholds float32 [Q] or None.
    -> (heat fp16 [N, Q] or None, topk_scores fp16 [S, Q, k], topk_points int64 [S, Q, k] (row inside the scene, -1 = padding),
        counts int64 [S, Q] or None).
    max_scene_rows: the longest scene, when the caller knows it (saves reading the offsets back).  Bad offsets are recorded
    in `err` when one is given (bank_check raises), and checked here otherwise.
    negatives fp16 [M, d], L2-normalised (osn_bank_search_contrast): heat, the selection and the counts then hold the
    relevancy sigmoid((score - the row's best negative score) / temperature) in place of the score."""
    lib = _prep(bank.device)
    if bank.dtype != torch.float16:
        raise TypeError("the bank must be float16 (got %s)" % bank.dtype)
    if bank.dim() != 2 or not bank.is_contiguous():
        raise ValueError("the bank must be a contiguous [rows, dim] matrix")
    n, d = bank.shape
    return _bank_search((lib.osn_bank_search, lib.osn_bank_search_contrast), (_p(bank),), n, d, 8, bank.device, scene_offsets, queries,
                        k, thresholds, normalize, want_heat, max_scene_rows, err, negatives, temperature)


def bank_append_fp8(codes, exps, row0, feats, err, gather=None):
    """Rows row0 : row0 + n of an fp8 bank = feats[gather], quantised: e4m3fn codes (uint8 [rows, d]) and one exponent
    byte per row (int8 [rows]), value = code * 2^e with e the smallest integer >= -120 that brings the row's largest
    magnitude to 448 or below (include/openscene_amd.h states the format bit for bit).  feats float32 or float16
    [rows, d], d % 16 == 0.  gather and err as bank_append.  -> n."""
    dev = feats.device
    lib = _prep(dev)
    if feats.dtype not in (torch.float32, torch.float16):
        raise TypeError("features must be float32 or float16 (got %s)" % feats.dtype)
    if feats.dim() != 2:
        raise ValueError("features must be [rows, dim]")
    feats = feats.contiguous()
    d = feats.shape[1]
    if d < 16 or d % 16:
        raise ValueError("the feature dim must be a multiple of 16 (got %d)" % d)
    if (codes.dtype != torch.uint8 or codes.dim() != 2 or codes.device != dev or not codes.is_contiguous()
            or codes.shape[1] != d):
        raise ValueError("codes must be a contiguous uint8 [rows, %d] matrix on the features' device" % d)
    if (exps.dtype != torch.int8 or exps.dim() != 1 or exps.device != dev or not exps.is_contiguous()
            or exps.shape[0] != codes.shape[0]):
        raise ValueError("exponents must be a contiguous int8 [%d] vector on the features' device" % codes.shape[0])
    gather, n, row0 = _bank_append_args(feats, codes, row0, err, gather)
    with _Dev(dev):
        check(lib.osn_bank_append_fp8(_p(feats), int(feats.dtype == torch.float16), feats.shape[0], _p(gather), n, d, _p(codes),
                                      _p(exps), row0, _p(err), _stream(dev)), "osn_bank_append_fp8")
    return n


def bank_search_fp8(codes, exps, scene_offsets, queries, k=16, thresholds=None, normalize=True, want_heat=False,
                    max_scene_rows=None, err=None, negatives=None, temperature=0.1):
    """bank_search over an fp8 bank: codes uint8 [N, d] (e4m3fn), exps int8 [N], d % 16 == 0; the score is taken on the
    stored values code * 2^e.  Everything else -- arguments, results, selection order, negatives -- is bank_search's."""
    dev = codes.device
    lib = _prep(dev)
    if codes.dtype != torch.uint8:
        raise TypeError("codes must be uint8 (got %s)" % codes.dtype)
    if exps.dtype != torch.int8:
        raise TypeError("exponents must be int8 (got %s)" % exps.dtype)
    if codes.dim() != 2 or not codes.is_contiguous():
        raise ValueError("codes must be a contiguous [rows, dim] matrix")
    if exps.dim() != 1 or exps.shape[0] != codes.shape[0] or exps.device != dev or not exps.is_contiguous():
        raise ValueError("exponents must be a contiguous [%d] vector on the codes' device" % codes.shape[0])
    n, d = codes.shape
    return _bank_search((lib.osn_bank_search_fp8, lib.osn_bank_search_contrast_fp8), (_p(codes), _p(exps)), n, d, 16, dev,
                        scene_offsets, queries, k, thresholds, normalize, want_heat, max_scene_rows, err, negatives, temperature)


def _same_bank(what, a, b):
    if b.dtype != a.dtype or tuple(b.shape) != tuple(a.shape) or b.device != a.device or not b.is_contiguous():
        raise ValueError("the other bank's %s must be a contiguous %s %s tensor on the bank's device (got %s %s on %s)"
                         % (what, a.dtype, tuple(a.shape), b.dtype, tuple(b.shape), b.device))


def bank_search_ensemble(bank, other, scene_offsets, queries, k=16, thresholds=None, normalize=True, want_heat=False,
                         max_scene_rows=None, err=None, negatives=None, temperature=0.1, mode="vocabulary", want_source=True):
    """bank_search over two fp16 banks of the same shape as one (osn_bank_search_ensemble; run/evaluate.py:302-324): row p
    of the heat-map is that of `other` where the pick says so, of `bank` elsewhere.  mode "vocabulary": the source whose best
    normalised score over the call's queries is larger (other only if strictly larger); "query": per element, the larger of
    the two scores (relevancies with negatives).  -> bank_search's four results and source: bool [N] ("vocabulary"), bool
    [N, Q] or, without want_source, None ("query").  The selection and the counts are taken on the combined heat-map."""
    lib = _prep(bank.device)
    if bank.dtype != torch.float16:
        raise TypeError("the bank must be float16 (got %s)" % bank.dtype)
    if bank.dim() != 2 or not bank.is_contiguous():
        raise ValueError("the bank must be a contiguous [rows, dim] matrix")
    _same_bank("rows", bank, other)
    n, d = bank.shape
    return _bank_search((lib.osn_bank_search_ensemble,), (_p(bank), _p(other)), n, d, 8, bank.device, scene_offsets, queries, k,
                        thresholds, normalize, want_heat, max_scene_rows, err, negatives, temperature, mode, want_source)


def bank_search_ensemble_fp8(codes, exps, other_codes, other_exps, scene_offsets, queries, k=16, thresholds=None, normalize=True,
                             want_heat=False, max_scene_rows=None, err=None, negatives=None, temperature=0.1, mode="vocabulary",
                             want_source=True):
    """bank_search_ensemble over two fp8 banks (osn_bank_search_ensemble_fp8): (codes, exps) and (other_codes, other_exps) as
    bank_search_fp8 takes them; everything else is bank_search_ensemble's."""
    dev = codes.device
    lib = _prep(dev)
    if codes.dtype != torch.uint8:
        raise TypeError("codes must be uint8 (got %s)" % codes.dtype)
    if exps.dtype != torch.int8:
        raise TypeError("exponents must be int8 (got %s)" % exps.dtype)
    if codes.dim() != 2 or not codes.is_contiguous():
        raise ValueError("codes must be a contiguous [rows, dim] matrix")
    if exps.dim() != 1 or exps.shape[0] != codes.shape[0] or exps.device != dev or not exps.is_contiguous():
        raise ValueError("exponents must be a contiguous [%d] vector on the codes' device" % codes.shape[0])
    _same_bank("codes", codes, other_codes)
    _same_bank("exponents", exps, other_exps)
    n, d = codes.shape
    return _bank_search((lib.osn_bank_search_ensemble_fp8,), (_p(codes), _p(exps), _p(other_codes), _p(other_exps)), n, d, 16, dev,
                        scene_offsets, queries, k, thresholds, normalize, want_heat, max_scene_rows, err, negatives, temperature,
                        mode, want_source)


# ------------------------------------------------------------------------ pool
BANK_POOL_CHUNK = 512            # OSN_BANK_POOL_CHUNK: the entries of a group that are reduced into one fp32 partial
BANK_POOL_MAX_DIM = 1024         # OSN_BANK_POOL_MAX_DIM: the widest row a wave keeps in registers


def _bank_groups(d, d_multiple, dev, starts, rows, n_entries, err):
    """What the pool and the Gram matrix check alike: the feature dim and the CSR groups over the bank.
    -> (starts, g, rows, n_entries, err, own_err)"""
    if d < d_multiple or d % d_multiple:
        raise ValueError("the feature dim must be a multiple of %d (got %d)" % (d_multiple, d))
    if d > BANK_POOL_MAX_DIM:
        raise ValueError("the feature dim must be at most %d (got %d)" % (BANK_POOL_MAX_DIM, d))
    if not isinstance(starts, torch.Tensor) or starts.dtype != torch.int64:
        raise TypeError("starts must be an int64 tensor")
    if starts.dim() != 1 or starts.shape[0] < 1 or starts.device != dev:
        raise ValueError("starts must be an int64 [G + 1] vector on the bank's device")
    starts = starts.contiguous()
    g = starts.shape[0] - 1
    if rows is not None:
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64:
            raise TypeError("rows must be an int64 tensor (or None: entry i is bank row i)")
        if rows.dim() != 1 or rows.device != dev:
            raise ValueError("rows must be an int64 [L] vector on the bank's device")
        rows = rows.contiguous()
        if n_entries is not None and int(n_entries) != rows.shape[0]:
            raise ValueError("n_entries=%d for %d rows" % (int(n_entries), rows.shape[0]))
        n_entries = rows.shape[0]
    elif n_entries is None:
        raise ValueError("without rows, n_entries (= starts[-1]) must be given")
    n_entries = int(n_entries)
    if n_entries < 0:
        raise ValueError("n_entries must not be negative (got %d)" % n_entries)
    own_err = err is None
    if own_err:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    elif err.dtype != torch.int32 or err.numel() != 1 or err.device != dev:
        raise ValueError("err must be an int32 [1] tensor on the bank's device")
    return starts, g, rows, n_entries, err, own_err


def _bank_pool(entry, bank_ptrs, n, d, d_multiple, dev, starts, rows, weights, normalize, n_entries, err):
    """bank_pool and bank_pool_fp8 behind their own checks of the bank: `entry` is the C entry that takes `bank_ptrs`
    (the fp16 rows, or the codes and the exponents) ahead of the arguments the two share."""
    starts, g, rows, n_entries, err, own_err = _bank_groups(d, d_multiple, dev, starts, rows, n_entries, err)
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32:
            raise TypeError("weights must be a float32 tensor")
        if tuple(weights.shape) != (n_entries,) or weights.device != dev:
            raise ValueError("weights must be a float32 [%d] vector on the bank's device (got %s)" % (n_entries, tuple(weights.shape)))
        weights = weights.contiguous()
    out = torch.empty((g, d), dtype=torch.float32, device=dev)
    wsum = torch.empty((g,), dtype=torch.float32, device=dev)
    count = torch.empty((g,), dtype=torch.int64, device=dev)
    wsb = _cached("osn_bank_pool_ws_bytes", g, n_entries, d)
    ws = _ws(wsb, dev)
    with _Dev(dev):
        check(entry(*bank_ptrs, n, d, _p(starts), g, _p(rows), n_entries, _p(weights), int(bool(normalize)), _p(out), _p(wsum),
                    _p(count), _p(err), _p(ws), ws.numel(), _stream(dev)), entry.__name__)
    if own_err and g > 0:
        bank_check(err)
    return out, wsum, count


def _fp16_bank(bank):
    """The checks of an fp16 bank's rows.  -> (n, d)"""
    if bank.dtype != torch.float16:
        raise TypeError("the bank must be float16 (got %s)" % bank.dtype)
    if bank.dim() != 2 or not bank.is_contiguous():
        raise ValueError("the bank must be a contiguous [rows, dim] matrix")
    return bank.shape


def _fp8_bank(codes, exps):
    """The checks of an fp8 bank's codes and exponents.  -> (n, d)"""
    if codes.dtype != torch.uint8:
        raise TypeError("codes must be uint8 (got %s)" % codes.dtype)
    if exps.dtype != torch.int8:
        raise TypeError("exponents must be int8 (got %s)" % exps.dtype)
    if codes.dim() != 2 or not codes.is_contiguous():
        raise ValueError("codes must be a contiguous [rows, dim] matrix")
    if exps.dim() != 1 or exps.shape[0] != codes.shape[0] or exps.device != codes.device or not exps.is_contiguous():
        raise ValueError("exponents must be a contiguous [%d] vector on the codes' device" % codes.shape[0])
    return codes.shape


def bank_pool(bank, starts, rows=None, weights=None, normalize=True, n_entries=None, err=None):
    """Sums of the (normalised, weighted) rows of every group of a CSR list of bank rows: an entry adds
    ``w * hf / (hf.norm() + 1e-5)`` (`run/evaluate.py:305`; normalize) or ``w * hf`` of its stored fp16 row, in fp32.
    bank fp16 [N, d], d <= BANK_POOL_MAX_DIM; starts int64 [G + 1] on the device, ascending from 0 to L; rows int64 [L] or
    None (entry i is bank row i; L = n_entries); weights float32 [L] or None (1).
    -> (sum float32 [G, d], wsum float32 [G], count int64 [G]).
    A group is reduced in chunks of BANK_POOL_CHUNK entries in a fixed order: bitwise repeatable.  A row outside the bank
    and a negative or non-finite weight skip their entry and are recorded in `err` when one is given (bank_check raises),
    and checked here otherwise."""
    lib = _prep(bank.device)
    n, d = _fp16_bank(bank)
    return _bank_pool(lib.osn_bank_pool, (_p(bank),), n, d, 8, bank.device, starts, rows, weights, normalize, n_entries, err)


def bank_pool_fp8(codes, exps, starts, rows=None, weights=None, normalize=True, n_entries=None, err=None):
    """bank_pool over an fp8 bank: codes uint8 [N, d] (e4m3fn), exps int8 [N], d % 16 == 0; a row's value is
    code * 2^e, decoded exactly.  Everything else is bank_pool's."""
    dev = codes.device
    lib = _prep(dev)
    n, d = _fp8_bank(codes, exps)
    return _bank_pool(lib.osn_bank_pool_fp8, (_p(codes), _p(exps)), n, d, 16, dev, starts, rows, weights, normalize, n_entries, err)


# ------------------------------------------------------------------------ gram
BANK_GRAM_SLICE = 2048           # OSN_BANK_GRAM_SLICE: the entries of a group that are reduced into one fp32 partial per tile pair


def _bank_gram(entry, bank_ptrs, n, d, d_multiple, dev, starts, rows, normalize, n_entries, err):
    """bank_gram and bank_gram_fp8 behind their own checks of the bank (the pool's checks of the groups)."""
    starts, g, rows, n_entries, err, own_err = _bank_groups(d, d_multiple, dev, starts, rows, n_entries, err)
    gram = torch.empty((g, d, d), dtype=torch.float32, device=dev)
    total = torch.empty((g, d), dtype=torch.float32, device=dev)
    count = torch.empty((g,), dtype=torch.int64, device=dev)
    wsb = _cached("osn_bank_gram_ws_bytes", g, n_entries, d)
    ws = _ws(wsb, dev)
    with _Dev(dev):
        check(entry(*bank_ptrs, n, d, _p(starts), g, _p(rows), n_entries, int(bool(normalize)), _p(gram), _p(total), _p(count),
                    _p(err), _p(ws), ws.numel(), _stream(dev)), entry.__name__)
    if own_err and g > 0:
        bank_check(err)
    return gram, total, count


def bank_gram(bank, starts, rows=None, normalize=True, n_entries=None, err=None):
    """Second and first moments of the rows of every group of a CSR list of bank rows: with
    ``h = (hf / (hf.norm() + 1e-5)).half()`` (`run/evaluate.py:305,310`; normalize) or ``h = hf`` of an entry's stored row,
    gram[g] = sum h h^T (fp16 MFMA: exact products, fp32 accumulation), sum[g] = sum h.
    bank, starts, rows, n_entries and err as bank_pool.
    -> (gram float32 [G, d, d], bitwise symmetric; sum float32 [G, d]; count int64 [G]).
    A group is reduced in slices of BANK_GRAM_SLICE entries in a fixed order: bitwise repeatable."""
    lib = _prep(bank.device)
    n, d = _fp16_bank(bank)
    return _bank_gram(lib.osn_bank_gram, (_p(bank),), n, d, 8, bank.device, starts, rows, normalize, n_entries, err)


def bank_gram_fp8(codes, exps, starts, rows=None, normalize=True, n_entries=None, err=None):
    """bank_gram over an fp8 bank: codes uint8 [N, d] (e4m3fn), exps int8 [N], d % 16 == 0; a row's value is
    code * 2^e, decoded exactly and rounded to fp16 (after the normalisation).  Everything else is bank_gram's."""
    dev = codes.device
    lib = _prep(dev)
    n, d = _fp8_bank(codes, exps)
    return _bank_gram(lib.osn_bank_gram_fp8, (_p(codes), _p(exps)), n, d, 16, dev, starts, rows, normalize, n_entries, err)


# ----------------------------------------------------------------------- match
BANK_MATCH_MAX_K = 8             # OSN_BANK_MATCH_MAX_K
BANK_MATCH_TILE_Q = 64           # OSN_BANK_MATCH_TILE_Q: the query rows of a workgroup
BANK_MATCH_TILE_E = 256          # OSN_BANK_MATCH_TILE_E: the exemplars of a tile
BANK_MATCH_MAX_SPLITS = 64       # OSN_BANK_MATCH_MAX_SPLITS: the most ranges the exemplar tiles are cut into


def _bank_rows(d, d_multiple, dev, rows, n, err):
    """What unit_rows and match check alike (the pool's wording): the feature dim, the row list, the err word.
    -> (rows, n_rows, err, own_err)"""
    if d < d_multiple or d % d_multiple:
        raise ValueError("the feature dim must be a multiple of %d (got %d)" % (d_multiple, d))
    if d > BANK_POOL_MAX_DIM:
        raise ValueError("the feature dim must be at most %d (got %d)" % (BANK_POOL_MAX_DIM, d))
    if rows is not None:
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64:
            raise TypeError("rows must be an int64 tensor (or None: entry i is bank row i)")
        if rows.dim() != 1 or rows.device != dev:
            raise ValueError("rows must be an int64 [L] vector on the bank's device")
        rows = rows.contiguous()
    n_rows = rows.shape[0] if rows is not None else n
    own_err = err is None
    if own_err:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    elif err.dtype != torch.int32 or err.numel() != 1 or err.device != dev:
        raise ValueError("err must be an int32 [1] tensor on the bank's device")
    return rows, n_rows, err, own_err


def _bank_unit_rows(entry, bank_ptrs, n, d, d_multiple, dev, rows, normalize, err):
    rows, m, err, own_err = _bank_rows(d, d_multiple, dev, rows, n, err)
    out = torch.empty((m, d), dtype=torch.float16, device=dev)
    with _Dev(dev):
        check(entry(*bank_ptrs, n, d, _p(rows), m, int(bool(normalize)), _p(out), _p(err), _stream(dev)), entry.__name__)
    if own_err and m > 0:
        bank_check(err)
    return out


def bank_unit_rows(bank, rows=None, normalize=True, err=None):
    """The operands of a list of bank rows as an fp16 image [M, d]: ``(hf / (hf.norm() + 1e-5)).half()``
    (`run/evaluate.py:305,310`; normalize) or the stored row, bit for bit what bank_gram multiplies.  bank fp16 [N, d],
    d <= BANK_POOL_MAX_DIM; rows int64 [M] on the device or None (every row).  A row outside the bank writes zeros and is
    recorded in `err` when one is given (bank_check raises), and checked here otherwise."""
    lib = _prep(bank.device)
    n, d = _fp16_bank(bank)
    return _bank_unit_rows(lib.osn_bank_unit_rows, (_p(bank),), n, d, 8, bank.device, rows, normalize, err)


def bank_unit_rows_fp8(codes, exps, rows=None, normalize=True, err=None):
    """bank_unit_rows over an fp8 bank: codes uint8 [N, d] (e4m3fn), exps int8 [N], d % 16 == 0; a row's value is
    code * 2^e, decoded exactly and rounded to fp16 (after the normalisation)."""
    dev = codes.device
    lib = _prep(dev)
    n, d = _fp8_bank(codes, exps)
    return _bank_unit_rows(lib.osn_bank_unit_rows_fp8, (_p(codes), _p(exps)), n, d, 16, dev, rows, normalize, err)


def bank_match_ws_bytes(n_rows, n_exemplars, d, k, splits=None):
    """The bytes of workspace a bank_match call takes: 8 * n_rows * k * splits plus a constant, never n_rows * n_exemplars."""
    return _cached("osn_bank_match_ws_bytes", int(n_rows), int(n_exemplars), int(d), int(k), 0 if splits is None else int(splits))


def _bank_match(entry, bank_ptrs, n, d, d_multiple, dev, exemplars, k, rows, normalize, splits, err):
    if not isinstance(exemplars, torch.Tensor) or exemplars.dtype != torch.float16:
        raise TypeError("exemplars must be a float16 tensor (bank_unit_rows makes them)")
    if exemplars.dim() != 2 or exemplars.shape[1] != d:
        raise ValueError("exemplars must be [M, %d] (got %s)" % (d, tuple(exemplars.shape)))
    if exemplars.device != dev:
        raise ValueError("exemplars must be on the bank's device")
    m = exemplars.shape[0]
    if not 1 <= m < (1 << 31):
        raise ValueError("1 .. 2^31 - 1 exemplars per call (got %d)" % m)
    exemplars = exemplars.contiguous()
    k = int(k)
    if not 1 <= k <= BANK_MATCH_MAX_K:
        raise ValueError("k must be in 1 .. %d (got %d)" % (BANK_MATCH_MAX_K, k))
    splits = 0 if splits is None else int(splits)
    if splits != 0 and not 1 <= splits <= BANK_MATCH_MAX_SPLITS:
        raise ValueError("splits must be in 1 .. %d or None (got %d)" % (BANK_MATCH_MAX_SPLITS, splits))
    rows, l, err, own_err = _bank_rows(d, d_multiple, dev, rows, n, err)
    idx = torch.empty((l, k), dtype=torch.int32, device=dev)
    score = torch.empty((l, k), dtype=torch.float32, device=dev)
    count = torch.empty((l,), dtype=torch.int32, device=dev)
    wsb = _cached("osn_bank_match_ws_bytes", l, m, d, k, splits)
    ws = _ws(wsb, dev)
    with _Dev(dev):
        check(entry(*bank_ptrs, n, d, _p(rows), l, int(bool(normalize)), _p(exemplars), m, k, splits, _p(idx), _p(score), _p(count),
                    _p(err), _p(ws), ws.numel(), _stream(dev)), entry.__name__)
    if own_err and l > 0:
        bank_check(err)
    return idx, score, count


def bank_match(bank, exemplars, k=1, rows=None, normalize=True, splits=None, err=None):
    """For each of the bank rows `rows` (int64 [L] on the device; None: every row) the k most similar of the exemplars.
    bank fp16 [N, d]; exemplars fp16 [M, d]: an image from bank_unit_rows; 1 <= k <= BANK_MATCH_MAX_K.  The query row's
    operand is bank_unit_rows' (normalize as there), the score the fp32 MFMA accumulation of the fp16 products over d in a
    fixed order, equal scores go to the lower exemplar position, a NaN ranks below -inf.
    -> (idx int32 [L, k], -1 past count; score float32 [L, k], -inf past count; count int32 [L] = min(k, M)).
    A workgroup takes BANK_MATCH_TILE_Q rows and tiles of BANK_MATCH_TILE_E exemplars; the tiles are cut into `splits`
    ranges (None: chosen so that the grid fills the device) -- the result does not depend on it.  Bitwise repeatable.  err
    as bank_unit_rows (a row outside the bank is matched as a zero row)."""
    lib = _prep(bank.device)
    n, d = _fp16_bank(bank)
    return _bank_match(lib.osn_bank_match, (_p(bank),), n, d, 8, bank.device, exemplars, k, rows, normalize, splits, err)


def bank_match_fp8(codes, exps, exemplars, k=1, rows=None, normalize=True, splits=None, err=None):
    """bank_match with the query rows of an fp8 bank: codes uint8 [N, d] (e4m3fn), exps int8 [N], d % 16 == 0.  The
    exemplars are an fp16 image all the same (bank_unit_rows_fp8 widens fp8 rows once)."""
    dev = codes.device
    lib = _prep(dev)
    n, d = _fp8_bank(codes, exps)
    return _bank_match(lib.osn_bank_match_fp8, (_p(codes), _p(exps)), n, d, 16, dev, exemplars, k, rows, normalize, splits, err)


# --------------------------------------------------------------------- objects
OBJECTS_MAX_M = 64
OBJECTS_MAX_POINTS = 1 << 22          # keeps score_sum inside int64 for raw scores at the fp16 maximum


def objects_find(heat, thresholds, xyz, inverse, coords4, nbr, scene_offsets, connectivity=26, min_points=1, max_objects=16,
                 return_point_ids=False, combine=True):
    """Objects of a heat-map: connected components of the voxels that hold a hit, ranked per (scene, query).
    heat fp16 [N, Q]; thresholds float32 [Q]; xyz float32 [N, 3]; inverse int32 [N] (point -> voxel row); coords4 int32
    [V, 4] (scene, x, y, z) and nbr int32 [27, V] = coords_unique's rows and kmap_build(..., 3, 1, self_map=True) over
    them; scene_offsets int64 [S + 1].  All on one device, contiguous.
    -> dict of [S, Q, M] tensors: n_points, n_voxels, peak_point, score_sum int64, peak_score fp16, vox_sum int64 [.., 3],
       box_min / box_max float32 [.., 3]; n_objects int64 [S, Q]; point_object int32 [N, Q] or None.
    The number of components is read back to the host once per call (one synchronisation) to size the record scratch."""
    dev = heat.device
    lib = _prep(dev)
    if heat.dtype != torch.float16:
        raise TypeError("heat must be float16 (got %s)" % heat.dtype)
    if heat.dim() != 2 or not heat.is_contiguous():
        raise ValueError("heat must be a contiguous [points, Q] matrix")
    n, q = heat.shape
    if not 1 <= q <= BANK_MAX_Q:
        raise ValueError("1 .. %d queries per call (got %d)" % (BANK_MAX_Q, q))
    if n >= OBJECTS_MAX_POINTS:
        raise ValueError("at most 2^22 - 1 points per call (got %d)" % n)
    if thresholds.dtype != torch.float32 or tuple(thresholds.shape) != (q,) or thresholds.device != dev:
        raise ValueError("thresholds must be a float32 [%d] vector on the heat-map's device" % q)
    if xyz.dtype != torch.float32 or tuple(xyz.shape) != (n, 3) or xyz.device != dev or not xyz.is_contiguous():
        raise ValueError("xyz must be a contiguous float32 [%d, 3] matrix on the heat-map's device" % n)
    if inverse.dtype != torch.int32 or tuple(inverse.shape) != (n,) or inverse.device != dev or not inverse.is_contiguous():
        raise ValueError("inverse must be a contiguous int32 [%d] vector on the heat-map's device" % n)
    if coords4.dtype != torch.int32 or coords4.dim() != 2 or coords4.shape[1] != 4 or coords4.device != dev or not coords4.is_contiguous():
        raise ValueError("coords4 must be contiguous int32 [V, 4] rows on the heat-map's device")
    v = coords4.shape[0]
    if nbr.dtype != torch.int32 or tuple(nbr.shape) != (27, v) or nbr.device != dev or not nbr.is_contiguous():
        raise ValueError("nbr must be a contiguous int32 [27, %d] table on the heat-map's device" % v)
    if scene_offsets.dtype != torch.int64 or scene_offsets.dim() != 1 or scene_offsets.shape[0] < 1 or scene_offsets.device != dev:
        raise ValueError("scene_offsets must be an int64 [S + 1] vector on the heat-map's device")
    if connectivity not in (6, 26):
        raise ValueError("connectivity must be 6 or 26 (got %r)" % (connectivity,))
    min_points, m = int(min_points), int(max_objects)
    if not 1 <= m <= OBJECTS_MAX_M:
        raise ValueError("max_objects must be in 1 .. %d (got %d)" % (OBJECTS_MAX_M, m))
    if min_points < 1:
        raise ValueError("min_points must be at least 1 (got %d)" % min_points)
    if q * v >= 1 << 31:
        raise ValueError("Q * voxels must stay below 2^31 (got %d x %d)" % (q, v))
    scene_offsets = scene_offsets.contiguous()
    thresholds = thresholds.contiguous()
    s = scene_offsets.shape[0] - 1
    err = torch.empty(1, dtype=torch.int32, device=dev)                  # (zeroed by the call)
    ws = torch.empty(max(_cached("osn_objects_ws_bytes", v, s, q), 16), dtype=torch.uint8, device=dev)   # own buffer: it lives across two calls
    out = {
        "n_points": torch.empty((s, q, m), dtype=torch.int64, device=dev),
        "n_voxels": torch.empty((s, q, m), dtype=torch.int64, device=dev),
        "peak_score": torch.empty((s, q, m), dtype=torch.float16, device=dev),
        "peak_point": torch.empty((s, q, m), dtype=torch.int64, device=dev),
        "score_sum": torch.empty((s, q, m), dtype=torch.int64, device=dev),
        "vox_sum": torch.empty((s, q, m, 3), dtype=torch.int64, device=dev),
        "box_min": torch.empty((s, q, m, 3), dtype=torch.float32, device=dev),
        "box_max": torch.empty((s, q, m, 3), dtype=torch.float32, device=dev),
        "n_objects": torch.empty((s, q), dtype=torch.int64, device=dev),
        "point_object": torch.empty((n, q), dtype=torch.int32, device=dev) if return_point_ids else None,
    }
    nc = ctypes.c_int64(0)
    with _Dev(dev):
        st = _stream(dev)
        check(lib.osn_objects_label(_p(heat), n, q, _p(thresholds), _p(inverse), _p(coords4), v, _p(nbr), int(connectivity),
                                    _p(scene_offsets), s, _p(err), _p(ws), ws.numel(), ctypes.byref(nc), st), "osn_objects_label")
        c = int(nc.value)
        rec = _ws(lib.osn_objects_records_bytes(c), dev)
        check(lib.osn_objects_find(_p(heat), _p(xyz), n, q, _p(thresholds), _p(inverse), _p(coords4), v, _p(scene_offsets), s, c,
                                   min_points, m, int(bool(combine)), _p(out["n_points"]), _p(out["n_voxels"]), _p(out["peak_score"]),
                                   _p(out["peak_point"]), _p(out["score_sum"]), _p(out["vox_sum"]), _p(out["box_min"]),
                                   _p(out["box_max"]), _p(out["n_objects"]), _p(out["point_object"]), _p(ws), ws.numel(), _p(rec),
                                   rec.numel(), st), "osn_objects_find")
    return out


# --------------------------------------------------------------------- regions
REGIONS_E_NBR, REGIONS_E_INVERSE, REGIONS_E_REGION = 1, 2, 4      # the bits of the regions' err word (csrc/regions.hip)
REGIONS_E_PAIR = 8                                                # ... and the one csrc/merge.hip adds
MERGE_RUN = 8                    # MERGE_RUN of csrc/merge.hip: the consecutive pairs a wave of rows_pair_dot takes


def regions_n_off(connectivity):
    """Rows of a `sim` array: the offsets below the centre of the 3^3 map (13), or the three faces among them."""
    if connectivity not in (6, 26):
        raise ValueError("connectivity must be 6 or 26 (got %r)" % (connectivity,))
    return 13 if connectivity == 26 else 3


def regions_check(err):
    """Raise if a regions call recorded an entry out of range in `err` (int32 [1]); zeroes the word.  Synchronises."""
    bits = int(err.item())
    if bits == 0:
        return
    err.zero_()
    what = [text for bit, text in ((REGIONS_E_NBR, "a neighbour row outside [-1, n_voxels)"),
                                   (REGIONS_E_INVERSE, "a point's voxel row outside [0, n_voxels)"),
                                   (REGIONS_E_REGION, "a region entry outside [-1, n_regions)"),
                                   (REGIONS_E_PAIR, "a pair end outside [0, n_regions)")) if bits & bit]
    raise _lib.OpenSceneAmdError("regions: %s (err bits %d); such entries were skipped" % ("; ".join(what) or "unknown error", bits))


def _regions_err(err, dev):
    if err is None:
        return torch.zeros(1, dtype=torch.int32, device=dev), True
    if not isinstance(err, torch.Tensor) or err.dtype != torch.int32 or err.numel() != 1 or err.device != dev:
        raise ValueError("err must be an int32 [1] tensor on the inputs' device")
    return err, False


def _regions_nbr(nbr, v, dev):
    if not isinstance(nbr, torch.Tensor) or nbr.dtype != torch.int32 or tuple(nbr.shape) != (27, v) or nbr.device != dev \
            or not nbr.is_contiguous():
        raise ValueError("nbr must be a contiguous int32 [27, %d] table on the rows' device" % v)


def regions_edges(vox, nbr, connectivity=26, err=None):
    """sim float32 [n_off, V]: the fp32 dot product of every voxel row with its neighbours below the centre of the 3^3 map
    (n_off = 13: k = 0 .. 12; connectivity 6: k = 4, 10, 12), every undirected edge once.  vox fp16 [V, d] unit rows,
    d % 8 == 0, 8 <= d <= BANK_POOL_MAX_DIM; nbr int32 [27, V] = kmap_build(..., 3, 1, self_map=True).  An absent
    neighbour gives -inf, a NaN in either row NaN.  Fixed order of additions: bitwise repeatable.  A neighbour row >= V is
    skipped and recorded in `err` when one is given (regions_check raises), and checked here otherwise."""
    if not isinstance(vox, torch.Tensor) or vox.dtype != torch.float16:
        raise TypeError("vox must be a float16 tensor")
    dev = vox.device
    lib = _prep(dev)
    if vox.dim() != 2 or not vox.is_contiguous():
        raise ValueError("vox must be a contiguous [voxels, dim] matrix")
    v, d = vox.shape
    if d < 8 or d % 8:
        raise ValueError("the feature dim must be a multiple of 8 (got %d)" % d)
    if d > BANK_POOL_MAX_DIM:
        raise ValueError("the feature dim must be at most %d (got %d)" % (BANK_POOL_MAX_DIM, d))
    n_off = regions_n_off(connectivity)
    _regions_nbr(nbr, v, dev)
    err, own = _regions_err(err, dev)
    sim = torch.empty((n_off, v), dtype=torch.float32, device=dev)
    with _Dev(dev):
        check(lib.osn_regions_edges(_p(vox), v, d, _p(nbr), int(connectivity), _p(sim), _p(err), _stream(dev)), "osn_regions_edges")
    if own and v > 0:
        regions_check(err)
    return sim


def regions_label(sim, nbr, connectivity=26, threshold=0.9, err=None):
    """voxel_root int32 [V]: the smallest voxel row of every voxel's component in the graph whose edges are the neighbour
    pairs with sim >= threshold (float32; NaN and -inf never unite).  sim float32 [n_off, V] (regions_edges), nbr its
    table.  The labelling is canonical: it does not depend on scheduling.  `err` as regions_edges."""
    if not isinstance(sim, torch.Tensor) or sim.dtype != torch.float32:
        raise TypeError("sim must be a float32 tensor")
    dev = sim.device
    lib = _prep(dev)
    n_off = regions_n_off(connectivity)
    if sim.dim() != 2 or sim.shape[0] != n_off or not sim.is_contiguous():
        raise ValueError("sim must be a contiguous float32 [%d, V] matrix for connectivity %d" % (n_off, connectivity))
    v = sim.shape[1]
    _regions_nbr(nbr, v, dev)
    threshold = float(threshold)
    if threshold != threshold or threshold in (float("inf"), float("-inf")):
        raise ValueError("the threshold must be finite (got %r)" % (threshold,))
    err, own = _regions_err(err, dev)
    root = torch.empty(v, dtype=torch.int32, device=dev)
    with _Dev(dev):
        check(lib.osn_regions_label(_p(sim), _p(nbr), v, int(connectivity), threshold, _p(root), _p(err), _stream(dev)),
              "osn_regions_label")
    if own and v > 0:
        regions_check(err)
    return root


def regions_records(voxel_region, n_regions, xyz, inverse, coords4, err=None):
    """Exact records of the regions of a labelling.  voxel_region int32 [V] in -1 .. R - 1; xyz float32 [N, 3]; inverse
    int32 [N] (point -> voxel row); coords4 int32 [V, 4] (scene, x, y, z).
    -> dict: n_points, n_voxels int64 [R]; vox_sum int64 [R, 3] (over the points, of their voxel's cell); box_min / box_max
       float32 [R, 3]; scene int32 [R].  Integer atomics only: bitwise repeatable.  Points of voxels with region -1 are
    counted nowhere.  An entry out of range is skipped and recorded in `err` (as regions_edges)."""
    if not isinstance(voxel_region, torch.Tensor) or voxel_region.dtype != torch.int32:
        raise TypeError("voxel_region must be an int32 tensor")
    dev = voxel_region.device
    lib = _prep(dev)
    if voxel_region.dim() != 1 or not voxel_region.is_contiguous():
        raise ValueError("voxel_region must be a contiguous int32 [V] vector")
    v = voxel_region.shape[0]
    r = int(n_regions)
    if not 0 <= r <= v:
        raise ValueError("n_regions must lie in 0 .. %d (got %d)" % (v, r))
    if xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.device != dev or not xyz.is_contiguous():
        raise ValueError("xyz must be a contiguous float32 [N, 3] matrix on the labelling's device")
    n = xyz.shape[0]
    if inverse.dtype != torch.int32 or tuple(inverse.shape) != (n,) or inverse.device != dev or not inverse.is_contiguous():
        raise ValueError("inverse must be a contiguous int32 [%d] vector on the labelling's device" % n)
    if coords4.dtype != torch.int32 or tuple(coords4.shape) != (v, 4) or coords4.device != dev or not coords4.is_contiguous():
        raise ValueError("coords4 must be contiguous int32 [%d, 4] rows on the labelling's device" % v)
    err, own = _regions_err(err, dev)
    out = {
        "n_points": torch.empty(r, dtype=torch.int64, device=dev),
        "n_voxels": torch.empty(r, dtype=torch.int64, device=dev),
        "vox_sum": torch.empty((r, 3), dtype=torch.int64, device=dev),
        "box_min": torch.empty((r, 3), dtype=torch.float32, device=dev),
        "box_max": torch.empty((r, 3), dtype=torch.float32, device=dev),
        "scene": torch.empty(r, dtype=torch.int32, device=dev),
    }
    with _Dev(dev):
        check(lib.osn_regions_records(_p(voxel_region), v, r, _p(xyz), _p(inverse), n, _p(coords4), _p(out["n_points"]),
                                      _p(out["n_voxels"]), _p(out["vox_sum"]), _p(out["box_min"]), _p(out["box_max"]),
                                      _p(out["scene"]), _p(err), _stream(dev)), "osn_regions_records")
    if own and (v > 0 or n > 0):
        regions_check(err)
    return out


# ----------------------------------------------------------------------- merge
def regions_contacts(voxel_region, nbr, connectivity, n_regions, err=None):
    """key int64 [n_off, V]: ``lo << 32 | hi`` of the regions of voxel v and its neighbour nbr[k_i, v] below the centre
    (n_off and k_i as regions_edges) where both are >= 0 and differ, else -1.  voxel_region int32 [V] in -1 .. R - 1.
    The distinct non-negative keys, sorted, are the region adjacency list; their multiplicities the contact counts
    (merge.region_adjacency).  Entries out of range are skipped and recorded in `err` (as regions_edges)."""
    if not isinstance(voxel_region, torch.Tensor) or voxel_region.dtype != torch.int32:
        raise TypeError("voxel_region must be an int32 tensor")
    dev = voxel_region.device
    lib = _prep(dev)
    if voxel_region.dim() != 1 or not voxel_region.is_contiguous():
        raise ValueError("voxel_region must be a contiguous int32 [V] vector")
    v = voxel_region.shape[0]
    n_off = regions_n_off(connectivity)
    _regions_nbr(nbr, v, dev)
    r = int(n_regions)
    if not 0 <= r <= v:
        raise ValueError("n_regions must lie in 0 .. %d (got %d)" % (v, r))
    err, own = _regions_err(err, dev)
    key = torch.empty((n_off, v), dtype=torch.int64, device=dev)
    with _Dev(dev):
        check(lib.osn_merge_contacts(_p(voxel_region), _p(nbr), v, int(connectivity), r, _p(key), _p(err), _stream(dev)),
              "osn_merge_contacts")
    if own and v > 0:
        regions_check(err)
    return key


def _merge_pairs(lo, hi, dev):
    for name, t in (("lo", lo), ("hi", hi)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise TypeError("%s must be an int32 tensor" % name)
    if lo.dim() != 1 or lo.shape != hi.shape or lo.device != dev or hi.device != dev or not lo.is_contiguous() or not hi.is_contiguous():
        raise ValueError("lo and hi must be contiguous int32 [E] vectors of one length on the rows' device")
    e = lo.shape[0]
    if e >= 2 ** 32 - 1:
        raise ValueError("at most 2^32 - 2 pairs (got %d)" % e)
    return e


def rows_pair_dot(rows, lo, hi, err=None):
    """sim float32 [E]: the fp32 dot product of rows[lo[e]] and rows[hi[e]].  rows fp16 [R, d], d % 8 == 0, 8 <= d <=
    BANK_POOL_MAX_DIM; lo, hi int32 [E].  The arithmetic is that of regions_edges -- the same bits for the same two rows --
    and the order of additions is fixed: bitwise repeatable.  An end outside [0, R) gives -inf and is recorded in `err`
    when one is given (regions_check raises), and checked here otherwise."""
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float16:
        raise TypeError("rows must be a float16 tensor")
    dev = rows.device
    lib = _prep(dev)
    if rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous [rows, dim] matrix")
    r, d = rows.shape
    if d < 8 or d % 8:
        raise ValueError("the feature dim must be a multiple of 8 (got %d)" % d)
    if d > BANK_POOL_MAX_DIM:
        raise ValueError("the feature dim must be at most %d (got %d)" % (BANK_POOL_MAX_DIM, d))
    e = _merge_pairs(lo, hi, dev)
    err, own = _regions_err(err, dev)
    sim = torch.empty(e, dtype=torch.float32, device=dev)
    with _Dev(dev):
        check(lib.osn_rows_pair_dot(_p(rows), r, d, _p(lo), _p(hi), e, _p(sim), _p(err), _stream(dev)), "osn_rows_pair_dot")
    if own and e > 0:
        regions_check(err)
    return sim


def regions_merge_round(lo, hi, sim, n_regions, threshold, err=None):
    """parent int32 [R]: the smallest member of every region's group after one round of star contraction over the pairs
    (lo[e], hi[e]) with sim[e] >= threshold (float32; NaN and -inf never pass): a region joins its best neighbour --
    greatest sim, then lowest e -- iff they name each other or the neighbour's own best pair is mutual.  Integer atomics and
    the union-find of regions_label: independent of scheduling.  `err` as rows_pair_dot."""
    if not isinstance(sim, torch.Tensor) or sim.dtype != torch.float32:
        raise TypeError("sim must be a float32 tensor")
    dev = sim.device
    lib = _prep(dev)
    e = _merge_pairs(lo, hi, dev)
    if tuple(sim.shape) != (e,) or not sim.is_contiguous():
        raise ValueError("sim must be a contiguous float32 [%d] vector, one per pair" % e)
    r = int(n_regions)
    if not 0 <= r < 2 ** 31:
        raise ValueError("n_regions must lie in 0 .. 2^31 - 1 (got %d)" % r)
    threshold = float(threshold)
    if threshold != threshold or threshold in (float("inf"), float("-inf")):
        raise ValueError("the threshold must be finite (got %r)" % (threshold,))
    err, own = _regions_err(err, dev)
    parent = torch.empty(r, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.osn_merge_ws_bytes(r)) // 8, 1), dtype=torch.int64, device=dev)
    with _Dev(dev):
        check(lib.osn_merge_round(_p(lo), _p(hi), _p(sim), e, r, threshold, _p(parent), _p(err), _p(ws), ws.numel() * 8,
                                  _stream(dev)), "osn_merge_round")
    if own and e > 0 and r > 0:
        regions_check(err)
    return parent


def rows_fold(src, starts, members, err=None):
    """dst float32 [G, d]: row g is the rows ``src[members[starts[g]:starts[g + 1]]]`` added to +0 one after the other, in list
    order, in float32 -- no atomics, the bits are a function of the inputs; an empty group gives zeros.  src float32 [R, d],
    d % 8 == 0, 8 <= d <= BANK_POOL_MAX_DIM; starts int64 [G + 1] on the device, ascending from 0 to L; members int32 [L].
    A member outside [0, R) or a bad starts entry is skipped and recorded in `err` (as rows_pair_dot)."""
    if not isinstance(src, torch.Tensor) or src.dtype != torch.float32:
        raise TypeError("src must be a float32 tensor")
    dev = src.device
    lib = _prep(dev)
    if src.dim() != 2 or not src.is_contiguous():
        raise ValueError("src must be a contiguous [rows, dim] matrix")
    r, d = src.shape
    if d < 8 or d % 8:
        raise ValueError("the feature dim must be a multiple of 8 (got %d)" % d)
    if d > BANK_POOL_MAX_DIM:
        raise ValueError("the feature dim must be at most %d (got %d)" % (BANK_POOL_MAX_DIM, d))
    if not isinstance(starts, torch.Tensor) or starts.dtype != torch.int64 or starts.dim() != 1 or starts.shape[0] < 1 \
            or starts.device != dev or not starts.is_contiguous():
        raise ValueError("starts must be a contiguous int64 [G + 1] vector on the rows' device")
    if not isinstance(members, torch.Tensor) or members.dtype != torch.int32 or members.dim() != 1 or members.device != dev \
            or not members.is_contiguous():
        raise ValueError("members must be a contiguous int32 [L] vector on the rows' device")
    g = starts.shape[0] - 1
    err, own = _regions_err(err, dev)
    dst = torch.empty((g, d), dtype=torch.float32, device=dev)
    with _Dev(dev):
        check(lib.osn_rows_fold(_p(src), r, d, _p(starts), _p(members), members.shape[0], g, _p(dst), _p(err), _stream(dev)),
              "osn_rows_fold")
    if own and g > 0:
        regions_check(err)
    return dst


# ------------------------------------------------------------------- voxelizer
def voxelize_fnv(xyz, T):
    """xyz float64 [N,3] (device), T 4x4 float64 (host, numpy or tensor) ->
    (grid float64 [N,3] shifted integral coords, inds int64 [Nv], inverse int64 [N])."""
    import numpy as np
    dev = xyz.device
    lib = _prep(dev)
    if xyz.dtype != torch.float64:
        raise TypeError("xyz must be float64 (the reference voxelises in float64)")
    xyz = xyz.contiguous()
    n = xyz.shape[0]
    T = np.ascontiguousarray(np.asarray(T, dtype=np.float64))
    t12 = (ctypes.c_double * 12)(*T[:3, :].reshape(-1).tolist())
    grid = torch.empty((max(n, 1), 3), dtype=torch.float64, device=dev)
    inds = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    inverse = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    with _Dev(dev):
        wsb = lib.osn_voxelize_ws_bytes(n)
        ws = _ws(wsb, dev)
        nv = ctypes.c_int64(0)
        check(lib.osn_voxelize_fnv(_p(xyz), n, t12, _p(grid), _p(inds), _p(inverse), ctypes.byref(nv), _p(ws),
                                   ws.numel(), _stream(dev)), "osn_voxelize_fnv")
    return grid[:n], inds[:int(nv.value)], inverse[:n]


def fnv_hash(grid):
    dev = grid.device
    lib = _prep(dev)
    grid = grid.to(torch.float64).contiguous()
    n, ncol = grid.shape
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    with _Dev(dev):
        check(lib.osn_fnv_hash(_p(grid), n, ncol, _p(keys), _stream(dev)), "osn_fnv_hash")
    return keys


def ravel_hash(grid):
    """ravel_hash_vec of an integral float64 [n, ncol <= 4] matrix -> int64 keys (uint64 bit pattern)."""
    dev = grid.device
    lib = _prep(dev)
    grid = grid.to(torch.float64).contiguous()
    n, ncol = grid.shape
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    ws = _ws(128, dev)
    with _Dev(dev):
        check(lib.osn_ravel_hash(_p(grid), n, ncol, _p(keys), _p(ws), ws.numel(), _stream(dev)), "osn_ravel_hash")
    return keys


# ------------------------------------------------------------------ loader
def feature_remap(mask_chunk, vox_ind):
    """mask_chunk bool/uint8 [N_pts], vox_ind int64 [N_vox] (device) ->
    (mask_vox bool [N_vox], src_row int64 [N_vox] (-1 = no feature), indices int64 [n_sel])."""
    dev = vox_ind.device
    lib = _prep(dev)
    if mask_chunk.device != dev:
        raise ValueError("mask_chunk on %s but vox_ind on %s" % (mask_chunk.device, dev))
    if vox_ind.dtype != torch.int64:
        raise TypeError("vox_ind must be int64")
    m8 = mask_chunk.contiguous().view(torch.uint8) if mask_chunk.dtype == torch.bool else mask_chunk.to(torch.uint8).contiguous()
    vox_ind = vox_ind.contiguous()
    n_pts, n_vox = m8.shape[0], vox_ind.shape[0]
    mask_vox = torch.empty(max(n_vox, 1), dtype=torch.uint8, device=dev)
    src_row = torch.empty(max(n_vox, 1), dtype=torch.int64, device=dev)
    indices = torch.empty(max(n_vox, 1), dtype=torch.int64, device=dev)
    with _Dev(dev):
        wsb = lib.osn_feature_remap_ws_bytes(n_pts, n_vox)
        ws = _ws(wsb, dev)
        nsel = ctypes.c_int64(0)
        check(lib.osn_feature_remap(_p(m8), _p(vox_ind), n_pts, n_vox, _p(mask_vox), _p(src_row), _p(indices),
                                    ctypes.byref(nsel), _p(ws), ws.numel(), _stream(dev)), "osn_feature_remap")
    return mask_vox[:n_vox].view(torch.bool), src_row[:n_vox], indices[:int(nsel.value)]


def batch_coords(xyz3, batch_index, out):
    """Write (batch_index, x, y, z) int32 rows of one scene into `out` (a [n, 4] row slice of the batch)."""
    dev = xyz3.device
    lib = _prep(dev)
    if xyz3.dtype != torch.int32 or out.dtype != torch.int32 or not out.is_contiguous():
        raise TypeError("xyz3 and out must be int32, out contiguous")
    xyz3 = xyz3.contiguous()
    n = xyz3.shape[0]
    if out.shape != (n, 4):
        raise ValueError("out must be [%d, 4], got %s" % (n, tuple(out.shape)))
    with _Dev(dev):
        check(lib.osn_batch_coords(_p(xyz3), n, int(batch_index), _p(out), _stream(dev)), "osn_batch_coords")
    return out


# ------------------------------------------------------- multi-view feature fusion
def fusion_project(coords3, world_to_camera, intrinsic4, depth, image_hw, cut_bound, vis_thres):
    """int64 [n, 3] (pixel row, pixel column, visible) of fusion_util.py:93-139; coords3 float64 [n, 3] on the device,
    world_to_camera a 4x4 float64 numpy array (host), intrinsic4 = (fx, fy, cx, cy), depth float64 [H, W] device or None."""
    dev = coords3.device
    lib = _prep(dev)
    if coords3.dtype != torch.float64 or coords3.dim() != 2 or coords3.shape[1] != 3:
        raise TypeError("coords must be float64 [n, 3] (the reference concatenates with a float64 column of ones)")
    coords3 = coords3.contiguous()
    n = coords3.shape[0]
    H, W = int(image_hw[0]), int(image_hw[1])
    if depth is not None:
        if depth.dtype != torch.float64 or tuple(depth.shape) != (H, W):
            raise TypeError("depth must be float64 [%d, %d]" % (H, W))
        depth = depth.contiguous()
    m16 = (ctypes.c_double * 16)(*[float(v) for v in world_to_camera.reshape(-1)])
    i4 = (ctypes.c_double * 4)(*[float(v) for v in intrinsic4])
    mapping = torch.empty((n, 3), dtype=torch.int64, device=dev)
    with _Dev(dev):
        check(lib.osn_fusion_project(_p(coords3), n, m16, i4, _p(depth), H, W, int(cut_bound), float(vis_thres),
                                     _p(mapping), _stream(dev)), "osn_fusion_project")
    return mapping


def fusion_accumulate(feat2d, mapping, sum_features, counter, image_hw=None):
    """One view: counter[p] += 1 and sum_features[p] += feat2d[:, row, col] for the visible points (in place).
    image_hw: the (H, W) the mapping was computed for; a feature map of another size is refused (the reference's
    indexing raises IndexError there).  Without it the kernel still never reads outside feat2d: pixels beyond its
    H x W are skipped."""
    dev = feat2d.device
    lib = _prep(dev)
    feat2d = _f32c(feat2d, "feat_2d")
    D, H, W = feat2d.shape
    if image_hw is not None and (int(image_hw[0]), int(image_hw[1])) != (H, W):
        raise IndexError("feat_2d is %d x %d but the mapping was computed for a %d x %d image" % (H, W, image_hw[0], image_hw[1]))
    if mapping.device != dev or sum_features.device != dev or counter.device != dev:
        raise ValueError("feat_2d, mapping, sum_features and counter must live on one device")
    n = mapping.shape[0]
    if mapping.dtype != torch.int64 or tuple(mapping.shape) != (n, 3):
        raise TypeError("mapping must be an int64 [n, 3] tensor")
    mapping = mapping.contiguous()
    if (sum_features.dtype != torch.float32 or tuple(sum_features.shape) != (n, D) or not sum_features.is_contiguous()
            or counter.dtype != torch.float32 or counter.numel() != n or not counter.is_contiguous()):
        raise TypeError("sum_features must be contiguous float32 [n, D] and counter contiguous float32 [n] / [n, 1]")
    with _Dev(dev):
        check(lib.osn_fusion_accumulate(_p(feat2d), D, H, W, _p(mapping), n, _p(sum_features), _p(counter), _stream(dev)),
              "osn_fusion_accumulate")


def fusion_finish(sum_features, counter):
    dev = sum_features.device
    lib = _prep(dev)
    n, D = sum_features.shape
    bank = torch.empty_like(sum_features)
    with _Dev(dev):
        check(lib.osn_fusion_finish(_p(sum_features), _p(counter), n, D, _p(bank), _stream(dev)), "osn_fusion_finish")
    return bank


# ------------------------------------------------------- scene views: splat rasteriser and shading (csrc/render.hip)
RENDER_MAX_PX = 16                      # the largest footprint radius in pixels (csrc/render.hip)
RENDER_BACKGROUND = -1                  # a zbuf word nothing was drawn on: all ones
_SHADE_MODES = {None: 0, "colors": 1, "labels": 2, "heat": 3}


def _rgb_word(c, name):
    c = tuple(int(v) for v in c)
    if len(c) != 3 or not all(0 <= v <= 255 for v in c):
        raise ValueError("%s must be three integers in 0 .. 255 (got %r)" % (name, c))
    return c[0] | c[1] << 8 | c[2] << 16


def _rgb_rows(t, rows, name, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise TypeError("%s must be a uint8 tensor" % name)
    if t.dim() != 2 or t.shape[1] != 3 or (rows is not None and t.shape[0] != rows) or t.device != dev or not t.is_contiguous():
        raise ValueError("%s must be a contiguous uint8 [%s, 3] matrix on the z-buffer's device" % (name, "rows" if rows is None else rows))
    return t


def render_splat(coords3, world_to_camera, intrinsics, image_hw, radius=0.02, max_px=4, near=0.05):
    """zbuf int64 [V, H, W]: per pixel the 64-bit unsigned minimum, over the points whose footprint covers it, of
    (bits of float32(depth) << 32 | point index), held as the int64 of the same bits; -1 (all ones) is background.
    coords3 float64 [n, 3] on the device (as fusion_project takes them); world_to_camera float64 [V, 4, 4] and intrinsics
    (fx, fy, cx, cy) [V, 4] numpy arrays on the host.  The centre pixel is bit for bit fusion_project's; the footprint is the
    disc of min(max_px, rint(radius * fx / depth)) pixels, clipped to the image.  A pure function of the inputs."""
    import numpy as np
    if not isinstance(coords3, torch.Tensor) or coords3.dtype != torch.float64:
        raise TypeError("coords must be a float64 tensor (the projection is fusion_project's)")
    dev = coords3.device
    if coords3.dim() != 2 or coords3.shape[1] != 3 or not coords3.is_contiguous():
        raise ValueError("coords must be a contiguous float64 [n, 3] matrix")
    n = coords3.shape[0]
    if n >= 2 ** 32 - 1:
        raise ValueError("at most 2^32 - 2 points (got %d)" % n)
    w2c = np.ascontiguousarray(np.asarray(world_to_camera, dtype=np.float64))
    k4 = np.ascontiguousarray(np.asarray(intrinsics, dtype=np.float64))
    if w2c.ndim != 3 or w2c.shape[1:] != (4, 4) or k4.shape != (w2c.shape[0], 4):
        raise ValueError("world_to_camera must be [V, 4, 4] and intrinsics [V, 4] (got %s and %s)" % (w2c.shape, k4.shape))
    V = w2c.shape[0]
    H, W = int(image_hw[0]), int(image_hw[1])
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError("the image must be at least 1 x 1 and below 2^31 pixels (got %d x %d)" % (H, W))
    radius, near, max_px = float(radius), float(near), int(max_px)
    if not 0.0 <= radius < float("inf"):
        raise ValueError("radius must be finite and >= 0 (got %r)" % (radius,))
    if not 0 <= max_px <= RENDER_MAX_PX:
        raise ValueError("max_px must be in 0 .. %d (got %d)" % (RENDER_MAX_PX, max_px))
    if not 0.0 < near < float("inf"):
        raise ValueError("near must be finite and > 0 (got %r)" % (near,))
    lib = _prep(dev)                              # (after the checks: they hold without a device)
    views = np.concatenate([w2c.reshape(V, 16), k4], axis=1).reshape(-1)
    v20 = (ctypes.c_double * max(views.size, 1))(*views.tolist())
    zbuf = torch.empty((V, H, W), dtype=torch.int64, device=dev)
    with _Dev(dev):
        check(lib.osn_render_splat(_p(coords3), n, v20, V, H, W, radius, max_px, near, _p(zbuf), _stream(dev)), "osn_render_splat")
    return zbuf


def render_shade(zbuf, n, mode=None, colors=None, values=None, column=0, table=None, lo=0.0, hi=1.0, other=(255, 0, 255),
                 background=(0, 0, 0)):
    """(point_id int32, depth float32, rgb uint8 [..., 3] or None), each of zbuf's shape: the winning point of every pixel
    (-1: background), its float32 depth (0: background), and its colour by `mode`:
      None      no picture
      "colors"  colors[id]; colors uint8 [n, 3]
      "labels"  table[values[id]]; values int32 / int64 [n], table = palette uint8 [C, 3]; a label outside [0, C): `other`
      "heat"    values fp16 / fp32 [n] or [n, Q] with `column` (read in place through the row stride); table = LUT uint8
                [256, 3]; NaN: `other`; below lo: colors[id] when colors (a base image, uint8 [n, 3]) is given, else table[0];
                else table[min(255, rint((h - lo) / (hi - lo) * 255))] in correctly rounded float32.
    Background pixels get `background`.  n is the number of points the z-buffer was drawn from."""
    if not isinstance(zbuf, torch.Tensor) or zbuf.dtype != torch.int64:
        raise TypeError("zbuf must be the int64 tensor render_splat returns")
    dev = zbuf.device
    if not zbuf.is_contiguous():
        raise ValueError("zbuf must be contiguous")
    n = int(n)
    if not 0 <= n < 2 ** 31:
        raise ValueError("n must be in 0 .. 2^31 - 1 (got %d)" % n)
    if mode not in _SHADE_MODES:
        raise ValueError('mode must be None, "colors", "labels" or "heat" (got %r)' % (mode,))
    P = zbuf.numel()
    vbytes, offset, stride = 0, 0, 1
    lo, hi = float(lo), float(hi)
    if mode == "colors" or (mode == "heat" and colors is not None):
        _rgb_rows(colors, n, "colors", dev)
    elif colors is not None:
        raise ValueError("colors is for the modes \"colors\" and \"heat\"")
    if mode in ("labels", "heat"):
        kinds = {torch.int32: 4, torch.int64: 8} if mode == "labels" else {torch.float16: 2, torch.float32: 4}
        if not isinstance(values, torch.Tensor) or values.dtype not in kinds:
            raise TypeError("%s values must be a tensor of %s" % (mode, " or ".join(str(k) for k in kinds)))
        if values.device != dev:
            raise ValueError("values must live on the z-buffer's device")
        vbytes = kinds[values.dtype]
        column = int(column)
        if values.dim() == 1 and column == 0 and values.shape[0] == n:
            stride = values.stride(0) if n > 1 else 1
        elif mode == "heat" and values.dim() == 2 and values.shape[0] == n and 0 <= column < values.shape[1]:
            stride = values.stride(0) if n > 1 else 1
            if values.stride(1) != 1 and values.shape[1] > 1:
                raise ValueError("the heat rows must be contiguous")
            offset = column
        else:
            raise ValueError("values must be [%d]%s (got %s, column %d)" % (n, " or [%d, Q] with a column in range" % n if mode == "heat" else "",
                                                                             tuple(values.shape), column))
        if stride < 1:
            raise ValueError("the values' row stride must be positive")
        _rgb_rows(table, 256 if mode == "heat" else None, "the LUT" if mode == "heat" else "the palette", dev)
        if mode == "heat" and not (lo < hi and hi - lo < float("inf") and torch.tensor(hi, dtype=torch.float32).item() >
                                   torch.tensor(lo, dtype=torch.float32).item()):
            raise ValueError("need finite lo < hi, distinct in float32 (got %r, %r)" % (lo, hi))
    elif values is not None or table is not None:
        raise ValueError("values and table are for the modes \"labels\" and \"heat\"")
    other, background = _rgb_word(other, "other"), _rgb_word(background, "background")
    lib = _prep(dev)                              # (after the checks: they hold without a device)
    point_id = torch.empty(zbuf.shape, dtype=torch.int32, device=dev)
    depth = torch.empty(zbuf.shape, dtype=torch.float32, device=dev)
    rgb = None if mode is None else torch.empty(tuple(zbuf.shape) + (3,), dtype=torch.uint8, device=dev)
    with _Dev(dev):
        check(lib.osn_render_shade(_p(zbuf), P, n, _p(point_id), _p(depth), _p(rgb), _SHADE_MODES[mode], _p(colors), _p(values), vbytes,
                                   offset, stride, _p(table), 0 if table is None else table.shape[0], lo, hi,
                                   other, background, _stream(dev)), "osn_render_shade")
    return point_id, depth, rgb


# ------------------------------------------------------------------- neighbours
KNN_MAX_K = 16
KNN_E_ORDER, KNN_E_CELL, KNN_E_POINT, KNN_E_NEIGHBOR = 1, 2, 4, 8      # the bits of the err word (csrc/neighbors.hip)


def knn_check(err):
    """Raise if a neighbour call recorded an entry out of range in `err` (int32 [1]); zeroes the word.  Synchronises."""
    bits = int(err.item())
    if bits == 0:
        return
    err.zero_()
    what = [text for bit, text in ((KNN_E_ORDER, "an order entry outside [0, M)"),
                                   (KNN_E_CELL, "a cell column or a table entry out of range"),
                                   (KNN_E_POINT, "a cell's list range or point out of range"),
                                   (KNN_E_NEIGHBOR, "a neighbour index or count out of range")) if bits & bit]
    raise _lib.OpenSceneAmdError("neighbours: %s (err bits %d); such entries were skipped" % ("; ".join(what) or "unknown error", bits))


def _knn_vec(t, name, dtype, shape, dev, optional=False):
    if t is None and optional:
        return
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise TypeError("%s must be a %s tensor" % (name, str(dtype).replace("torch.", "")))
    if tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s %s tensor on the points' device" % (name, str(dtype).replace("torch.", ""), list(shape)))


def knn_k(k):
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError("k must be in 1 .. %d (got %d)" % (KNN_MAX_K, k))
    return k


def knn_grid(xyz, cell_start, cell_points, nbr, query_xyz, q_cell, k, r2, exclude=None, order=None, err=None):
    """The k nearest source points of every query inside the 27 cells around it.
    xyz float32 [N, 3] the grid's points; cell_start int32 [V + 1] / cell_points int32 [n_src]: the CSR of the SOURCE points
    per voxel row; nbr int32 [27, C] the voxel rows around each cell column (-1 absent); query_xyz float32 [M, 3]; q_cell
    int32 [M] the column of each query (-1: no neighbours); exclude int32 [M] a point never returned, or None; order int32
    [M] the sequence the lanes take the queries in (cell order), or None; 1 <= k <= 16; r2 the float32 squared radius.
    -> (idx int32 [M, k] (-1 past count), dist2 float32 [M, k] (+inf past count), count int32 [M]): ascending (d2, index)
    over the candidates with d2 <= r2, d2 from separately rounded float32 operations.  Exact and bitwise repeatable.  An
    entry out of range is skipped and recorded in `err` when one is given (knn_check raises), and checked here otherwise."""
    if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float32:
        raise TypeError("xyz must be a float32 tensor")
    dev = xyz.device
    if xyz.dim() != 2 or xyz.shape[1] != 3 or not xyz.is_contiguous():
        raise ValueError("xyz must be a contiguous float32 [N, 3] matrix")
    n = xyz.shape[0]
    if not isinstance(cell_start, torch.Tensor) or cell_start.dtype != torch.int32:
        raise TypeError("cell_start must be an int32 tensor")
    if cell_start.dim() != 1 or cell_start.shape[0] < 1 or cell_start.device != dev or not cell_start.is_contiguous():
        raise ValueError("cell_start must be a contiguous int32 [V + 1] vector on the points' device")
    v = cell_start.shape[0] - 1
    if not isinstance(cell_points, torch.Tensor) or cell_points.dtype != torch.int32:
        raise TypeError("cell_points must be an int32 tensor")
    if cell_points.dim() != 1 or cell_points.shape[0] > n or cell_points.device != dev or not cell_points.is_contiguous():
        raise ValueError("cell_points must be a contiguous int32 vector of at most %d entries on the points' device" % n)
    if not isinstance(nbr, torch.Tensor) or nbr.dtype != torch.int32:
        raise TypeError("nbr must be an int32 tensor")
    if nbr.dim() != 2 or nbr.shape[0] != 27 or nbr.device != dev or not nbr.is_contiguous():
        raise ValueError("nbr must be a contiguous int32 [27, C] table on the points' device")
    if not isinstance(query_xyz, torch.Tensor) or query_xyz.dtype != torch.float32:
        raise TypeError("query_xyz must be a float32 tensor")
    if query_xyz.dim() != 2 or query_xyz.shape[1] != 3 or query_xyz.device != dev or not query_xyz.is_contiguous():
        raise ValueError("query_xyz must be a contiguous float32 [M, 3] matrix on the points' device")
    m = query_xyz.shape[0]
    if m >= (1 << 31) // KNN_MAX_K:
        raise ValueError("fewer than 2^27 queries per call (got %d)" % m)
    _knn_vec(q_cell, "q_cell", torch.int32, (m,), dev)
    _knn_vec(exclude, "exclude", torch.int32, (m,), dev, optional=True)
    _knn_vec(order, "order", torch.int32, (m,), dev, optional=True)
    k = knn_k(k)
    r2 = float(r2)
    if not (r2 >= 0.0 and r2 != float("inf")):
        raise ValueError("r2 must be finite and >= 0 (got %r)" % (r2,))
    err, own = _regions_err(err, dev)
    lib = _prep(dev)                              # (after the checks: they hold without a device)
    idx = torch.empty((m, k), dtype=torch.int32, device=dev)
    dist2 = torch.empty((m, k), dtype=torch.float32, device=dev)
    count = torch.empty(m, dtype=torch.int32, device=dev)
    with _Dev(dev):
        check(lib.osn_knn_grid(_p(xyz), n, _p(cell_start), _p(cell_points), cell_points.shape[0], v, _p(nbr), nbr.shape[1],
                               _p(query_xyz), _p(q_cell), _p(exclude), _p(order), m, k, r2, _p(idx), _p(dist2), _p(count), _p(err),
                               _stream(dev)), "osn_knn_grid")
    if own and m > 0:
        knn_check(err)
    return idx, dist2, count


def knn_blend(values, idx, dist2, count, inverse=False, eps=0.0, fill=0.0, err=None):
    """Blend rows of `values` along neighbour lists: out[m] = sum_j w_j values[idx[m, j]] / sum_j w_j over j < count[m] in
    ascending j, w_j = 1 or (inverse) 1 / (dist2[m, j] + eps); float32 products, sums and divide, rounded once to the values'
    type.  values fp16 / fp32 [N, C], C >= 1; idx int32 [M, k], dist2 float32 [M, k], count int32 [M] as knn_grid returns
    them.  -> (out [M, C] in the values' type, found bool [M]); count == 0 gives `fill` and found False.  k = 1 without
    inverse copies the row bit for bit.  `err` as knn_grid."""
    if not isinstance(values, torch.Tensor) or values.dtype not in (torch.float16, torch.float32):
        raise TypeError("values must be a float16 or float32 tensor (got %s)"
                        % (values.dtype if isinstance(values, torch.Tensor) else type(values).__name__))
    dev = values.device
    if values.dim() != 2 or values.shape[1] < 1 or not values.is_contiguous():
        raise ValueError("values must be a contiguous [N, C] matrix with C >= 1")
    n, c = values.shape
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32:
        raise TypeError("idx must be an int32 tensor")
    if idx.dim() != 2 or idx.device != dev or not idx.is_contiguous():
        raise ValueError("idx must be a contiguous int32 [M, k] matrix on the values' device")
    m, k = idx.shape
    k = knn_k(k)
    if m >= (1 << 31) // KNN_MAX_K:
        raise ValueError("fewer than 2^27 queries per call (got %d)" % m)
    _knn_vec(dist2, "dist2", torch.float32, (m, k), dev)
    _knn_vec(count, "count", torch.int32, (m,), dev)
    eps, fill = float(eps), float(fill)
    if inverse and not (eps > 0.0 and eps != float("inf")):
        raise ValueError("inverse weights need a finite eps > 0 (got %r)" % (eps,))
    err, own = _regions_err(err, dev)
    lib = _prep(dev)
    out = torch.empty((m, c), dtype=values.dtype, device=dev)
    found = torch.empty(m, dtype=torch.bool, device=dev)
    with _Dev(dev):
        check(lib.osn_knn_blend(_p(values), values.element_size(), n, c, _p(idx), _p(dist2), _p(count), m, k, int(bool(inverse)), eps,
                                fill, _p(out), _p(found), _p(err), _stream(dev)), "osn_knn_blend")
    if own and m > 0:
        knn_check(err)
    return out, found


def knn_vote(labels, idx, count, fill=-1, err=None):
    """The label most of a query's neighbours hold.  labels int64 [N] (negative: ignored); idx int32 [M, k], count int32 [M].
    -> int64 [M]: a tie goes to the label whose first holder is nearest (the smallest j); `fill` without a labelled
    neighbour.  Exact.  `err` as knn_grid."""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64:
        raise TypeError("labels must be an int64 tensor")
    dev = labels.device
    if labels.dim() != 1 or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous int64 [N] vector")
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32:
        raise TypeError("idx must be an int32 tensor")
    if idx.dim() != 2 or idx.device != dev or not idx.is_contiguous():
        raise ValueError("idx must be a contiguous int32 [M, k] matrix on the labels' device")
    m, k = idx.shape
    k = knn_k(k)
    if m >= (1 << 31) // KNN_MAX_K:
        raise ValueError("fewer than 2^27 queries per call (got %d)" % m)
    _knn_vec(count, "count", torch.int32, (m,), dev)
    fill = int(fill)
    err, own = _regions_err(err, dev)
    lib = _prep(dev)
    out = torch.empty(m, dtype=torch.int64, device=dev)
    with _Dev(dev):
        check(lib.osn_knn_vote(_p(labels), labels.shape[0], _p(idx), _p(count), m, k, fill, _p(out), _p(err), _stream(dev)), "osn_knn_vote")
    if own and m > 0:
        knn_check(err)
    return out


# ------------------------------------------------------- nearest sources at any range (csrc/reach.hip)
REACH_MAX = 4096
REACH_ITEM = 256                     # queries per work item: one workgroup, one query per lane
REACH_E_ITEM, REACH_E_BLOCK, REACH_E_CELL, REACH_E_ORDER = 1, 2, 4, 8      # the bits of the err word (csrc/reach.hip)


def reach_check(err):
    """Raise if ops.reach_nearest recorded an entry out of range in `err` (int32 [1]); zeroes the word.  Synchronises."""
    bits = int(err.item())
    if bits == 0:
        return
    err.zero_()
    what = [text for bit, text in ((REACH_E_ITEM, "a work item's ranges out of range"),
                                   (REACH_E_BLOCK, "a block's entry range or coordinates out of range"),
                                   (REACH_E_CELL, "a cell outside the packable range |c| < 32767"),
                                   (REACH_E_ORDER, "an order entry outside [0, C)")) if bits & bit]
    raise _lib.OpenSceneAmdError("reach: %s (err bits %d); such entries were skipped" % ("; ".join(what) or "unknown error", bits))


def reach_value(reach):
    if isinstance(reach, bool) or not hasattr(reach, "__index__") or isinstance(reach, torch.Tensor):
        raise TypeError("reach must be an int (got %s)" % type(reach).__name__)
    reach = int(reach)
    if not 1 <= reach <= REACH_MAX:
        raise ValueError("reach must be in 1 .. %d cells (got %d)" % (REACH_MAX, reach))
    return reach


def _reach_block_key(cells):
    """int64 [R]: (scene, bx, by, bz) of int32 [R, 4] rows as one ascending key; block = cell >> 3, an arithmetic shift."""
    c = cells.long()
    b = (c[:, 1:] >> 3) + 4096                               # 13 bits per axis for |cell| < 32767
    return ((c[:, 0] * 8192 + b[:, 0]) * 8192 + b[:, 1]) * 8192 + b[:, 2]


def reach_plan(query_cells, source_cells, source_ids):
    """The sorted arrays osn_reach_nearest takes (include/openscene_amd.h), in torch: (q_sorted int32 [C, 4], order int32 [C],
    items int32 [W, 4], src int32 [S, 4] rows (x, y, z, id), blocks int32 [B, 4], block_start int32 [B + 1]).  Queries and
    sources are sorted by (scene, block); the items are runs of at most REACH_ITEM sorted queries cut at scene boundaries,
    each with the range of its scene's blocks."""
    dev = query_cells.device
    i32 = dict(dtype=torch.int32, device=dev)
    order = torch.sort(_reach_block_key(query_cells), stable=True)[1]
    q_sorted = query_cells[order].contiguous()
    s_key, s_perm = torch.sort(_reach_block_key(source_cells), stable=True)
    s_cells = source_cells[s_perm]
    src = torch.cat([s_cells[:, 1:], source_ids[s_perm][:, None]], 1).contiguous()
    _keys, per_block = torch.unique_consecutive(s_key, return_counts=True)
    block_start = torch.zeros(per_block.shape[0] + 1, dtype=torch.int64, device=dev)
    block_start[1:] = torch.cumsum(per_block, 0)
    first = s_cells[block_start[:-1]]
    blocks = torch.cat([first[:, :1], first[:, 1:] >> 3], 1).contiguous()
    scenes, per_scene = torch.unique_consecutive(q_sorted[:, 0], return_counts=True)
    scene_end = torch.cumsum(per_scene, 0)
    scene_start = scene_end - per_scene
    per_scene_items = (per_scene + REACH_ITEM - 1) // REACH_ITEM
    item_first = torch.cumsum(per_scene_items, 0) - per_scene_items
    seg = torch.repeat_interleave(torch.arange(scenes.shape[0], device=dev), per_scene_items)
    q_start = scene_start[seg] + (torch.arange(seg.shape[0], device=dev) - item_first[seg]) * REACH_ITEM
    q_end = torch.minimum(q_start + REACH_ITEM, scene_end[seg])
    block_scene = blocks[:, 0].contiguous()
    item_scene = scenes[seg].contiguous()
    b_start = torch.searchsorted(block_scene, item_scene, right=False)
    b_end = torch.searchsorted(block_scene, item_scene, right=True)
    items = torch.stack([q_start, q_end, b_start, b_end], 1).to(torch.int32).contiguous()
    return q_sorted, order.to(torch.int32).contiguous(), items, src, blocks, block_start.to(torch.int32).contiguous()


def reach_nearest(query_cells, source_cells, source_ids, reach, err=None):
    """For every query cell the nearest source cell of the same scene inside a Euclidean ball of `reach` cells, exactly.
    query_cells int32 [C, 4] rows (scene, x, y, z); source_cells int32 [S, 4]; source_ids int32 [S] (>= 0); reach an int in
    1 .. 4096.  The candidates of a query are the sources of its scene with |dx|, |dy|, |dz| <= reach and
    d2 = dx^2 + dy^2 + dz^2 <= reach^2; the result is the minimum of the key uint32(d2) << 32 | uint32(id) over them.
    -> (nearest int32 [C]: the id, dist2 int32 [C]: its d2), both -1 without a candidate; a tie in d2 goes to the lowest id.
    Integers only: exact, and two calls give the same bits.  Cells lie in |c| < 32767; one outside is skipped and recorded
    in `err` when one is given (reach_check raises), and checked here otherwise.  The sort by (scene, 8^3 block) and the
    work items are torch (reach_plan); the search is csrc/reach.hip."""
    for t, name in ((query_cells, "query_cells"), (source_cells, "source_cells")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
            raise TypeError("%s must be an int32 tensor" % name)
        if t.dim() != 2 or t.shape[1] != 4:
            raise ValueError("%s must be int32 [R, 4] rows (scene, x, y, z) (got %s)" % (name, tuple(t.shape)))
    dev = query_cells.device
    if source_cells.device != dev:
        raise ValueError("source_cells must be on the queries' device (%s, got %s)" % (dev, source_cells.device))
    if not isinstance(source_ids, torch.Tensor) or source_ids.dtype != torch.int32:
        raise TypeError("source_ids must be an int32 tensor")
    c, s = query_cells.shape[0], source_cells.shape[0]
    if tuple(source_ids.shape) != (s,) or source_ids.device != dev:
        raise ValueError("source_ids must be an int32 [%d] vector on the queries' device" % s)
    if c >= 1 << 31 or s >= 1 << 31:
        raise ValueError("fewer than 2^31 cells per call")
    reach = reach_value(reach)
    err, own = _regions_err(err, dev)
    _prep(dev)                                    # (after the checks: they hold without a device)
    if c == 0 or s == 0:
        none = torch.full((c,), -1, dtype=torch.int32, device=dev)
        return none, none.clone()
    nearest, dist2 = reach_run(reach_plan(query_cells, source_cells, source_ids), reach, err)
    if own:
        reach_check(err)
    return nearest, dist2


def reach_run(plan, reach, err):
    """The search over a reach_plan (the kernel alone: what tools/micro_reach.py times) -> (nearest, dist2); `err` is required
    and not read here."""
    q_sorted, order, items, src, blocks, block_start = plan
    dev, c = q_sorted.device, q_sorted.shape[0]
    lib = _prep(dev)
    dist2 = torch.full((c,), -1, dtype=torch.int32, device=dev)           # (a query no item names keeps -1)
    nearest = torch.full((c,), -1, dtype=torch.int32, device=dev)
    with _Dev(dev):
        check(lib.osn_reach_nearest(_p(q_sorted), _p(order), c, _p(items), items.shape[0], _p(src), src.shape[0], _p(blocks),
                                    _p(block_start), blocks.shape[0], reach_value(reach), _p(dist2), _p(nearest), _p(err), _stream(dev)),
              "osn_reach_nearest")
    return nearest, dist2


# ------------------------------------------------------- two scans in one frame: rigid RANSAC, moments (csrc/align.hip)
RIGID_MAX_HYPOTHESES = 1 << 20       # OSN_RIGID_MAX_HYPOTHESES
RIGID_MOMENTS_CHUNK = 1024           # OSN_RIGID_MOMENTS_CHUNK: the pairs that are reduced into one float64 partial


def _rigid_pairs(src, dst):
    if not isinstance(src, torch.Tensor) or src.dtype != torch.float32:
        raise TypeError("src must be a float32 tensor")
    if src.dim() != 2 or src.shape[1] != 3 or not src.is_contiguous():
        raise ValueError("src must be a contiguous float32 [P, 3] matrix (got %s)" % (tuple(src.shape),))
    if not isinstance(dst, torch.Tensor) or dst.dtype != torch.float32:
        raise TypeError("dst must be a float32 tensor")
    if dst.dim() != 2 or dst.shape[1] != 3 or not dst.is_contiguous() or dst.device != src.device:
        raise ValueError("dst must be a contiguous float32 [N, 3] matrix on src's device (got %s)" % (tuple(dst.shape),))
    if src.shape[0] >= 1 << 31 or dst.shape[0] >= 1 << 31:
        raise ValueError("fewer than 2^31 pairs per call")
    return src.device, src.shape[0]


def _rigid_xf(xf, dev):
    if not isinstance(xf, torch.Tensor) or xf.dtype != torch.float32:
        raise TypeError("xf must be a float32 tensor")
    if xf.dim() != 2 or xf.shape[1] != 12 or xf.device != dev or not xf.is_contiguous():
        raise ValueError("xf must be a contiguous float32 [H, 12] matrix on the pairs' device (got %s)" % (tuple(xf.shape),))
    if xf.shape[0] > RIGID_MAX_HYPOTHESES:
        raise ValueError("at most %d hypotheses per call (got %d)" % (RIGID_MAX_HYPOTHESES, xf.shape[0]))
    return xf.shape[0]


def _rigid_level(v, name):
    v = float(v)
    if not (v >= 0.0 and v != float("inf")):
        raise ValueError("%s must be finite and >= 0 (got %r)" % (name, v))
    return v


def rigid_from_triplets(src, dst, triplets, threshold, area2_min=0.0):
    """The rigid motion of every triplet of pairs.  src, dst float32 [P, 3]; triplets int32 [H, 3] on their device: three
    pair numbers each.  -> (xf float32 [H, 12]: R row-major then t, the motion that takes the src triangle onto the dst
    triangle, in separately rounded float64 operations rounded once to float32; valid bool [H]).  Invalid -- identity, valid
    False -- when a number lies outside [0, P) or two are equal, when a triangle's |a x b|^2 is not > area2_min, or when a side
    differs between the triangles by more than 2 * threshold (include/openscene_amd.h states the order of operations)."""
    dev, p = _rigid_pairs(src, dst)
    if dst.shape[0] != p:
        raise ValueError("src and dst must hold a row per pair (got %d and %d)" % (p, dst.shape[0]))
    if not isinstance(triplets, torch.Tensor) or triplets.dtype != torch.int32:
        raise TypeError("triplets must be an int32 tensor")
    if triplets.dim() != 2 or triplets.shape[1] != 3 or triplets.device != dev or not triplets.is_contiguous():
        raise ValueError("triplets must be a contiguous int32 [H, 3] matrix on the pairs' device (got %s)" % (tuple(triplets.shape),))
    h = triplets.shape[0]
    if h > RIGID_MAX_HYPOTHESES:
        raise ValueError("at most %d hypotheses per call (got %d)" % (RIGID_MAX_HYPOTHESES, h))
    threshold, area2_min = _rigid_level(threshold, "threshold"), _rigid_level(area2_min, "area2_min")
    lib = _prep(dev)
    xf = torch.empty((h, 12), dtype=torch.float32, device=dev)
    valid = torch.empty(h, dtype=torch.bool, device=dev)
    with _Dev(dev):
        check(lib.osn_rigid_from_triplets(_p(src), _p(dst), p, _p(triplets), h, threshold, area2_min, _p(xf), _p(valid), _stream(dev)),
              "osn_rigid_from_triplets")
    return xf, valid


def rigid_score(src, dst, xf, tau2, valid=None):
    """int32 [H]: how many of the P pairs every transform of xf (float32 [H, 12]) moves to within tau2 -- r2 <= tau2 with r2
    the separately rounded float32 residual of include/openscene_amd.h, exact; -1 where valid (bool [H] or None) is False.
    H x P residuals and no temporary."""
    dev, p = _rigid_pairs(src, dst)
    if dst.shape[0] != p:
        raise ValueError("src and dst must hold a row per pair (got %d and %d)" % (p, dst.shape[0]))
    h = _rigid_xf(xf, dev)
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype != torch.bool:
            raise TypeError("valid must be a bool tensor")
        if tuple(valid.shape) != (h,) or valid.device != dev or not valid.is_contiguous():
            raise ValueError("valid must be a contiguous bool [%d] vector on the pairs' device" % h)
    tau2 = _rigid_level(tau2, "tau2")
    lib = _prep(dev)
    counts = torch.empty(h, dtype=torch.int32, device=dev)
    with _Dev(dev):
        check(lib.osn_rigid_score(_p(src), _p(dst), p, _p(xf), _p(valid), h, tau2, _p(counts), _stream(dev)), "osn_rigid_score")
    return counts


def rigid_best(counts):
    """int32 [2] on the device: (the largest of counts int32 [H], H >= 1; the lowest hypothesis that has it)."""
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32:
        raise TypeError("counts must be an int32 tensor")
    if counts.dim() != 1 or not 1 <= counts.shape[0] <= RIGID_MAX_HYPOTHESES or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous int32 [H] vector, 1 <= H <= %d (got %s)" % (RIGID_MAX_HYPOTHESES, tuple(counts.shape)))
    dev = counts.device
    lib = _prep(dev)
    best = torch.empty(2, dtype=torch.int32, device=dev)
    with _Dev(dev):
        check(lib.osn_rigid_best(_p(counts), counts.shape[0], _p(best), _stream(dev)), "osn_rigid_best")
    return best


def rigid_moments(src, dst, xf12, tau2, dst_idx=None):
    """What one transform does to the pairs.  xf12: 12 floats on the host (R row-major, t), taken as float32.  Pair i is
    (src[i], dst[i]) or, with dst_idx int32 [P], (src[i], dst[dst_idx[i]]) -- an index < 0 or >= len(dst) means no partner.
    -> (inlier bool [P], r2 float32 [P] (+inf without a partner), moments float64 [16] on the device: over the inliers n,
    sum s (3), sum d (3), sum s d^T (9, row-major)).  The mask and r2 are the score's, bit for bit; the sums run in a fixed
    order (chunks of RIGID_MOMENTS_CHUNK pairs): two calls give the same bits."""
    dev, p = _rigid_pairs(src, dst)
    n_dst = dst.shape[0]
    if dst_idx is None:
        if n_dst != p:
            raise ValueError("src and dst must hold a row per pair (got %d and %d): pass dst_idx" % (p, n_dst))
    else:
        if not isinstance(dst_idx, torch.Tensor) or dst_idx.dtype != torch.int32:
            raise TypeError("dst_idx must be an int32 tensor")
        if tuple(dst_idx.shape) != (p,) or dst_idx.device != dev or not dst_idx.is_contiguous():
            raise ValueError("dst_idx must be a contiguous int32 [%d] vector on the pairs' device" % p)
    x = [float(v) for v in xf12]
    if len(x) != 12:
        raise ValueError("xf12 holds 12 values: R row-major, then t (got %d)" % len(x))
    x = (ctypes.c_float * 12)(*x)
    tau2 = _rigid_level(tau2, "tau2")
    lib = _prep(dev)
    inlier = torch.empty(p, dtype=torch.bool, device=dev)
    r2 = torch.empty(p, dtype=torch.float32, device=dev)
    moments = torch.empty(16, dtype=torch.float64, device=dev)
    nbytes = _cached("osn_rigid_moments_ws_bytes", p)
    ws = _ws(nbytes, dev)
    with _Dev(dev):
        check(lib.osn_rigid_moments(_p(src), _p(dst), _p(dst_idx), p, n_dst, x, tau2, _p(inlier), _p(r2), _p(moments), _p(ws), ws.numel(),
                                    _stream(dev)), "osn_rigid_moments")
    return inlier, r2, moments


# ------------------------------------------------- supervised segmentation head: cross-entropy, argmax, confusion, votes
def _seg_index(t, name, n, dev):
    if t.dtype != torch.int64 or t.dim() != 1 or t.device != dev or (n is not None and t.shape[0] != n):
        raise ValueError("%s must be an int64 vector%s on the logits' device" % (name, "" if n is None else " of %d entries" % n))
    return t.contiguous()


def seg_loss_fwd(logits, labels, ignore_index=255, rows=None, want_loss=True, want_pred=False, confusion=None, validate=False):
    """-> (loss float32 scalar or None, pred int64 [n_lab] or None, state): cross-entropy with ignore_index over the rows
    `logits[rows]` (all rows when rows is None) against `labels`, their argmax, and `confusion` [c, c] int64 += the counts of
    (pred, label) over the labelled rows.  validate: raise on a label outside [0, c) that is not ignore_index or a rows entry
    outside [0, n) (synchronises).  `state` feeds seg_loss_bwd."""
    dev = logits.device
    lib = _prep(dev)
    if logits.dim() != 2:
        raise ValueError("logits must be a [n, c] matrix")
    logits = _f32c(logits, "logits")
    n, c = logits.shape
    if not 1 <= c <= 256 or n < 1:
        raise ValueError("logits are %s: the kernels take 1 <= c <= 256 classes and at least one row" % (tuple(logits.shape),))
    if rows is not None:
        rows = _seg_index(rows, "rows", None, dev)
    n_lab = n if rows is None else rows.shape[0]
    labels = _seg_index(labels, "labels", n_lab, dev)
    if confusion is not None and (confusion.dtype != torch.int64 or tuple(confusion.shape) != (c, c) or confusion.device != dev
                                  or not confusion.is_contiguous()):
        raise ValueError("confusion must be a contiguous int64 [%d, %d] matrix on the logits' device" % (c, c))
    state = torch.empty(int(_cached("osn_seg_loss_state_bytes", n_lab, c)), dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev) if want_loss else None
    pred = torch.empty(n_lab, dtype=torch.int64, device=dev) if want_pred else None
    with _Dev(dev):
        check(lib.osn_seg_loss_fwd(_p(logits), _p(rows), _p(labels), n, n_lab, c, int(ignore_index), _p(loss), _p(pred), _p(confusion),
                                   _p(state), state.numel(), _stream(dev)), "osn_seg_loss_fwd")
        if validate:
            check(lib.osn_seg_loss_check(_p(state), n, n_lab, c, _stream(dev)), "osn_seg_loss_check")
    return loss, pred, state


def seg_loss_bwd(logits, labels, state, ignore_index=255, gloss=None):
    """d loss / d logits [n, c] of seg_loss_fwd (rows = None) times gloss (a float32 device scalar, None = 1)."""
    dev = logits.device
    lib = _prep(dev)
    logits = _f32c(logits, "logits")
    n, c = logits.shape
    labels = _seg_index(labels, "labels", n, dev)
    if gloss is not None:
        gloss = gloss.to(device=dev, dtype=torch.float32).contiguous()
    glogits = torch.empty_like(logits)
    with _Dev(dev):
        check(lib.osn_seg_loss_bwd(_p(logits), _p(labels), _p(gloss), n, c, int(ignore_index), _p(glogits), _p(state), state.numel(),
                                   _stream(dev)), "osn_seg_loss_bwd")
    return glogits


def seg_vote(logits, votes, rows=None):
    """votes [n_pts, c] += logits[rows] (logits itself when rows is None), in place -- run/eval_mink.py:210's `store = pred +
    store` on the device.  A rows entry outside [0, n) adds nothing."""
    dev = logits.device
    lib = _prep(dev)
    logits = _f32c(logits, "logits")
    n, c = logits.shape
    if rows is not None:
        rows = _seg_index(rows, "rows", None, dev)
    n_pts = n if rows is None else rows.shape[0]
    if votes.dtype != torch.float32 or tuple(votes.shape) != (n_pts, c) or votes.device != dev or not votes.is_contiguous():
        raise ValueError("votes must be a contiguous float32 [%d, %d] matrix on the logits' device" % (n_pts, c))
    with _Dev(dev):
        check(lib.osn_seg_vote(_p(logits), _p(rows), n, n_pts, c, _p(votes), _stream(dev)), "osn_seg_vote")
    return votes


# ------------------------------------------------------- elastic distortion (Point3DLoader's pre-voxeliser transform)
def _xyz64(xyz, name="xyz"):
    if xyz.dtype != torch.float64:
        raise TypeError("%s must be float64 (the reference distorts in float64), got %s" % (name, xyz.dtype))
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("%s must be [n, 3], got %s" % (name, tuple(xyz.shape)))
    if not xyz.is_contiguous():
        raise ValueError("%s must be contiguous" % name)


def bbox(xyz):
    """float64 [6] on the device: per-axis min of a float64 [n, 3] cloud, then per-axis max (``coords.min(0)``,
    ``coords.max(0)``).  An empty cloud raises, as numpy's min does."""
    dev = xyz.device
    lib = _prep(dev)
    _xyz64(xyz)
    n = xyz.shape[0]
    out = torch.empty(6, dtype=torch.float64, device=dev)
    with _Dev(dev):
        ws = _ws(lib.osn_bbox_ws_bytes(n), dev)
        check(lib.osn_bbox(_p(xyz), n, _p(out), _p(ws), ws.numel(), _stream(dev)), "osn_bbox")
    return out


def elastic_blur(noise):
    """The six ``scipy.ndimage.convolve`` box-filter passes of augmentation.py:181-185, in place on a contiguous float32
    [nx, ny, nz, 3] device grid (bit-identical)."""
    dev = noise.device
    lib = _prep(dev)
    if noise.dtype != torch.float32 or noise.dim() != 4 or noise.shape[3] != 3 or not noise.is_contiguous():
        raise ValueError("noise must be a contiguous float32 [nx, ny, nz, 3] grid")
    nx, ny, nz = (int(s) for s in noise.shape[:3])
    with _Dev(dev):
        ws = _ws(lib.osn_elastic_blur_ws_bytes(nx, ny, nz), dev)
        check(lib.osn_elastic_blur(_p(noise), nx, ny, nz, _p(ws), ws.numel(), _stream(dev)), "osn_elastic_blur")
    return noise


def elastic_apply(xyz, noise, axes, magnitude):
    """xyz + RegularGridInterpolator(axes, noise, bounds_error=0, fill_value=0)(xyz) * magnitude (augmentation.py:188-194,
    bit-identical), and the bounding box of the result (float64 [6], device).  noise: float32 [nx, ny, nz, 3] device grid;
    axes: three ascending float64 node arrays (host) of nx, ny, nz >= 2 nodes.  -> (out float64 [n, 3], bbox6)."""
    import numpy as np
    dev = xyz.device
    lib = _prep(dev)
    _xyz64(xyz)
    if noise.dtype != torch.float32 or noise.dim() != 4 or noise.shape[3] != 3 or not noise.is_contiguous():
        raise ValueError("noise must be a contiguous float32 [nx, ny, nz, 3] grid")
    dims = tuple(int(s) for s in noise.shape[:3])
    axes = [np.asarray(a, dtype=np.float64) for a in axes]
    if tuple(a.shape[0] for a in axes) != dims:
        raise ValueError("axes of %s nodes for a %s grid" % ([a.shape[0] for a in axes], dims))
    ax = torch.from_numpy(np.concatenate(axes)).to(dev)
    n = xyz.shape[0]
    out = torch.empty((n, 3), dtype=torch.float64, device=dev)
    box = torch.empty(6, dtype=torch.float64, device=dev)
    with _Dev(dev):
        ws = _ws(lib.osn_elastic_apply_ws_bytes(n), dev)
        check(lib.osn_elastic_apply(_p(xyz), n, _p(noise), dims[0], dims[1], dims[2], _p(ax), float(magnitude), _p(out),
                                    _p(box), _p(ws), ws.numel(), _stream(dev)), "osn_elastic_apply")
    return out, box


def elastic_distort(xyz, granularity, magnitude, bbox6=None, return_bbox=False):
    """One field of ElasticDistortion.elastic_distortion (augmentation.py:159-194) on a float64 [n, 3] device cloud,
    bit-identical to numpy / scipy.  The noise is drawn on the host from ``numpy.random`` exactly as the reference draws it
    (the grid size comes from the cloud's bounding box: its 6 doubles are the one read-back of a field) and the axes come
    from ``np.linspace`` on the host; the blur and the interpolation run on the device.
    bbox6: the cloud's bounding box if already known (the previous field's ``return_bbox``), else computed here.
    -> out float64 [n, 3] (a new tensor), or (out, bbox6 of out) with return_bbox."""
    import numpy as np
    _xyz64(xyz)
    dev = xyz.device
    if bbox6 is None:
        bbox6 = bbox(xyz)
    b = bbox6.cpu().numpy()
    coords_min, coords_max = b[:3], b[3:]
    noise_dim = ((coords_max - coords_min) // granularity).astype(int) + 3     # == (coords - coords_min).max(0) // g
    noise = np.random.randn(*noise_dim, 3).astype(np.float32)
    axes = [np.linspace(d_min, d_max, d)
            for d_min, d_max, d in zip(coords_min - granularity, coords_min + granularity * (noise_dim - 2), noise_dim)]
    grid = elastic_blur(torch.from_numpy(noise).to(dev))
    out, box = elastic_apply(xyz, grid, axes, magnitude)
    return (out, box) if return_bbox else out


# ------------------------------------------------------------ pooling layers
GPOOL_CHUNK = 512                # OSN_GPOOL_CHUNK: the rows of a batch that are reduced into one fp32 partial
POOL_MODES = ("sum", "avg", "max")          # the `mode` word of osn_pool_* / osn_gpool_*: the position in this tuple
BROADCAST_OPS = ("add", "mul")              # the `op` word of osn_broadcast_fwd


def _pool_mode(mode):
    if mode not in POOL_MODES:
        raise ValueError("pooling mode %r (one of %s)" % (mode, ", ".join(POOL_MODES)))
    return POOL_MODES.index(mode)


def _pool_table(nbr, rows, name):
    if nbr.dtype != torch.int32 or nbr.dim() != 2 or (rows is not None and nbr.shape[1] != rows):
        raise TypeError("%s must be an int32 [K, %s] neighbour table" % (name, "rows" if rows is None else rows))
    if nbr.shape[0] not in (8, 27):
        raise ValueError("%s has %d offsets; pooling takes the 8 of a 2^3 kernel or the 27 of a 3^3 kernel" % (name, nbr.shape[0]))
    return nbr if nbr.is_contiguous() else nbr.contiguous()


def _pool_vec(t, name, dtype, n, dev):
    if t.dtype != dtype or t.dim() != 1 or t.shape[0] != n or t.device != dev:
        raise TypeError("%s must be %s [%d] on %s" % (name, dtype, n, dev))
    return t if t.is_contiguous() else t.contiguous()


def _pool_feats(t, name, rows=None):
    if t.dim() != 2 or t.shape[1] < 1 or (rows is not None and t.shape[0] != rows):
        raise ValueError("%s must be a [%s, c >= 1] matrix (got %s)" % (name, "rows" if rows is None else rows, tuple(t.shape)))
    return _f32c(t, name)


def pool_count(nbr, n_in):
    """int32 [n_out]: the present neighbours of every output row of the table nbr [K, n_out] over n_in input rows."""
    dev = nbr.device
    lib = _prep(dev)
    nbr = _pool_table(nbr, None, "nbr")
    K, n_out = nbr.shape
    cnt = torch.empty(n_out, dtype=torch.int32, device=dev)
    with _Dev(dev):
        check(lib.osn_pool_count(_p(nbr), int(n_in), n_out, K, _p(cnt), _stream(dev)), "osn_pool_count")
    return cnt


def pool_fwd(x, nbr, mode):
    """Local pooling of x [n_in, c] over nbr [K, n_out] -> (y [n_out, c], arg int32 [n_out, c] for "max", else None)."""
    m = _pool_mode(mode)
    dev = x.device
    lib = _prep(dev)
    x = _pool_feats(x, "x")
    nbr = _pool_table(nbr, None, "nbr")
    (n_in, c), (K, n_out) = x.shape, nbr.shape
    y = torch.empty((n_out, c), dtype=torch.float32, device=dev)
    arg = torch.empty((n_out, c), dtype=torch.int32, device=dev) if mode == "max" else None
    with _Dev(dev):
        check(lib.osn_pool_fwd(_p(x), n_in, _p(nbr), n_out, K, c, m, _p(y), _p(arg), _stream(dev)), "osn_pool_fwd")
    return y, arg


def pool_bwd(gy, nbr_bwd, flip, mode, cnt=None, arg=None):
    """Input gradient [n_in, c] of pool_fwd from gy [n_out, c] through the inverse table nbr_bwd [K, n_in] (flip: the forward table
    of an odd stride-1 kernel, read mirrored); cnt int32 [n_out] for "avg", arg int32 [n_out, c] for "max"."""
    m = _pool_mode(mode)
    dev = gy.device
    lib = _prep(dev)
    gy = _pool_feats(gy, "grad_output")
    nbr_bwd = _pool_table(nbr_bwd, None, "nbr_bwd")
    (n_out, c), (K, n_in) = gy.shape, nbr_bwd.shape
    if mode == "avg":
        cnt = _pool_vec(cnt, "cnt", torch.int32, n_out, dev)
    if mode == "max":
        if arg is None or arg.dtype != torch.int32 or arg.shape != gy.shape:
            raise TypeError("arg must be the int32 %s matrix of the forward pass" % (tuple(gy.shape),))
        arg = arg.contiguous()
    gx = torch.empty((n_in, c), dtype=torch.float32, device=dev)
    with _Dev(dev):
        check(lib.osn_pool_bwd(_p(gy), n_out, _p(nbr_bwd), n_in, K, int(bool(flip)), c, m, _p(cnt) if mode == "avg" else None,
                               _p(arg) if mode == "max" else None, _p(gx), _stream(dev)), "osn_pool_bwd")
    return gx


def _gpool_lists(order, offsets, n, dev):
    order = _pool_vec(order, "order", torch.int32, n, dev)
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.shape[0] < 1 or offsets.device != dev:
        raise TypeError("offsets must be int64 [n_batches + 1] on %s" % (dev,))
    return order, offsets.contiguous(), offsets.shape[0] - 1


def _gpool_reduce(entry, x, x2, order, offsets, m, want_arg):
    dev = x.device
    lib = _prep(dev)
    n, c = x.shape
    order, offsets, B = _gpool_lists(order, offsets, n, dev)
    y = torch.empty((B, c), dtype=torch.float32, device=dev)
    arg = torch.empty((B, c), dtype=torch.int32, device=dev) if want_arg else None
    ws = _ws(_cached("osn_gpool_ws_bytes", n, B, c), dev)
    with _Dev(dev):
        if entry == "osn_gpool_fwd":
            rc = lib.osn_gpool_fwd(_p(x), n, c, _p(order), _p(offsets), B, m, _p(y), _p(arg), _p(ws), ws.numel(), _stream(dev))
        else:
            rc = lib.osn_broadcast_bwd_pooled(_p(x), _p(x2), n, c, _p(order), _p(offsets), B, _p(y), _p(ws), ws.numel(), _stream(dev))
        check(rc, entry)
    return y, arg


def gpool_fwd(x, order, offsets, mode):
    """Global pooling of x [n, c]: one row per batch, the batches' rows as CSR (order int32 [n], offsets int64 [B + 1]) ->
    (y [B, c], arg int32 [B, c] for "max", else None)."""
    m = _pool_mode(mode)
    return _gpool_reduce("osn_gpool_fwd", _pool_feats(x, "x"), None, order, offsets, m, mode == "max")


def gpool_bwd(gy, rank, offsets, n, mode, arg=None):
    """Input gradient [n, c] of gpool_fwd: rank int32 [n] = every row's batch position."""
    m = _pool_mode(mode)
    dev = gy.device
    lib = _prep(dev)
    gy = _pool_feats(gy, "grad_output")
    B, c = gy.shape
    rank = _pool_vec(rank, "rank", torch.int32, n, dev)
    if offsets.dtype != torch.int64 or offsets.shape != (B + 1,):
        raise TypeError("offsets must be int64 [%d]" % (B + 1))
    if mode == "max":
        if arg is None or arg.dtype != torch.int32 or arg.shape != gy.shape:
            raise TypeError("arg must be the int32 %s matrix of the forward pass" % (tuple(gy.shape),))
        arg = arg.contiguous()
    gx = torch.empty((n, c), dtype=torch.float32, device=dev)
    with _Dev(dev):
        check(lib.osn_gpool_bwd(_p(gy), _p(rank), _p(offsets.contiguous()), _p(arg) if mode == "max" else None, n, B, c, m, _p(gx),
                                _stream(dev)), "osn_gpool_bwd")
    return gx


def broadcast_fwd(x, g, rank, op):
    """y[i] = x[i] + g[rank[i]] ("add") or x[i] * g[rank[i]] ("mul"): x [n, c], g [B, c], rank int32 [n]."""
    if op not in BROADCAST_OPS:
        raise ValueError("broadcast op %r (one of %s)" % (op, ", ".join(BROADCAST_OPS)))
    dev = x.device
    lib = _prep(dev)
    x, g = _pool_feats(x, "x"), _pool_feats(g, "pooled")
    n, c = x.shape
    if g.shape[1] != c:
        raise ValueError("broadcast: %d feature columns against %d pooled columns" % (c, g.shape[1]))
    rank = _pool_vec(rank, "rank", torch.int32, n, dev)
    y = torch.empty_like(x)
    with _Dev(dev):
        check(lib.osn_broadcast_fwd(_p(x), _p(g), _p(rank), n, g.shape[0], c, BROADCAST_OPS.index(op), _p(y), _stream(dev)),
              "osn_broadcast_fwd")
    return y


def broadcast_bwd_pooled(gy, x, order, offsets):
    """Gradient [B, c] of the pooled operand of a broadcast: the per-batch sum of gy (x None: addition) or of gy * x."""
    gy = _pool_feats(gy, "grad_output")
    if x is not None:
        x = _pool_feats(x, "x", gy.shape[0])
        if x.shape != gy.shape:
            raise ValueError("broadcast_bwd_pooled: shapes %s and %s differ" % (tuple(gy.shape), tuple(x.shape)))
    return _gpool_reduce("osn_broadcast_bwd_pooled", gy, x, order, offsets, 0, False)[0]


# ------------------------------------------------------------ points in and out of the grid (csrc/field.hip)
SEGMENT_MODES = ("sum", "avg")              # the `mode` word of osn_segment_reduce: the position in this tuple
FIELD_MAX_POINTS = ((1 << 31) - 1) // 8     # 8 m is an int32 pair index

InterpPlan = collections.namedtuple("InterpPlan", "pair offsets")


def _segment_mode(mode):
    if mode not in SEGMENT_MODES:
        raise ValueError("segment mode %r (one of %s)" % (mode, ", ".join(SEGMENT_MODES)))
    return SEGMENT_MODES.index(mode)


def _csr_offsets(offsets, dev):
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.shape[0] < 1 or offsets.device != dev:
        raise TypeError("offsets must be int64 [segments + 1] on %s" % (dev,))
    return offsets.contiguous()


def _positions(positions):
    if positions.dim() != 2 or positions.shape[1] != 4 or not positions.dtype.is_floating_point:
        raise TypeError("positions must be floating-point [M, 4] rows (batch, x, y, z) in lattice units")
    return _f32c(positions.float(), "positions")


def field_map(table, positions, stride):
    """The eight corners of every position's cell in the stride's coordinate table and their trilinear weights ->
    (nbr int32 [8, M], w float32 [8, M], bad int32 [1]: the invalid rows, counted on the device; reading it synchronises)."""
    positions = _positions(positions)
    dev = positions.device
    lib = _prep(dev)
    m = positions.shape[0]
    nbr = torch.empty((8, m), dtype=torch.int32, device=dev)
    w = torch.empty((8, m), dtype=torch.float32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    with _Dev(dev):
        check(lib.osn_field_map(_p(table.keys), _p(table.vals), table.cap, _p(positions), m, int(stride), _p(nbr), _p(w), _p(bad),
                                _stream(dev)), "osn_field_map")
    return nbr, w, bad


def _interp_tables(nbr, w, dev):
    if nbr.dtype != torch.int32 or nbr.dim() != 2 or nbr.shape[0] != 8 or nbr.device != dev:
        raise TypeError("nbr must be the int32 [8, M] corner table of field_map on %s" % (dev,))
    if w.dtype != torch.float32 or w.shape != nbr.shape or w.device != dev:
        raise TypeError("w must be the float32 %s weight table of field_map on %s" % (tuple(nbr.shape), dev))
    return nbr.contiguous(), w.contiguous()


def interp_fwd(x, nbr, w):
    """y [M, c] = the trilinear interpolation of x [n_in, c] over field_map's tables."""
    dev = x.device
    lib = _prep(dev)
    x = _pool_feats(x, "x")
    nbr, w = _interp_tables(nbr, w, dev)
    (n_in, c), m = x.shape, nbr.shape[1]
    y = torch.empty((m, c), dtype=torch.float32, device=dev)
    with _Dev(dev):
        check(lib.osn_interp_fwd(_p(x), n_in, _p(nbr), _p(w), m, c, _p(y), _stream(dev)), "osn_interp_fwd")
    return y


def interp_plan(nbr, n_in):
    """The backward plan of an interpolation: the flat indices e = k M + m of the present corners sorted by (voxel row, e)
    (a stable torch sort of the flattened table) and every voxel row's range in that list.  Built once per map."""
    m = nbr.shape[1]
    if m > FIELD_MAX_POINTS:
        raise ValueError("interp_plan: %d positions (8 M must stay below 2^31)" % m)
    flat = nbr.reshape(-1).long()
    e = torch.nonzero((flat >= 0) & (flat < int(n_in))).reshape(-1)
    rows = flat[e]
    perm = torch.sort(rows, stable=True)[1]
    counts = torch.bincount(rows, minlength=int(n_in))
    offsets = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).long()
    return InterpPlan(e[perm].int(), offsets)


def interp_bwd(gy, plan, w, n_in, out=None):
    """gx [n_in, c] of interp_fwd from gy [M, c] through interp_plan's lists; every element is written (out: the caller's own
    contiguous float32 [n_in, c] destination)."""
    dev = gy.device
    lib = _prep(dev)
    gy = _pool_feats(gy, "grad_output")
    m, c = gy.shape
    if w.dtype != torch.float32 or w.shape != (8, m) or w.device != dev:
        raise TypeError("w must be the float32 [8, %d] weight table of field_map on %s" % (m, dev))
    pair = plan.pair
    if pair.dtype != torch.int32 or pair.dim() != 1 or pair.device != dev:
        raise TypeError("plan.pair must be int32 [pairs] on %s" % (dev,))
    offsets = _csr_offsets(plan.offsets, dev)
    if offsets.shape[0] != int(n_in) + 1:
        raise TypeError("plan.offsets must be int64 [%d]" % (int(n_in) + 1))
    if out is not None and (out.dtype != torch.float32 or out.shape != (int(n_in), c) or out.device != dev or not out.is_contiguous()):
        raise TypeError("out must be a contiguous float32 [%d, %d] matrix on %s" % (int(n_in), c, dev))
    gx = torch.empty((int(n_in), c), dtype=torch.float32, device=dev) if out is None else out
    with _Dev(dev):
        check(lib.osn_interp_bwd(_p(gy), m, c, _p(pair.contiguous()), pair.shape[0], _p(offsets), _p(w.contiguous()), int(n_in), _p(gx),
                                 _stream(dev)), "osn_interp_bwd")
    return gx


def segment_reduce(x, order, offsets, mode):
    """y [segments, c]: the rows order[offsets[u] .. offsets[u + 1]) of x [n, c] added in list order ("avg": divided once by the
    length).  order int32 [n], offsets int64 [segments + 1]."""
    md = _segment_mode(mode)
    dev = x.device
    lib = _prep(dev)
    x = _pool_feats(x, "x")
    n, c = x.shape
    order = _pool_vec(order, "order", torch.int32, n, dev)
    offsets = _csr_offsets(offsets, dev)
    n_seg = offsets.shape[0] - 1
    y = torch.empty((n_seg, c), dtype=torch.float32, device=dev)
    with _Dev(dev):
        check(lib.osn_segment_reduce(_p(x), n, c, _p(order), _p(offsets), n_seg, md, _p(y), _stream(dev)), "osn_segment_reduce")
    return y


def segment_expand(g, rank, offsets=None, mode="sum"):
    """y [n, c] = g[rank[i]] ("avg": divided by the length of segment rank[i], from offsets): the gather osn_gpool_bwd performs,
    with a segment in the place of a batch.  rank int32 [n]."""
    md = _segment_mode(mode)
    dev = g.device
    lib = _prep(dev)
    g = _pool_feats(g, "g")
    n_seg, c = g.shape
    n = rank.shape[0]
    rank = _pool_vec(rank, "rank", torch.int32, n, dev)
    if mode == "avg":
        offsets = _csr_offsets(offsets, dev)
        if offsets.shape[0] != n_seg + 1:
            raise TypeError("offsets must be int64 [%d]" % (n_seg + 1))
    y = torch.empty((n, c), dtype=torch.float32, device=dev)
    with _Dev(dev):
        check(lib.osn_gpool_bwd(_p(g), _p(rank), _p(offsets) if mode == "avg" else None, None, n, n_seg, c, md, _p(y), _stream(dev)),
              "osn_gpool_bwd")
    return y
