#!/usr/bin/env python
"""Gate of "the weight-stationary reduction emits the next norm's backward column sums" (tools/probes/ws_reduce_sums.hip): the two
launches spconv_ws_reduce_kernel<K> -> col_reduce_kernel<1, mask> against one kernel in the column sums' geometry whose row is the
ascending-k sum over the partial planes (held to 128 and to 64 VGPRs), on the small maps' shapes -- 27 x 128 on the 3.3 k-row level,
27 x 256 on the 730-row level, 8 x 128 -- alone and beside wgrad_tl_kernel<4,4> on the side stream.  Each form is replayed from a HIP
graph (REPS launches, ROUNDS alternating measurements: median (max - min), us per call), after its finished rows and its fp64
partials were compared bit for bit with the two launches'.  BUILD=1 only builds the probe (no GPU needed)."""
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SRC = os.path.join(ROOT, "tools", "probes", "ws_reduce_sums.hip")
OUT = os.path.join(ROOT, "tools", "probes", "bin", "libprobe_ws_sums.so")


def build_probe():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    deps = [SRC] + [os.path.join(ROOT, "openscene_amd", "csrc", f) for f in ("bn.hip", "spconv_ws.hip", "epilogue.h")]
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-DNDEBUG",
                               "-Wno-deprecated-declarations", "-I", os.path.join(ROOT, "openscene_amd", "csrc"), SRC, "-o", OUT])
    return OUT


def main():
    if os.environ.get("BUILD") == "1":
        print(build_probe())
        return
    import numpy as np
    import torch
    from openscene_amd import _lib, ops, synthetic as syn
    from openscene_amd.sparse import CoordinateManager
    reps, rounds = int(os.environ.get("REPS", "40")), int(os.environ.get("ROUNDS", "6"))
    dev = torch.device("cuda", 0)
    _lib.load()
    ctypes.CDLL(_lib.LIB_PATH, mode=ctypes.RTLD_GLOBAL)     # (the probe takes the library's error reporting from the library itself)
    lib = ctypes.CDLL(build_probe())
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    lib.osn_dbg_ws_reduce_sums.argtypes = [i32, vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, f32, i32, vp, vp]
    vox = syn.shuffled(syn.grid_voxels(syn.room_points(0), 0.02), 0)
    cm = CoordinateManager(torch.from_numpy(syn.batch_coords([vox])).to(dev))
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    rng = np.random.default_rng(0)

    def table8(n):                                           # a 2^3 table: every row 1 .. 8 neighbours, row 0 none
        t = np.where(rng.random((8, n)) < 0.4, rng.integers(0, n, (8, n)), -1).astype(np.int32)
        t[rng.integers(0, 8, n), np.arange(n)] = 0
        t[:, 0] = -1
        return torch.from_numpy(t).to(dev)

    n3, n4 = cm.size(8), cm.size(16)
    configs = [("27x128 %d rows" % n3, cm.kmap(8, 8, 3)[0].contiguous(), 128), ("27x256 %d rows" % n4, cm.kmap(16, 16, 3)[0].contiguous(), 256),
               ("8x128 %d rows" % n3, table8(n3), 128)]
    # the side stream: the product's weight gradient 128 -> 128 on the 101 k-row level = wgrad_tl_kernel<4,4>
    n0 = cm.size(1)
    tiles = cm.kmap_tiles(1, 1, 3)[0]
    tl0 = ops.tile_lists(tiles[1], out_rows=tiles[0])
    ops.pair_lists(tl0)
    xs, gs = torch.randn(n0, 128, device=dev), torch.randn(n0, 128, device=dev)
    side = torch.cuda.Stream(device=dev)
    for name, nbr, c in configs:
        K, n = nbr.shape
        planes = torch.randn(K, n, c, generator=g, device=dev)
        planes[:, 1, 0] = float("nan")                       # (a NaN where row 1 has a neighbour: it must land where the two launches put it)
        zeros = torch.zeros(64, device=dev)
        x = torch.randn(n, c, generator=g, device=dev) * 2.5 + 0.7
        gamma, beta = torch.rand(c, generator=g, device=dev) + 0.5, torch.randn(c, generator=g, device=dev) * 0.3
        mean, var = x.mean(0), x.var(0, unbiased=False)
        n_rb = (n + 63) // 64 + 1

        def call(fused, mask_x, out, part):
            rc = lib.osn_dbg_ws_reduce_sums(fused, planes.data_ptr(), nbr.data_ptr(), zeros.data_ptr(), out.data_ptr(), n, K, c, x.data_ptr(),
                                            mean.data_ptr(), var.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5, mask_x, part.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc

        for mask_x in (1, 0):
            res = []
            for fused in (0, 1, 2):
                out, part = torch.full((n, c), 7.0, device=dev), torch.zeros(n_rb, 2, c, dtype=torch.float64, device=dev)
                call(fused, mask_x, out, part)
                torch.cuda.synchronize()
                res.append((out, part))
            for fused in (1, 2):
                same = [torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                                    b.view(torch.int64 if b.dtype == torch.float64 else torch.int32)) for a, b in zip(res[0], res[fused])]
                assert all(same), "%s mask_x %d fused %d: rows %s, partials %s" % (name, mask_x, fused, same[0], same[1])
            assert bool(torch.isnan(res[0][0]).any().item()) == bool((nbr[:, 1] >= 0).any().item())
        print("%s: finished rows and partials of both fused forms bit for bit the two launches' (mask from x and none)" % name, flush=True)
        out, part = torch.empty(n, c, device=dev), torch.zeros(n_rb, 2, c, dtype=torch.float64, device=dev)
        graphs = {}
        for fused in (0, 1, 2):
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(reps):
                    call(fused, 1, out, part)
            gr.replay()
            graphs[fused] = gr
        torch.cuda.synchronize()
        for beside in (False, True):
            t = {0: [], 1: [], 2: []}
            for _ in range(rounds):
                for fused in (0, 1, 2):
                    if beside:
                        with torch.cuda.stream(side):
                            for _ in range(30):
                                ops.spconv_wgrad_tl(xs, gs, tl0, 27)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    graphs[fused].replay()
                    e1.record()
                    torch.cuda.synchronize()
                    t[fused].append(e0.elapsed_time(e1) * 1e3 / reps)
            print("%-18s %-18s two launches %6.2f (%.2f) | fused <= 128 VGPRs %6.2f (%.2f) | fused <= 64 VGPRs %6.2f (%.2f)" % (
                name, "beside wgrad<4,4>" if beside else "alone", statistics.median(t[0]), max(t[0]) - min(t[0]), statistics.median(t[1]),
                max(t[1]) - min(t[1]), statistics.median(t[2]), max(t[2]) - min(t[2])), flush=True)


if __name__ == "__main__":
    main()
