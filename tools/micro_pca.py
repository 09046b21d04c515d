"""Cost of the feature PCA (csrc/gram.hip, openscene_amd.pca) against the same Gram matrix composed in torch on the same device:
the bank widened (fp16) or dequantised (fp8) to float32 in row chunks, normalised, rounded to fp16, and ``xh.T @ xh`` accumulated
in float32 over the chunks.  HIP events around back-to-back calls after a warm-up, in windows of at least 50 ms.  The bank:
8 scenes x 150 k x 768, fp16 and its fp8 twin.

    python tools/micro_pca.py [iters] [--out FILE]

Prints (and with --out also writes) one JSON object per line, kind=pca, per case and bank kind:
  case=bank          the whole bank as one group
  case=scenes        one group per scene (no index array)
  case=one_scene     one 150 k scene
  us                 one call of ops.bank_gram / ops.bank_gram_fp8 as a user makes it: the scan, scale, Gram and finish launches,
                     the three result allocations and the Python around them; back-to-back calls over a window of at least
                     50 ms (`calls` of them), best of two windows.  us_raw: the same with normalize=False (the scale launch reads no row)
  flops              n d (d + 128): two per multiply-add of the computed triangle of 128-column tiles (the diagonal tiles whole);
                     mfma_share = flops / us over the 2.5 PFLOP/s of dense fp16 MFMA
  bytes_read         what the launches read: the scale pass's n rows, the Gram pass's two column strips per tile pair and slice
                     (most of them from the L2 the tile pairs of a slice share), the partials written and read once each;
                     bank_bytes = the distinct rows; hbm_share and bank_hbm_share = each / us over 8 TB/s.  bound names the
                     larger of flops over the MFMA peak and bank_bytes over the HBM peak, roof_us is that least time
  ws_bytes           osn_bank_gram_ws_bytes: the fp32 partials (64 KiB per slice and tile pair) and one scale per entry
  us_torch           the torch route in chunks of CHUNK rows (at least three calls and 50 ms); a chunk's product is an fp16 matrix
                     (torch's fp16 matmul: fp32 accumulation inside, fp16 out) added into a float32 one; torch_temp_bytes = the
                     float32 and fp16 temporaries of one chunk
  us_eigh            principal_directions(k=3): the Gram matrices to the host and torch.linalg.eigh in float64 (host clock)
  us_project, us_colors   Basis.project (the heat pass over the rows of the case, 3 fp16 queries) and Basis.colors (project, a
                     sort per coordinate, the map), host clock around a synchronised call, best of three
  max_rel_diff       the two routes' Gram matrices compared, over the largest element (a parity check: the tool stops beyond
                     2e-3 -- the torch route rounds every chunk's product to fp16)"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import _lib, ops                                  # noqa: E402
from openscene_amd import pca                                        # noqa: E402
from openscene_amd.descriptors import PointGroups                    # noqa: E402
from openscene_amd.search import FeatureBank                         # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = None
if "--out" in sys.argv:
    OUT = sys.argv[sys.argv.index("--out") + 1]
    ARGS = [a for a in ARGS if a != OUT]
ITERS = int(ARGS[0]) if ARGS else 5
WINDOW_MS = 50.0
dev = torch.device("cuda", 0)
HBM_PEAK = 8.0e12
MFMA_F16_PEAK = 2.5e15
SCENES, ROWS, DIM, CHUNK, TILE = 8, 150_000, 768, 16384, 128
_lines = []


def timed(f, iters=ITERS, warmup=2, window_ms=WINDOW_MS):
    """(us per call, calls): device events around back-to-back calls, at least `iters` of them and at least `window_ms` long."""
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while True:
        a.record()
        for _ in range(iters):
            f()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= window_ms:
            return ms * 1e3 / iters, iters
        iters = int(iters * 1.2 * window_ms / max(ms, 1e-3)) + 1


def host_timed(f, repeats=3):
    """us of one synchronised call by the host clock, best of `repeats` after one warm-up call"""
    f()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e6)
    return best


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    _lines.append(line)


def make_bank(gen):
    bank = FeatureBank(DIM, dev, capacity_rows=SCENES * ROWS)
    for i in range(SCENES):
        x = torch.randn(ROWS, DIM, generator=gen, device=dev)
        x[:, :8] += 2.0 + 0.5 * i                                        # a common direction that differs from scene to scene
        x[torch.rand(ROWS, generator=gen, device=dev) < 0.1] = 0          # points without a fused feature
        bank.add_scene("scene%d" % i, x.half())
        del x
    return bank


def kernel_route(bank, groups, err, normalize=True):
    kw = dict(rows=groups.rows, normalize=normalize, n_entries=groups.n_entries, err=err)
    if bank.dtype == "fp8":
        return ops.bank_gram_fp8(bank.codes, bank.exponents, groups.starts, **kw)[0]
    return ops.bank_gram(bank.features, groups.starts, **kw)[0]


def torch_route(bank, spans):
    """spans: the row range of every group.  -> float32 [G, d, d]"""
    out = torch.zeros((len(spans), bank.dim, bank.dim), dtype=torch.float32, device=dev)
    table = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(dev) if bank.dtype == "fp8" else None
    for g, (a, b) in enumerate(spans):
        for r0 in range(a, b, CHUNK):
            r1 = min(r0 + CHUNK, b)
            if bank.dtype == "fp16":
                wide = bank.features[r0:r1].float()
            else:
                wide = torch.ldexp(table[bank.codes[r0:r1].long()], bank.exponents[r0:r1].int()[:, None])
            xh = (wide / (wide.norm(dim=-1, keepdim=True) + 1e-5)).half()
            out[g] += (xh.t() @ xh).float()
    return out


def measure(case, bank, groups, spans):
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    n, d, g = groups.n_entries, bank.dim, groups.n_groups
    got = kernel_route(bank, groups, err)
    ops.bank_check(err)
    want = torch_route(bank, spans)
    diff = ((got - want).abs().max() / want.abs().max().clamp(min=1e-30)).item()
    if not diff <= 2e-3:
        raise SystemExit("%s %s: the kernel and the torch route disagree by %.3e of the largest element" % (case, bank.dtype, diff))
    del got, want
    us, calls = min(timed(lambda: kernel_route(bank, groups, err)) for _ in range(2))
    us_raw, _ = min(timed(lambda: kernel_route(bank, groups, err, normalize=False)) for _ in range(2))
    us_torch, _ = timed(lambda: torch_route(bank, spans), iters=3, warmup=1)
    elt = 2 if bank.dtype == "fp16" else 1
    nt = (d + TILE - 1) // TILE
    n_pairs = nt * (nt + 1) // 2
    slices = sum((b - a + ops.BANK_GRAM_SLICE - 1) // ops.BANK_GRAM_SLICE for a, b in spans)
    flops = n * d * (d + TILE)
    partial_bytes = slices * n_pairs * TILE * TILE * 4
    bank_bytes = n * (d * elt + (1 if elt == 1 else 0))
    bytes_read = bank_bytes + n * TILE * elt * (2 * n_pairs - nt) + 2 * partial_bytes
    ws_bytes = int(_lib.load().osn_bank_gram_ws_bytes(g, n, d))
    m = pca.moments(bank, groups)
    us_eigh = min(_host(lambda: pca.principal_directions(m, k=3)) for _ in range(2))
    basis = pca.principal_directions(m, k=3)
    scene = 0 if n < bank.rows else None                                 # one scene: its rows alone
    us_project = host_timed(lambda: basis.project(bank, 0, scene=scene))
    us_colors = host_timed(lambda: basis.colors(bank, 0, scene=scene))
    emit(kind="pca", case=case, bank=bank.dtype, scenes=SCENES, rows_per_scene=ROWS, d=d, groups=g, entries=n, slice=ops.BANK_GRAM_SLICE,
         us=us, calls=calls, us_raw=us_raw, us_torch=us_torch, speedup=us_torch / us, flops=flops,
         mfma_share=flops / us * 1e6 / MFMA_F16_PEAK, bytes_read=bytes_read, bank_bytes=bank_bytes,
         hbm_share=bytes_read / us * 1e6 / HBM_PEAK, bank_hbm_share=bank_bytes / us * 1e6 / HBM_PEAK,
         bound="compute" if flops / MFMA_F16_PEAK >= bank_bytes / HBM_PEAK else "memory",
         roof_us=max(flops / MFMA_F16_PEAK, bank_bytes / HBM_PEAK) * 1e6,
         ws_bytes=ws_bytes, torch_temp_bytes=CHUNK * d * (4 + 4 + 2) + d * d * 2, us_eigh=us_eigh, us_project=us_project,
         us_colors=us_colors, projected_rows=n, max_rel_diff=diff)


def _host(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e6


def main():
    gen = torch.Generator(device=dev).manual_seed(26)
    bank = make_bank(gen)
    bank8 = bank.to_fp8()
    off = bank.offsets
    whole = PointGroups(torch.tensor([0, bank.rows], dtype=torch.int64, device=dev), None, n_entries=bank.rows)
    one = PointGroups(bank.offsets_tensor()[:2].clone(), None, n_entries=ROWS)
    for b in (bank, bank8):
        measure("bank", b, whole, [(0, b.rows)])
        measure("scenes", b, PointGroups.from_scenes(b), list(zip(off[:-1], off[1:])))
        measure("one_scene", b, one, [(0, ROWS)])
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
