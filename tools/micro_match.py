"""Cost of matching bank rows to exemplars (csrc/match.hip, openscene_amd.match) against the same lists composed in torch on the
same device: the query rows widened (fp16) or dequantised (fp8) to float32 in row chunks, normalised, rounded to fp16,
``xq @ xe.T`` per chunk and ``torch.topk`` of it.  HIP events around back-to-back calls after a warm-up, in windows of at least
50 ms.  The bank: 8 scenes x 150 k x 768, fp16 and its fp8 twin; the exemplars: rows of the last scene, prepared once by
``ops.bank_unit_rows`` (both routes read the same fp16 image).

    python tools/micro_match.py [iters] [--out FILE]

Prints (and with --out also writes) one JSON object per line, kind=match, per case, k and bank kind:
  case=scene_x_1k / scene_x_20k / scene_x_150k   one 150 k scene against M exemplars
  case=bank_x_20k                                the whole bank (1.2 M rows) against 20 k exemplars
  case=clicks_x_150k                             64 scattered rows against 150 k exemplars: the split path
  us                 one call of ops.bank_match / ops.bank_match_fp8 as a user makes it with an err word of the caller's: the
                     match and merge launches, the three result allocations and the Python around them; back-to-back calls
                     over a window of at least 50 ms (`calls` of them), best of two windows
  us_kernels         the C entry alone on preallocated results and workspace: the two launches
  flops              2 L M d; mfma_share = flops / us_kernels over the 2.5 PFLOP/s of dense fp16 MFMA
  exemplar_bytes     what the workgroups request of the exemplar image from the caches: ceil(L / 64) x M x d x 2 (every
                     workgroup streams its whole exemplar range once); exemplar_tbs = that / us_kernels in TB/s;
                     query_bytes = the L rows read once per split
  splits, ws_bytes   the split in effect and osn_bank_match_ws_bytes: 8 L k splits plus a constant
  us_torch           the torch route in chunks of `torch_chunk` rows (the chunk's fp16 product held to 1 GiB), at least one call
                     and 50 ms; torch_temp_bytes = the float32 / fp16 temporaries and the product of one chunk.  Its product is an
                     fp16 matrix (fp32 accumulation inside, fp16 out): not of equal precision -- top1_agree is the share of rows
                     on which the two routes name the same best exemplar, not a parity check
  us_unit_rows       ops.bank_unit_rows of the M exemplar rows (done once per exemplar set)"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import _lib, ops                                  # noqa: E402
from openscene_amd.ops import _p, _stream                            # noqa: E402
from openscene_amd.search import FeatureBank                         # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = None
if "--out" in sys.argv:
    OUT = sys.argv[sys.argv.index("--out") + 1]
    ARGS = [a for a in ARGS if a != OUT]
ITERS = int(ARGS[0]) if ARGS else 3
WINDOW_MS = 50.0
dev = torch.device("cuda", 0)
MFMA_F16_PEAK = 2.5e15
SCENES, ROWS, DIM = 8, 150_000, 768
PRODUCT_BYTES = 1 << 30
_lines = []


def timed(f, iters=ITERS, warmup=1, window_ms=WINDOW_MS):
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


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    _lines.append(line)


def make_bank(gen):
    bank = FeatureBank(DIM, dev, capacity_rows=SCENES * ROWS)
    for i in range(SCENES):
        x = torch.randn(ROWS, DIM, generator=gen, device=dev)
        x[:, :8] += 2.0 + 0.5 * i                                        # a common direction that differs from scene to scene
        bank.add_scene("scene%d" % i, x.half())
        del x
    return bank


def stored(bank, a, b):
    """the bank arrays of rows [a, b): what the ops take ahead of their shared arguments"""
    return (bank.codes[a:b], bank.exponents[a:b]) if bank.dtype == "fp8" else (bank.features[a:b],)


def kernel_route(bank, span, rows, image, k, err):
    f = ops.bank_match_fp8 if bank.dtype == "fp8" else ops.bank_match
    return f(*stored(bank, *span), image, k=k, rows=rows, err=err)


def raw_entry(bank, span, rows, image, k, err):
    """-> a closure that calls the C entry on preallocated arrays"""
    lib = _lib.load()
    arrays = stored(bank, *span)
    n = arrays[0].shape[0]
    l = n if rows is None else rows.shape[0]
    m, d = image.shape
    idx = torch.empty((l, k), dtype=torch.int32, device=dev)
    score = torch.empty((l, k), dtype=torch.float32, device=dev)
    count = torch.empty((l,), dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.osn_bank_match_ws_bytes(l, m, d, k, 0)), dtype=torch.uint8, device=dev)
    entry = lib.osn_bank_match_fp8 if bank.dtype == "fp8" else lib.osn_bank_match
    ptrs = tuple(_p(t) for t in arrays)
    st = _stream(dev)

    def call():
        rc = entry(*ptrs, n, d, _p(rows), l, 1, _p(image), m, k, 0, _p(idx), _p(score), _p(count), _p(err), _p(ws), ws.numel(), st)
        if rc != 0:
            raise SystemExit("%s returned %d" % (entry.__name__, rc))
    return call, ws.numel()


def torch_route(bank, span, rows, image, k, chunk):
    a, b = span
    table = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().to(dev) if bank.dtype == "fp8" else None
    l = (b - a) if rows is None else rows.shape[0]
    idx = torch.empty((l, k), dtype=torch.int64, device=dev)
    score = torch.empty((l, k), dtype=torch.float16, device=dev)
    for r0 in range(0, l, chunk):
        r1 = min(r0 + chunk, l)
        sel = slice(a + r0, a + r1) if rows is None else rows[r0:r1] + a
        if bank.dtype == "fp16":
            wide = bank.features[sel].float()
        else:
            wide = torch.ldexp(table[bank.codes[sel].long()], bank.exponents[sel].int()[:, None])
        xq = (wide / (wide.norm(dim=-1, keepdim=True) + 1e-5)).half()
        score[r0:r1], idx[r0:r1] = torch.topk(xq @ image.t(), k, dim=1)
    return idx, score


def measure(case, bank, span, rows, image, k):
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    a, b = span
    l = (b - a) if rows is None else rows.shape[0]
    m, d = image.shape
    got = kernel_route(bank, span, rows, image, k, err)[0]
    ops.bank_check(err)
    chunk = max(1, min(l, PRODUCT_BYTES // (2 * m)))
    want = torch_route(bank, span, rows, image, k, chunk)[0]
    agree = float((got[:, 0].long() == want[:, 0]).double().mean())
    del got, want
    us, calls = min(timed(lambda: kernel_route(bank, span, rows, image, k, err)) for _ in range(2))
    raw, ws_bytes = raw_entry(bank, span, rows, image, k, err)
    us_kernels, _ = min(timed(raw) for _ in range(2))
    ops.bank_check(err)
    us_torch, _ = timed(lambda: torch_route(bank, span, rows, image, k, chunk), iters=1, warmup=1)
    elt = 2 if bank.dtype == "fp16" else 1
    n_qt = (l + ops.BANK_MATCH_TILE_Q - 1) // ops.BANK_MATCH_TILE_Q
    splits = (ws_bytes - 4096) // (8 * l * k) if l else 0              # (the workspace is 8 L k splits, rounded up to 256, + 4096)
    flops = 2 * l * m * d
    exemplar_bytes = n_qt * m * d * 2
    emit(kind="match", case=case, bank=bank.dtype, rows=l, exemplars=m, d=d, k=k, us=us, calls=calls, us_kernels=us_kernels,
         us_torch=us_torch, speedup=us_torch / us, flops=flops, mfma_share=flops / us_kernels * 1e6 / MFMA_F16_PEAK,
         exemplar_bytes=exemplar_bytes, exemplar_tbs=exemplar_bytes / us_kernels * 1e6 / 1e12,
         query_bytes=l * (d * elt + (1 if elt == 1 else 0)) * max(splits, 1), splits=splits, ws_bytes=ws_bytes, torch_chunk=chunk,
         torch_temp_bytes=chunk * d * (4 + 4 + 2) + chunk * m * 2 + chunk * k * 10, top1_agree=agree)


def main():
    gen = torch.Generator(device=dev).manual_seed(27)
    bank = make_bank(gen)
    bank8 = bank.to_fp8()
    last = bank.offsets[SCENES - 1]
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    images = {}
    for name, m in (("1k", 1000), ("20k", 20000), ("150k", ROWS)):
        src = torch.randperm(ROWS, generator=gen, device=dev)[:m] + last
        images[name] = ops.bank_unit_rows(bank.features, src, err=err)
        us_unit, _ = timed(lambda: ops.bank_unit_rows(bank.features, src, err=err))
        emit(kind="match_unit_rows", exemplars=m, d=DIM, us_unit_rows=us_unit)
    ops.bank_check(err)
    clicks = torch.randint(0, ROWS, (64,), generator=gen, device=dev)
    for b in (bank, bank8):
        for k in (1, 8):
            for name in ("1k", "20k", "150k"):
                measure("scene_x_" + name, b, (0, ROWS), None, images[name], k)
            measure("bank_x_20k", b, (0, b.rows), None, images["20k"], k)
            measure("clicks_x_150k", b, (0, ROWS), clicks, images["150k"], k)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
