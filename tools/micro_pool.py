"""Cost of the descriptor pool (csrc/pool.hip) against the same sums composed in torch on the same device: the bank widened
(fp16) or dequantised (fp8) to float32, normalised, and index_add_ed per group.  HIP events around back-to-back calls after a
warm-up, in windows of at least 50 ms.  The bank: 8 scenes x 150 k x 768, fp16 and its fp8 twin.

    python tools/micro_pool.py [iters] [--out FILE]

Prints (and with --out also writes) one JSON object per line, kind=pool, per case and bank kind:
  case=scenes        one descriptor per scene (no index array)
  case=objects       the objects of 32 queries, 16 per (scene, query), at 0.1 %, 2 % and 20 % of the points being hits
                     (hit_share): synthetic point -> object maps through PointGroups.from_objects
  case=one_scene     one 150 k scene
  us                 one call of ops.bank_pool / ops.bank_pool_fp8 as a user makes it: the scan, pool and finish launches, the
                     three result allocations and the Python around them; back-to-back calls over a window of at least 50 ms
                     (`calls` of them), best of two windows.  The small cases are therefore bounded by the host, not the device
  us_torch           the torch route, the sum of its parts (each timed alone, at least three calls and 50 ms); the whole bank
                     is widened and normalised whatever the groups hold, so speedup_index_add = index_add / us is the ratio
                     a gather-first torch route could approach; torch_temp_bytes = the float32 temporaries it allocates
  bytes              L * row bytes + 4 * G * d (row bytes: 2 d for fp16, d + 1 for fp8); hbm_share = bytes / us over 8 TB/s.
                     The calls re-read the same rows: where bank_bytes_touched (the distinct rows' bytes, at most) is below
                     the 256 MB of last-level cache the rows can come from there, and hbm_share is no share of HBM bandwidth
  max_abs_diff       the two routes' sums compared (a parity check: the tool stops if they disagree beyond 1e-3 of the largest)"""
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import ops                                        # noqa: E402
from openscene_amd.descriptors import PointGroups                    # noqa: E402
from openscene_amd.search import FeatureBank                         # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = None
if "--out" in sys.argv:
    OUT = sys.argv[sys.argv.index("--out") + 1]
    ARGS = [a for a in ARGS if a != OUT]
ITERS = int(ARGS[0]) if ARGS else 20
WINDOW_MS = 50.0
dev = torch.device("cuda", 0)
HBM_PEAK = 8.0e12
SCENES, ROWS, DIM, QUERIES, OBJECTS = 8, 150_000, 768, 32, 16
_lines = []


def timed(f, iters=ITERS, warmup=2, window_ms=WINDOW_MS):
    """(us per call, calls): device events around back-to-back calls, at least `iters` of them and at least `window_ms` long
    (a first window of `iters` calls sizes the second; a window of a millisecond measures the clock and the scheduler)."""
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
        x[torch.rand(ROWS, generator=gen, device=dev) < 0.1] = 0          # points without a fused feature
        bank.add_scene("scene%d" % i, x.half())
        del x
    return bank


def object_groups(bank, share, gen):
    """A synthetic find_objects result: every (point, query) is a hit with probability `share`, of a random object of 16."""
    n = bank.rows
    po = torch.randint(0, OBJECTS, (n, QUERIES), generator=gen, device=dev, dtype=torch.int32)
    po[torch.rand(n, QUERIES, generator=gen, device=dev) >= share] = -1
    fake = types.SimpleNamespace(point_object=po, offsets=bank.offsets,
                                 n_points=torch.empty((SCENES, QUERIES, OBJECTS), dtype=torch.int64, device="meta"))
    return PointGroups.from_objects(fake)


def kernel_route(bank, groups, err):
    kw = dict(rows=groups.rows, n_entries=groups.n_entries, err=err)
    if bank.dtype == "fp8":
        return ops.bank_pool_fp8(bank.codes, bank.exponents, groups.starts, **kw)[0]
    return ops.bank_pool(bank.features, groups.starts, **kw)[0]


def torch_route(bank, groups, group_of_entry, parts=None, scene=None):
    """scene: work on that scene's rows alone (the groups then index it from 0)"""
    def step(name, f):
        if parts is None:
            return f()
        out = [None]

        def g():
            out[0] = f()
        parts[name] = timed(g, iters=3, warmup=1)[0]
        return out[0]
    if bank.dtype == "fp16":
        wide = step("widen", lambda: (bank.features if scene is None else bank.scene(scene)).float())
    else:
        wide = step("widen", lambda: bank.dequantize(scene))
    unit = step("normalise", lambda: wide / (wide.norm(dim=-1, keepdim=True) + 1e-5))
    del wide

    def add():
        out = torch.zeros((groups.n_groups, bank.dim), dtype=torch.float32, device=dev)
        return out.index_add_(0, group_of_entry, unit if groups.rows is None else unit[groups.rows])
    return step("index_add", add)


def measure(case, bank, groups, **meta):
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    length = groups.starts[1:] - groups.starts[:-1]
    group_of_entry = torch.repeat_interleave(torch.arange(groups.n_groups, device=dev), length, output_size=groups.n_entries)
    scene = 0 if groups.rows is None and groups.n_entries < bank.rows else None     # one scene: torch works on its rows alone
    torch_rows = bank.rows if scene is None else groups.n_entries
    got = kernel_route(bank, groups, err)
    ops.bank_check(err)
    want = torch_route(bank, groups, group_of_entry, scene=scene)
    diff = (got - want).abs().max().item() if got.numel() else 0.0
    if not diff <= 1e-3 * max(want.abs().max().item(), 1e-30):
        raise SystemExit("%s %s: the kernel and the torch route disagree by %.3e" % (case, bank.dtype, diff))
    del got, want
    us, calls = min(timed(lambda: kernel_route(bank, groups, err)) for _ in range(2))
    parts = {}
    torch_route(bank, groups, group_of_entry, parts, scene=scene)
    us_torch = sum(parts.values())
    row_bytes = 2 * bank.dim if bank.dtype == "fp16" else bank.dim + 1
    entries = groups.n_entries
    nbytes = entries * row_bytes + 4 * groups.n_groups * bank.dim
    temp = 4 * bank.dim * (2 * torch_rows + (entries if groups.rows is not None else 0))
    emit(kind="pool", case=case, bank=bank.dtype, scenes=SCENES, rows_per_scene=ROWS, d=bank.dim, groups=groups.n_groups,
         entries=entries, us=us, calls=calls, us_torch=us_torch, torch_parts_us=parts, speedup=us_torch / us,
         speedup_index_add=parts["index_add"] / us, bytes=nbytes, hbm_share=nbytes / us * 1e6 / HBM_PEAK,
         bank_bytes_touched=min(entries, bank.rows) * row_bytes, torch_temp_bytes=temp, max_abs_diff=diff, **meta)


def main():
    gen = torch.Generator(device=dev).manual_seed(15)
    bank = make_bank(gen)
    bank8 = bank.to_fp8()
    one = PointGroups(bank.offsets_tensor()[:2].clone(), None, n_entries=ROWS)
    shares = [(s, object_groups(bank, s, gen)) for s in (0.001, 0.02, 0.2)]
    for b in (bank, bank8):
        measure("scenes", b, PointGroups.from_scenes(b))
        for share, groups in shares:
            measure("objects", b, groups, hit_share=share, queries=QUERIES, objects_per_scene_query=OBJECTS)
        measure("one_scene", b, one)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
