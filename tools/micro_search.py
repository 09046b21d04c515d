"""Cost of the bank search (csrc/search.hip) against the same answer composed from what the package offered before it:
the fp16 bank widened to float32, ops.cosine_query(want_scores=True), the norm and the division in torch, torch.topk per
scene and query.  HIP events around back-to-back calls after a warm-up.

    python tools/micro_search.py [iters]

Prints one JSON object per line:
  kind=search   per shape (scenes x rows x d x Q, k = 16): us of the whole search, of the heat pass alone (a call without
                scenes) and their difference (the select pass), the select pass's share, the heat pass's fraction of the HBM
                roof on 2 N d + 2 N Q bytes, and the composed path's us with its parts (widen / query / norm + divide / topk)
  kind=append   osn_bank_append against X[g].half() in torch"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import ops                                        # noqa: E402
from openscene_amd.search import FeatureBank, search                 # noqa: E402

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda", 0)
HBM_PEAK = 8.0e12
K = 16


def timed(f, iters=ITERS, warmup=3):
    """us per call: device events around `iters` calls."""
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def emit(**kw):
    print(json.dumps(kw), flush=True)


def make_bank(scenes, n, d, gen):
    bank = FeatureBank(d, dev, capacity_rows=scenes * n)
    for i in range(scenes):
        x = torch.randn(n, d, generator=gen, device=dev)
        x[torch.rand(n, generator=gen, device=dev) < 0.1] = 0          # points without a fused feature
        bank.add_scene("scene%d" % i, x.half())
        del x
    return bank


def composed(bank, text, offsets, parts=None):
    """The parent commit's route to the same heat-map and top-k."""
    def step(name, f):
        if parts is None:
            return f()
        out = [None]

        def g():
            out[0] = f()
        parts[name] = timed(g, iters=max(3, ITERS // 4), warmup=1)
        return out[0]
    h = bank.features
    wide = step("widen", lambda: h.float())
    scores = step("query", lambda: ops.cosine_query(wide, text, want_scores=True)[0])
    heat = step("norm_divide", lambda: (scores.float() / (wide.norm(dim=-1, keepdim=True) + 1e-5)).half())

    def topk():
        out = []
        for a, b in zip(offsets[:-1], offsets[1:]):
            out.append(torch.topk(heat[a:b].t().float(), min(K, b - a), dim=1))
        return out
    step("topk", topk)
    return heat


def shapes():
    gen = torch.Generator(device=dev).manual_seed(1)
    for scenes, n, d, q in ((1, 150_000, 768, 1), (1, 150_000, 768, 8), (1, 150_000, 768, 32), (8, 150_000, 768, 32),
                            (1, 550_000, 768, 32), (1, 550_000, 768, 1), (8, 150_000, 512, 32)):
        bank = make_bank(scenes, n, d, gen)
        text = torch.nn.functional.normalize(torch.randn(q, d, generator=gen, device=dev), dim=1).half()
        rows = scenes * n
        empty = torch.zeros(1, dtype=torch.int64, device=dev)
        r = {"all": [], "heat": [], "composed": []}
        for _ in range(2):                                            # A B C A B C: shows the spread
            r["all"].append(timed(lambda: search(bank, text, k=K, return_heat=True)))
            r["heat"].append(timed(lambda: ops.bank_search(bank.features, empty, text, k=K, want_heat=True, max_scene_rows=0)))
            r["composed"].append(timed(lambda: composed(bank, text, bank.offsets), iters=max(3, ITERS // 4), warmup=1))
        parts = {}
        composed(bank, text, bank.offsets, parts)
        us_all, us_heat, us_comp = min(r["all"]), min(r["heat"]), min(r["composed"])
        nbytes = 2 * rows * d + 2 * rows * q
        emit(kind="search", scenes=scenes, rows_per_scene=n, d=d, q=q, k=K, us_search=r["all"], us_heat_pass=r["heat"],
             us_select_pass=us_all - us_heat, select_share=(us_all - us_heat) / us_all, bytes=nbytes,
             heat_hbm_share=nbytes / us_heat * 1e6 / HBM_PEAK, search_hbm_share=nbytes / us_all * 1e6 / HBM_PEAK,
             us_composed=r["composed"], composed_parts_us=parts, speedup=us_comp / us_all)
        del bank


def append():
    gen = torch.Generator(device=dev).manual_seed(2)
    for nv, n, d in ((75_000, 150_000, 768), (75_000, 150_000, 512)):
        x = torch.randn(nv, d, generator=gen, device=dev)
        g = torch.randint(0, nv, (n,), generator=gen, device=dev)
        bank = torch.empty((n, d), dtype=torch.float16, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        us = timed(lambda: ops.bank_append(bank, 0, x, err, gather=g))
        ops.bank_check(err)
        us_torch = timed(lambda: bank.copy_(x[g].half()))
        nbytes = n * d * 6 + n * 8
        emit(kind="append", rows=n, d=d, us=us, us_torch=us_torch, bytes=nbytes, hbm_share=nbytes / us * 1e6 / HBM_PEAK)


if __name__ == "__main__":
    shapes()
    append()
