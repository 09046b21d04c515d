"""Cost of the bank search (csrc/search.hip) against the same answer composed from what the package offered before it:
the fp16 bank widened to float32, ops.cosine_query(want_scores=True), the norm and the division in torch, torch.topk per
scene and query.  HIP events around back-to-back calls after a warm-up.

    python tools/micro_search.py [iters] [--no-composed] [--contrast-only]
    python tools/micro_search.py [iters] --ensemble-only          (the default run does not time the ensemble)

Prints one JSON object per line:
  kind=search   per shape (scenes x rows x d x Q, k = 16): us of the whole search, of the heat pass alone (a call without
                scenes) and their difference (the select pass), the select pass's share, the heat pass's fraction of the HBM
                roof on 2 N d + 2 N Q bytes, and the composed path's us with its parts (widen / query / norm + divide / topk)
                fp8 bank of the same rows (bank.to_fp8()), timed in the same A B loop: us_search_fp8, us_heat_pass_fp8, the
                heat pass's fraction of the roof on N (d + 1) + 2 N Q (+ 2 N Q for heatT) bytes, its ratio to the fp16 heat
                pass, and -- after a parity check of 2048 sampled rows against the float64 formula on the stored values
                (abs <= 2e-3, or the tool stops) -- the fidelity against the fp16 bank: largest and rms difference of the
                normalised scores, overlap of the per-scene top-16
  kind=append   osn_bank_append against X[g].half() in torch; osn_bank_append_fp8 from float32 and from float16 rows
  kind=contrast search with negatives (8 scenes x 150 k x 768, 32 queries + 4 negatives, k = 16, heat returned; fp16 and fp8
                bank) against two routes on the same build, the three timed in turn for ROUNDS rounds: plain36 = the plain
                search with the 36 rows as queries (the same MFMA work and bank traffic, four more heat columns written);
                torch_route = that plain search, then the relevancy formula in torch on the [N, 36] heat-map and torch.topk
                per scene.  Per route every round's us, the minimum and the spread (max - min) / min; the ratios of the
                minima.  Before timing, the relevancy map is held to 1 fp16 ulp of the float64 formula on the plain36
                heat-map (or the tool stops).
  kind=ensemble (--ensemble-only) two banks searched as one (8 scenes x 150 k x 768, 32 queries, without and with 4 negatives,
                k = 16, heat returned; fp16 and fp8 banks; both modes) against two routes on the same build, timed in turn for
                ROUNDS rounds: composed = two searches with return_heat (two more, normalised and plain, where the vocabulary
                pick is not taken on the maps themselves), torch max / compare / where, torch.topk per scene; plain = the
                search of one bank, the floor on half the ensemble's bytes.  Whole call and heat pass alone (a call without
                scenes).  Per route every round's us, the minimum and the spread; composed / ensemble and ensemble / (2 x
                plain).  Before timing, the ensemble's heat-map and source are held to the composed ones bit for bit (or the
                tool stops)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import ops                                        # noqa: E402
from openscene_amd.search import FeatureBank, search                 # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
ITERS = int(ARGS[0]) if ARGS else 20
COMPOSED = "--no-composed" not in sys.argv
CONTRAST_ONLY = "--contrast-only" in sys.argv
ROUNDS = 5
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


def fp8_parity(bank8, text, heat8, gen):
    """2048 sampled rows of the fp8 heat-map against acc * 2^e / (sqrt(sum c^2) * 2^e + 1e-5) in float64 -> max abs deviation."""
    rows = torch.randint(0, bank8.rows, (2048,), generator=gen, device=dev)
    table = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().to(dev)
    c = table[bank8.codes[rows].long()]
    s = torch.pow(torch.tensor(2.0, dtype=torch.float64, device=dev), bank8.exponents[rows].double())[:, None]
    ref = (c @ text.double().t()) * s / (c.square().sum(dim=1, keepdim=True).sqrt() * s + 1e-5)
    worst = (heat8[rows].double() - ref).abs().max().item()
    if not worst <= 2e-3:
        raise SystemExit("fp8 heat-map is off the float64 formula by %.3e" % worst)
    return worst


def fidelity(res, res8):
    diff = (res8.heat.float() - res.heat.float()).double()
    same = 0
    for s in range(res.topk_points.shape[0]):
        for q in range(res.topk_points.shape[1]):
            same += len(set(res.topk_points[s, q].tolist()) & set(res8.topk_points[s, q].tolist()))
    return {"max_abs": diff.abs().max().item(), "rms": diff.square().mean().sqrt().item(),
            "topk_overlap": same / res.topk_points.numel()}


def shapes():
    gen = torch.Generator(device=dev).manual_seed(1)
    for scenes, n, d, q in ((1, 150_000, 768, 1), (1, 150_000, 768, 8), (1, 150_000, 768, 32), (8, 150_000, 768, 32),
                            (1, 550_000, 768, 32), (1, 550_000, 768, 1), (8, 150_000, 512, 32)):
        bank = make_bank(scenes, n, d, gen)
        text = torch.nn.functional.normalize(torch.randn(q, d, generator=gen, device=dev), dim=1).half()
        rows = scenes * n
        empty = torch.zeros(1, dtype=torch.int64, device=dev)
        bank8 = bank.to_fp8()
        res, res8 = search(bank, text, k=K, return_heat=True), search(bank8, text, k=K, return_heat=True)
        parity = fp8_parity(bank8, text, res8.heat, gen)
        fid = fidelity(res, res8)
        del res, res8
        r = {"all": [], "heat": [], "composed": [], "all8": [], "heat8": []}
        for _ in range(2):                                            # A B C A B C: shows the spread
            r["all"].append(timed(lambda: search(bank, text, k=K, return_heat=True)))
            r["all8"].append(timed(lambda: search(bank8, text, k=K, return_heat=True)))
            r["heat"].append(timed(lambda: ops.bank_search(bank.features, empty, text, k=K, want_heat=True, max_scene_rows=0)))
            r["heat8"].append(timed(lambda: ops.bank_search_fp8(bank8.codes, bank8.exponents, empty, text, k=K, want_heat=True,
                                                                max_scene_rows=0)))
            if COMPOSED:
                r["composed"].append(timed(lambda: composed(bank, text, bank.offsets), iters=max(3, ITERS // 4), warmup=1))
        parts = {}
        if COMPOSED:
            composed(bank, text, bank.offsets, parts)
        us_all, us_heat, us_comp = min(r["all"]), min(r["heat"]), min(r["composed"]) if COMPOSED else None
        us_all8, us_heat8 = min(r["all8"]), min(r["heat8"])
        nbytes = 2 * rows * d + 2 * rows * q
        nbytes8 = rows * (d + 1) + 2 * rows * q
        emit(kind="search", scenes=scenes, rows_per_scene=n, d=d, q=q, k=K, us_search=r["all"], us_heat_pass=r["heat"],
             us_select_pass=us_all - us_heat, select_share=(us_all - us_heat) / us_all, bytes=nbytes,
             heat_hbm_share=nbytes / us_heat * 1e6 / HBM_PEAK, search_hbm_share=nbytes / us_all * 1e6 / HBM_PEAK,
             us_composed=r["composed"], composed_parts_us=parts, speedup=us_comp / us_all if COMPOSED else None,
             us_search_fp8=r["all8"], us_heat_pass_fp8=r["heat8"], bytes_fp8=nbytes8, bytes_fp8_with_heatT=nbytes8 + 2 * rows * q,
             heat_hbm_share_fp8=nbytes8 / us_heat8 * 1e6 / HBM_PEAK,
             heat_hbm_share_fp8_with_heatT=(nbytes8 + 2 * rows * q) / us_heat8 * 1e6 / HBM_PEAK,
             heat_fp8_over_fp16=us_heat8 / us_heat, search_fp8_over_fp16=us_all8 / us_all, fp8_parity_max_abs=parity,
             fp8_vs_fp16=fid)
        del bank, bank8


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
        codes = torch.empty((n, d), dtype=torch.uint8, device=dev)
        exps = torch.empty((n,), dtype=torch.int8, device=dev)
        for src, width in ((x, 4), (x.half(), 2)):
            us8 = timed(lambda: ops.bank_append_fp8(codes, exps, 0, src, err, gather=g))
            ops.bank_check(err)
            nbytes8 = n * d * width + n * (d + 1) + n * 8
            emit(kind="append_fp8", source="float%d" % (8 * width), rows=n, d=d, us=us8, bytes=nbytes8,
                 hbm_share=nbytes8 / us8 * 1e6 / HBM_PEAK, rows_per_s=n / us8 * 1e6)


def contrast():
    scenes, n, d, q, m, tau = 8, 150_000, 768, 32, 4, 0.1
    gen = torch.Generator(device=dev).manual_seed(3)
    bank16 = make_bank(scenes, n, d, gen)
    rows = torch.nn.functional.normalize(torch.randn(q + m, d, generator=gen, device=dev), dim=1).half()
    text, neg = rows[:q].contiguous(), rows[q:].contiguous()
    for kind, bank in (("fp16", bank16), ("fp8", bank16.to_fp8())):
        def ours():
            return search(bank, text, k=K, return_heat=True, negatives=neg, temperature=tau)

        def plain36():
            return search(bank, rows, k=K, return_heat=True)

        def torch_route():
            heat = plain36().heat.float()
            rel = torch.sigmoid((heat[:, :q] - heat[:, q:].max(dim=1, keepdim=True)[0]) / tau).half()
            return rel, [torch.topk(rel[a:b].t().float(), min(K, b - a), dim=1) for a, b in zip(bank.offsets[:-1], bank.offsets[1:])]
        heat = plain36().heat[::97].double()                   # parity on every 97th row
        z = (heat[:, :q] - heat[:, q:].max(dim=1, keepdim=True)[0]) / float(torch.tensor(tau, dtype=torch.float32))
        want = (1.0 / (1.0 + torch.exp(-z))).cpu().numpy().astype("float16")
        got = ours().heat[::97].cpu().numpy()
        ok = (got == got) == (want == want)
        ulps = abs(got.view("int16").astype("int64") - want.view("int16").astype("int64"))[got == got]
        if not ok.all() or ulps.max() > 1:
            raise SystemExit("relevancy map is off the float64 formula by %d ulp" % ulps.max())
        us = {"contrast": [], "plain36": [], "torch_route": []}
        for _ in range(ROUNDS):                                # A B C A B C: shows the spread
            us["contrast"].append(timed(ours))
            us["plain36"].append(timed(plain36))
            us["torch_route"].append(timed(torch_route, iters=max(3, ITERS // 4), warmup=1))
        lo = {k_: min(v) for k_, v in us.items()}
        emit(kind="contrast", bank=kind, scenes=scenes, rows_per_scene=n, d=d, q=q, m=m, k=K, temperature=tau, iters=ITERS,
             us=us, us_min=lo, spread={k_: (max(v) - min(v)) / min(v) for k_, v in us.items()},
             contrast_over_plain36=lo["contrast"] / lo["plain36"], torch_route_over_contrast=lo["torch_route"] / lo["contrast"],
             parity_max_ulp=int(ulps.max()), parity_share_differing=float((ulps != 0).mean()))


def ensemble():
    scenes, n, d, q, m, tau = 8, 150_000, 768, 32, 4, 0.1
    gen = torch.Generator(device=dev).manual_seed(4)
    a16, b16 = make_bank(scenes, n, d, gen), make_bank(scenes, n, d, gen)
    rows = torch.nn.functional.normalize(torch.randn(q + m, d, generator=gen, device=dev), dim=1).half()
    text, negs = rows[:q].contiguous(), rows[q:].contiguous()
    empty = torch.zeros(1, dtype=torch.int64, device=dev)
    for kind, a, b in (("fp16", a16, b16), ("fp8", a16.to_fp8(), b16.to_fp8())):
        for neg in (None, negs):
            kw = dict(k=K, return_heat=True, negatives=neg, temperature=tau)
            if kind == "fp16":
                def plain_heat():
                    return ops.bank_search(a.features, empty, text, k=K, want_heat=True, max_scene_rows=0, negatives=neg, temperature=tau)
            else:
                def plain_heat():
                    return ops.bank_search_fp8(a.codes, a.exponents, empty, text, k=K, want_heat=True, max_scene_rows=0, negatives=neg,
                                               temperature=tau)
            for mode in ops.BANK_ENSEMBLE_MODES:
                def ours():
                    return search(a, text, ensemble=b, ensemble_mode=mode, **kw)

                if kind == "fp16":
                    def ours_heat():
                        return ops.bank_search_ensemble(a.features, b.features, empty, text, k=K, want_heat=True, max_scene_rows=0,
                                                        negatives=neg, temperature=tau, mode=mode)
                else:
                    def ours_heat():
                        return ops.bank_search_ensemble_fp8(a.codes, a.exponents, b.codes, b.exponents, empty, text, k=K, want_heat=True,
                                                            max_scene_rows=0, negatives=neg, temperature=tau, mode=mode)

                def composed_heat():
                    xa, xb = search(a, text, **kw).heat, search(b, text, **kw).heat
                    if mode == "query":
                        source = xa.float() < xb.float()
                        return torch.where(source, xb, xa), source
                    na, nb = (xa, xb) if neg is None else (search(a, text, k=K, return_heat=True).heat, search(b, text, k=K, return_heat=True).heat)
                    source = na.float().max(dim=1)[0] < nb.float().max(dim=1)[0]
                    return torch.where(source[:, None], xb, xa), source

                def composed_route():
                    heat, source = composed_heat()
                    return heat, source, [torch.topk(heat[o:e].t().float(), min(K, e - o), dim=1) for o, e in zip(a.offsets[:-1], a.offsets[1:])]

                def plain():
                    return search(a, text, **kw)
                got, (want_heat, want_source) = ours(), composed_heat()
                if not (torch.equal(got.heat.view(torch.int16), want_heat.view(torch.int16)) and torch.equal(got.source, want_source)):
                    raise SystemExit("the ensemble's heat-map or source is not the composed one (%s %s)" % (kind, mode))
                share = want_source.double().mean().item()
                del got, want_heat, want_source
                us = {"ensemble": [], "ensemble_heat": [], "composed": [], "composed_heat": [], "plain": [], "plain_heat": []}
                for _ in range(ROUNDS):                        # A B C A B C: shows the spread
                    us["ensemble"].append(timed(ours))
                    us["ensemble_heat"].append(timed(ours_heat))
                    us["plain"].append(timed(plain))
                    us["plain_heat"].append(timed(plain_heat))
                    us["composed"].append(timed(composed_route, iters=max(3, ITERS // 4), warmup=1))
                    us["composed_heat"].append(timed(composed_heat, iters=max(3, ITERS // 4), warmup=1))
                lo = {k_: min(v) for k_, v in us.items()}
                emit(kind="ensemble", bank=kind, mode=mode, scenes=scenes, rows_per_scene=n, d=d, q=q, m=0 if neg is None else m, k=K,
                     temperature=tau, iters=ITERS, share_from_second=share, us=us, us_min=lo,
                     spread={k_: (max(v) - min(v)) / min(v) for k_, v in us.items()},
                     composed_over_ensemble=lo["composed"] / lo["ensemble"],
                     composed_heat_over_ensemble_heat=lo["composed_heat"] / lo["ensemble_heat"],
                     ensemble_over_two_plain=lo["ensemble"] / (2 * lo["plain"]),
                     ensemble_heat_over_two_plain_heat=lo["ensemble_heat"] / (2 * lo["plain_heat"]))


if __name__ == "__main__":
    if "--ensemble-only" in sys.argv:
        ensemble()
        sys.exit(0)
    if not CONTRAST_ONLY:
        shapes()
        append()
    contrast()
