"""The fp8 bank's format restated in torch (CPU), its scores in float64, and CPU stand-ins for the two fp8 kernels
(tests/test_search_fp8_cpu.py).

A row x is stored as d e4m3fn codes and one exponent e: value = code * 2^e, e the smallest integer >= -120 with
max|x| * 2^-e <= 448 (0 for a zero row and for a row with a non-finite element, whose codes are all NaN)."""
import torch

import search_reference as sr


def quantize(x):
    """float32 / float16 [N, d] -> (codes uint8 [N, d], exponents int8 [N]), on the CPU."""
    x = x.detach().cpu().float()
    bad = ~torch.isfinite(x).all(dim=1)
    amax = torch.where(bad[:, None], torch.zeros_like(x), x).abs().amax(dim=1)
    m, ex = torch.frexp(amax)                                # amax = m * 2^ex, m in [0.5, 1)
    e = torch.where(m <= 0.875, ex - 9, ex - 8).clamp(min=-120)
    e = torch.where((amax == 0) | bad, torch.zeros_like(e), e)
    scaled = torch.ldexp(x, -e[:, None])                     # exact
    scaled[bad] = float("nan")
    codes = scaled.to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, e.to(torch.int8)


def code_values():
    """float64 [256]: the value of every e4m3fn code."""
    return torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double()


def dequantize(codes, exps):
    """float64 [N, d]: code * 2^e."""
    c = code_values()[codes.cpu().long()]
    return c * torch.pow(torch.tensor(2.0, dtype=torch.float64), exps.cpu().double())[:, None]


def scores_f64(codes, exps, t, normalize):
    """float64 evaluation of the fp8 score: acc * 2^e / (sqrt(sum c^2) * 2^e + 1e-5) (normalize) or acc * 2^e."""
    c = code_values()[codes.cpu().long()]
    s = torch.pow(torch.tensor(2.0, dtype=torch.float64), exps.cpu().double())[:, None]
    acc = c @ t.cpu().double().t()
    if normalize:
        return acc * s / (c.square().sum(dim=1, keepdim=True).sqrt() * s + 1e-5)
    return acc * s


def same_codes(codes, exps, ref_codes, ref_exps):
    """Bit for bit, an e4m3 NaN being any code with code & 0x7F == 0x7F."""
    codes, ref_codes = codes.cpu(), ref_codes.cpu()
    nan, ref_nan = (codes & 0x7F) == 0x7F, (ref_codes & 0x7F) == 0x7F
    return (codes.shape == ref_codes.shape and torch.equal(exps.cpu(), ref_exps.cpu()) and torch.equal(nan, ref_nan)
            and torch.equal(codes[~nan], ref_codes[~nan]))


# ---- CPU stand-ins for ops.bank_append_fp8 / ops.bank_search_fp8 (host-logic tests only)
def bank_append_fp8(codes, exps, row0, feats, err, gather=None):
    idx = torch.arange(feats.shape[0]) if gather is None else gather.long()
    ok = (idx >= 0) & (idx < feats.shape[0])
    if not bool(ok.all()):
        err |= 1
    dst = torch.arange(idx.shape[0])[ok] + int(row0)
    c, e = quantize(feats[idx[ok]])
    codes[dst] = c
    exps[dst] = e
    return idx.shape[0]


def bank_search_fp8(codes, exps, scene_offsets, queries, k=16, thresholds=None, normalize=True, want_heat=False, max_scene_rows=None,
                    err=None):
    heat = scores_f64(codes, exps, queries, normalize).half()
    top_s, top_p, counts = sr.select(heat, scene_offsets.tolist(), k, thresholds)
    return (heat if want_heat else None), top_s, top_p, counts
