"""The arithmetic contract of the bank search's heat-maps in one place (plain helper module; imported by test_search_bounds_cpu.py
and test_gpu_search_bounds.py).  Stated once more in the header of csrc/search.hip and beside osn_bank_search / osn_bank_search_fp8 in
include/openscene_amd.h.

One score.  v = the stored row in float64 (an fp16 bank: the fp16 row; an fp8 bank: code_k * 2^e), t = the fp16 query,
S = sum v_k t_k, A = sum |v_k| |t_k|, N = sqrt(sum v_k^2), all float64; c = conv_bounds.FWD_C = 2e-6, the project's bound for an
fp32-accumulating MFMA contraction.  Rounding is monotone, so every fp16 score a kernel writes must satisfy
    normalize = 0    fp16_rne(S - c A)  <=  got  <=  fp16_rne(S + c A)
    normalize = 1    fp16_rne(L)  <=  got  <=  fp16_rne(U),   D = N + 1e-5,
                     L, U = the minimum and maximum of (S -+ c A) / (D (1 -+ DELTA)) over the four sign choices
each end rounded from float64 to fp16 in ONE step (numpy's astype(float16)); a raw score beyond the fp16 range is +-inf by that very
rounding.  Special rows are exact: a row of zeros (of either sign) scores +0.0 bit for bit; a row that holds a NaN scores NaN for
every query; a row that holds an inf scores NaN for every query with normalize = 1 and on an fp8 bank (its codes are all NaN), and
S itself (+-inf, NaN where the query is zero at that element) with normalize = 0 on an fp16 bank.

DELTA = 1.4e-5.  Measured in test_search_bounds_cpu.py over every finite row of every operand kind at every width below: the
relative error of fp32 sqrtf(sum of squares) + 1e-5f against float64 sqrt(sum v^2) + 1e-5, the sum taken
    in the kernels' order (norm_fp32 "lanes": the 8 or 16 squares of a 16-byte piece in sequence, the pieces of a lane added over the
    128-wide chunks, a butterfly over the 16 lanes of an fp16 row / the 8 lanes of an fp8 row):   worst 1.46e-7 (fp16), 2.31e-7 (fp8)
    in one ascending chain:                                                                  worst 3.43e-6 (fp16), 5.26e-7 (fp8)
The ascending worst is the rows of 768 elements of one magnitude (norm_1e-3: 3.43e-6, +-60000: 2.54e-6), whose equal addends all
round the same way; random rows stay below 8.6e-7 here, as query_bounds measured (1.07e-6).  So the worse of the two times four,
1.372e-5 rounded up, stands here as a constant of its own, above query_bounds.DELTA = 4.5e-6.  It is 1.4 to 2.9 % of an fp16 step.

Operands (seeded, shared, read-only): operands(bank, kind, d) -> N = 300 rows and Q = 65 queries; the GPU cases with fewer rows or
queries take the first n rows and the first q queries, so one float64 reference per (bank, kind, d, normalize) serves them all.
Ordinary rows: query_bounds.features / query_bounds.text of the six KINDS (for the fp8 bank row i times 2^(i % 3 - 1), exact, so
that neighbouring rows of a 32-row sweep carry different exponents whatever the kind).  Planted rows (PLANTED; row 0 stays ordinary:
it is the n = 1 case):
    zero, minus_zero (one -0.0, else +0.0), norm_1e-7, norm_1e-5, norm_1e-3 (where the 1e-5 of the denominator matters),
    subnormals (fp16 subnormals only), pos60000 / neg60000 (+-60000 in every element: raw scores overflow), twin_a = twin_b (equal rows
    in different 128-row tiles), one_inf, one_nan, flat / flat_neg (+-0.25 everywhere).
The bank is cut at row CUT = 64 into two scenes behind an empty one: the first holds +-60000, the second one_inf and +-flat, so
that at most one row of a scene scores +inf and -- flat and its negative, 60000 and its negative -- the kinds whose ordinary
scores crowd together (coherent, cancellation) still have a winner float64 can name.
The fp8 bank has a seventh kind, "exponents": row i carries the exponent byte EXPS[i % 7] (-120, -60, 0, 60, 100, 113, 120) in one
of three sizes, i // 7 % 3: the sizes of test_gpu_search_fp8.hand_placed_rows (0.01 randn * 2^e and one element, (9 + i) % d, of -250 * 2^e), dense
rows uniform in +-250 * 2^e, and rows of +-250 * 2^e in every element (the largest norm float32 rows can have at e = 120).  Its raw
scores are +-inf or 0 by construction, several +inf a scene: its top 1 is held with normalize = 1 only.

emulate() is the two score expressions as the header states them, in numpy fp32 with the contraction as one ascending chain; mutant=
carries one defect at a time (MUTANTS).  CATCHES names, for every mutant, the cases of CASES (one per bank and kind, both modes) on
which it leaves the contract; NOT_CAUGHT_BEFORE the mutants that pass what the suite had before: unit_rows at the shapes of
test_gpu_search_shared.py with abs <= 2e-3 (legacy_check).  fp8_form="scaled_denominator" is the expression the fp8 kernel had before
this contract was written, acc * 2^e / (sqrtf(ss) * 2^e + 1e-5f): it overflows at large e (test_search_bounds_cpu.py records where).
"""
import collections
import functools

import numpy as np
import torch

import conv_bounds as cb
import query_bounds as qb
import search_fp8_reference as f8
import search_reference as sr

C = cb.FWD_C
DELTA = 1.4e-5
EPS = 1e-5
KINDS = qb.KINDS
FP8_KINDS = KINDS + ("exponents",)
BANKS = ("fp16", "fp8")
WIDTHS = {"fp16": (8, 136, 520, 768), "fp8": (16, 272, 528, 768)}
NS = (1, 129, 300)
QS = (1, 33, 65)
N, Q = 300, 65
CUT = 64                           # scenes: [0, 0), [0, min(CUT, n // 2)), [.., n)
EXPS = (-120, -60, 0, 60, 100, 113, 120)
PLANTED = {"zero": 1, "minus_zero": 2, "norm_1e-7": 3, "norm_1e-5": 4, "norm_1e-3": 5, "twin_a": 6, "subnormals": 7, "pos60000": 8,
           "neg60000": 9, "one_inf": 100, "one_nan": 101, "flat": 102, "flat_neg": 103, "twin_b": 128}
MUTANTS = ("round_toward_zero", "accumulator_rounded_to_fp16_first", "fp16_accumulate", "eps_missing", "eps_scaled_with_the_row",
           "norm_squares_in_fp16", "norm_skips_tail_chunk", "norm_of_neighbour_row", "scale_of_neighbour_row",
           "subnormal_inputs_flushed", "tail_group_dropped")
FP8_ONLY = ("eps_scaled_with_the_row", "scale_of_neighbour_row")


def kinds(bank):
    return FP8_KINDS if bank == "fp8" else KINDS


def offsets(n):
    """The scene offsets of an n-row case: an empty scene, then two."""
    return [0, 0, min(CUT, n // 2), n]


# named cases of the mutant table: one per bank and kind, at one width each (every width occurs), caught = outside in either mode
_CASE_D = {"unit": 3, "row_scales": 1, "wide_elements": 2, "coherent": 3, "cancellation": 1, "half_ties": 0, "exponents": 2}
CASES = {"%s/%s" % (b, k): (b, k, WIDTHS[b][_CASE_D[k]]) for b in BANKS for k in kinds(b)}

# mutant -> the named cases on which it leaves the contract (test_search_bounds_cpu.py asserts exactly these).  The planted rows sit
# in every kind, so most defects show on every case; the two that need a partial chunk do not show at d = 768.  An fp8 bank stores
# no fp16 subnormal (its smallest code is 2^-9; tiny rows live in the exponent): flushed subnormals show there through the query only.
_ALL = tuple(CASES)
_FP8 = tuple(c for c in CASES if CASES[c][0] == "fp8")
_TAILED = tuple(c for c in CASES if CASES[c][2] % 128)          # all but unit and coherent, which sit at d = 768
CATCHES = {
    "round_toward_zero": _ALL,
    "accumulator_rounded_to_fp16_first": _ALL,
    "fp16_accumulate": _ALL,
    "eps_missing": _ALL,                               # (the zero rows alone: 0 / 0)
    "eps_scaled_with_the_row": _FP8,
    "norm_squares_in_fp16": _ALL,
    "norm_skips_tail_chunk": _TAILED,
    "norm_of_neighbour_row": _ALL,
    "scale_of_neighbour_row": _FP8,
    "subnormal_inputs_flushed": tuple(c for c in _ALL if c != "fp8/half_ties"),       # (d = 16: no subnormal in 65 unit queries)
    "tail_group_dropped": _TAILED,
}

# the mutants that pass legacy_check, i.e. what the three older search tests could not see (asserted, all listed)
NOT_CAUGHT_BEFORE = ("round_toward_zero", "accumulator_rounded_to_fp16_first", "eps_scaled_with_the_row", "subnormal_inputs_flushed")


# ---------------------------------------------------------------------------------------------------------------- operands
def _tiny_row(norm, d, g, dense):
    """a row of norm ~ `norm`: every element (dense), or as few elements as keep each one at or above 8 fp16 subnormal steps"""
    m = d if dense else int(min(d, max(1.0, (norm / 2.0 ** -21) ** 2)))
    r = torch.zeros(d)
    sign = torch.where(torch.rand(m, generator=g) < 0.5, -1.0, 1.0)
    r[torch.randperm(d, generator=g)[:m]] = sign * (norm / m ** 0.5)
    return r


def exponent_rows(n, d, g):
    """float32 [n, d]: row i quantises to the exponent byte EXPS[i % 7], in the size i // 7 % 3 of the module docstring."""
    x = torch.empty(n, d)
    for i in range(n):
        e, size = EXPS[i % len(EXPS)], i // len(EXPS) % 3
        if size == 0:
            r = 0.01 * torch.randn(d, generator=g)
            r[(9 + i) % d] = -250.0                # (300 * 2^120 is no float32)
        elif size == 1:
            r = (torch.rand(d, generator=g) * 2 - 1) * 250.0
            r[i % d] = 250.0
        else:
            r = torch.where(torch.rand(d, generator=g) < 0.5, -250.0, 250.0)
        x[i] = torch.ldexp(r, torch.tensor(e))
    return x


@functools.lru_cache(maxsize=None)
def operands(bank, kind, d):
    """(rows float32 [N, d], queries fp16 [Q, d]); shared, never modified.  The rows are what add_scene is given, after .half() for
    the kinds an fp16 bank is fed in fp16 (fed_as_fp16)."""
    g = torch.Generator().manual_seed(cb._seed("search", bank, kind, d))
    t = qb.text("unit" if kind == "exponents" else kind, Q, d, g).half()
    if kind == "exponents":
        x = exponent_rows(N, d, g)
        x[PLANTED["zero"]] = 0.0
        return x, t
    x = qb.features(kind, N, d, g)
    if bank == "fp8":
        x = x * (2.0 ** (torch.arange(N) % 3 - 1).float())[:, None]
    P = PLANTED
    x[P["zero"]] = 0.0
    x[P["minus_zero"]] = 0.0
    x[P["minus_zero"], 5 % d] = -0.0
    for name, norm in (("norm_1e-7", 1e-7), ("norm_1e-5", 1e-5), ("norm_1e-3", 1e-3)):
        x[P[name]] = _tiny_row(norm, d, g, dense=bank == "fp8")
    x[P["subnormals"]] = torch.randint(-1023, 1024, (d,), generator=g).float() * 2.0 ** -24
    x[P["subnormals"], 0] = 2.0 ** -24
    x[P["pos60000"]] = 60000.0
    x[P["neg60000"]] = -60000.0
    x[P["one_inf"], 3 % d] = float("inf")
    x[P["one_nan"], 6 % d] = float("nan")
    x[P["flat"]] = 0.25
    x[P["flat_neg"]] = -0.25
    x[P["twin_b"]] = x[P["twin_a"]]
    return x, t


def fed_as_fp16(bank, kind):
    """An fp16 bank gets half_ties and row_scales as float32 (the append kernel rounds them) and the other kinds as fp16 (copied)."""
    return bank == "fp16" and kind not in ("half_ties", "row_scales")


Stored = collections.namedtuple("Stored", "bank h codes exps")     # h fp16 [n, d] | codes uint8 [n, d], exps int8 [n] (torch, CPU)


@functools.lru_cache(maxsize=None)
def stored(bank, kind, d):
    """What a right append leaves in the bank for operands(bank, kind, d): x.half(), or search_fp8_reference.quantize(x)."""
    x = operands(bank, kind, d)[0]
    if bank == "fp16":
        return Stored(bank, x.half(), None, None)
    codes, exps = f8.quantize(x)
    return Stored(bank, None, codes, exps)


def values(st):
    """float64 numpy [n, d]: the stored values (an fp8 NaN row: NaN)."""
    if st.bank == "fp16":
        return st.h.double().numpy()
    return f8.dequantize(st.codes, st.exps).numpy()


def same_store(bank_obj, st, n):
    """The device bank holds exactly the first n rows of `st` (NaN matched as NaN)."""
    if st.bank == "fp16":
        got, want = bank_obj.features.cpu(), st.h[:n]
        nan = torch.isnan(want)
        return got.shape == want.shape and torch.equal(torch.isnan(got), nan) and sr.same_bits(got[~nan], want[~nan])
    return f8.same_codes(bank_obj.codes, bank_obj.exponents, st.codes[:n], st.exps[:n])


# ------------------------------------------------------------------------------------------------------------ the score interval
fp16_rne = qb.fp16_rne
Ref = collections.namedtuple("Ref", "centre L U lo hi zero")     # float64 exact score and unrounded ends; fp16 ends; zero rows [n]


def interval(v, t, normalize, c=C, delta=DELTA):
    """The contract's interval for stored values v [n, d] and queries t [q, d] (float64 numpy)."""
    v, t = np.asarray(v, dtype=np.float64), np.asarray(t, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        S = v @ t.T
        A = np.abs(v) @ np.abs(t).T
        bad = ~np.isfinite(v).all(1)
        if normalize:
            D = (np.sqrt((v * v).sum(1)) + EPS)[:, None]
            a, b = S - c * A, S + c * A
            L = np.minimum(a / (D * (1 + delta)), a / (D * (1 - delta)))
            U = np.maximum(b / (D * (1 + delta)), b / (D * (1 - delta)))
            centre = S / D
            centre[bad], L[bad], U[bad] = np.nan, np.nan, np.nan
        else:
            fin = np.isfinite(S)
            centre, L, U = S, np.where(fin, S - c * A, S), np.where(fin, S + c * A, S)
    return Ref(centre, L, U, fp16_rne(L), fp16_rne(U), (v == 0).all(1))


@functools.lru_cache(maxsize=None)
def reference(bank, kind, d, normalize):
    """interval() of the stored operands, [N, Q]; computed once, never modified (cases with fewer rows and queries slice it)."""
    return interval(values(stored(bank, kind, d)), operands(bank, kind, d)[1].double().numpy(), normalize)


def cut(ref, n, q):
    return Ref(*(a[:n, :q] for a in ref[:5]), ref.zero[:n])


def _as_np(scores):
    return scores.detach().cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores)


def outside(got, ref):
    """bool [n, q]: the scores that break the contract (a zero row: anything but +0.0, bit for bit)."""
    got = _as_np(got)
    assert got.dtype == np.float16 and got.shape == ref.lo.shape, (got.dtype, got.shape, ref.lo.shape)
    with np.errstate(invalid="ignore"):
        ok = ((ref.lo <= got) & (got <= ref.hi)) | (np.isnan(ref.lo) & np.isnan(got))
    ok[ref.zero] = got.view(np.uint16)[ref.zero] == 0
    return ~ok


def worst_ratio(got, ref):
    """(worst position in the interval, number of scores outside).  Position: how far towards an end of the UNROUNDED interval
    [L, U] the score's own rounding cell reaches from the exact score -- 0 where the score is the rounding of the exact value, 1 at
    the end, inf where a special value is not met."""
    got = _as_np(got)
    bad = outside(got, ref)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        g = qb._wide(got)
        below = 0.5 * (g + qb._wide(np.nextafter(got, np.float16(-np.inf))))
        above = 0.5 * (g + qb._wide(np.nextafter(got, np.float16(np.inf))))
        below = np.where(got == -np.inf, -np.inf, below)
        above = np.where(got == np.inf, np.inf, above)
        up, down = ref.U - ref.centre, ref.centre - ref.L
        pos = np.maximum(np.where(below > ref.centre, (below - ref.centre) / up, 0.0),
                         np.where(above < ref.centre, (ref.centre - above) / down, 0.0))
        pos = np.where(np.isfinite(ref.centre) & ~ref.zero[:, None], pos, 0.0)
        pos = np.where(np.isnan(pos), 0.0, pos)
        pos = np.where(bad & ~(pos > 1), np.inf, pos)           # (outside by a special value or at a rounding boundary)
    return (float(pos.max()) if pos.size else 0.0), int(bad.sum())


def within(got, ref, label):
    ratio, n_bad = worst_ratio(got, ref)
    print("RATIO %s: worst position %.3f, %d outside" % (label, ratio, n_bad))
    assert n_bad == 0, "%s: %d scores outside their interval, worst position %.2f" % (label, n_bad, ratio)
    return ratio


def top1_decided(ref, offs):
    """per non-empty scene: (scene, float64 best row inside the scene int64 [q], bool [q]: that row's lower end lies above every
    other row's upper end).  NaN scores rank below every number, as the selection ranks them."""
    out = []
    lo, hi = ref.lo.astype(np.float64), ref.hi.astype(np.float64)
    for s, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        if b == a:
            continue
        c = np.where(np.isnan(ref.centre[a:b]), -np.inf, ref.centre[a:b])
        w = np.argmax(c, axis=0)
        cols = np.arange(c.shape[1])
        others = np.where(np.isnan(hi[a:b]), -np.inf, hi[a:b])
        others[w, cols] = -np.inf
        low = lo[a:b][w, cols]
        with np.errstate(invalid="ignore"):
            dec = (low > others.max(0)) if b - a > 1 else ~np.isnan(low)
        out.append((s, w, dec))
    return out


def undecided_share(ref, offs):
    d = np.concatenate([dec for _, _, dec in top1_decided(ref, offs)])
    return 1.0 - float(d.mean())


# ------------------------------------------------------------------------------------------------------------------ emulation
F4 = np.float32


def _flush16(a):
    """fp16-valued float32 array with the fp16 subnormals made zero"""
    return np.where(np.abs(a) < 2.0 ** -14, np.copysign(F4(0), a), a).astype(F4)


def contract_fp32(x, t, fp16_acc=False, drop_tail=0):
    """fp32 [n, q]: sum_k x_k t_k as ONE ascending chain from +0 (the products of fp16 values are exact in fp32).  fp16_acc: the
    running sum rounded to fp16 after every step.  drop_tail: the last `drop_tail` elements left out."""
    n, d = x.shape
    acc = np.zeros((n, t.shape[0]), dtype=F4)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(d - drop_tail):
            acc = acc + np.outer(x[:, k], t[:, k])
            if fp16_acc:
                acc = acc.astype(np.float16).astype(F4)
    return acc


def norm_fp32(x, order, lanes=16, fp16_squares=False, whole_chunks_only=False):
    """fp32 [n]: the sum of squares of every row of the fp16-valued float32 array x, taken in `order`: "ascending" (one chain) or
    "lanes" -- the heat kernels': a row's 128-wide chunk is 128 / lanes elements a lane; a lane sums the squares of its piece in
    sequence from 0, adds that to its running sum over the chunks; a butterfly (partner distance 1, 2, ..) joins the lanes.
    lanes = 16 for fp16 rows (8 halfs a lane), 8 for fp8 rows (16 codes a lane)."""
    x = np.asarray(x, dtype=F4)
    n, d = x.shape
    rnd = (lambda a: a.astype(np.float16).astype(F4)) if fp16_squares else (lambda a: a)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = rnd(x * x)
        if whole_chunks_only:
            d = d // 128 * 128
        if order == "ascending":
            s = np.zeros(n, dtype=F4)
            for k in range(d):
                s = rnd(s + sq[:, k])
            return s
        assert order == "lanes"
        piece = 128 // lanes
        ls = np.zeros((n, lanes), dtype=F4)
        for d0 in range(0, d, 128):
            for l in range(lanes):
                j = d0 + l * piece
                if j >= d:
                    break
                s = np.zeros(n, dtype=F4)
                for k in range(j, min(j + piece, d)):
                    s = rnd(s + sq[:, k])
                ls[:, l] = rnd(ls[:, l] + s)
        m = 1
        while m < lanes:
            ls = rnd(ls + ls[:, np.arange(lanes) ^ m])
            m <<= 1
        return ls[:, 0]


def denominator_error(v, order, lanes):
    """Worst relative error over the rows of v (finite, fp16-valued or code-valued) of fp32 sqrtf(sum of squares) + 1e-5f against
    float64."""
    den32 = np.sqrt(norm_fp32(v, order, lanes)).astype(F4) + F4(EPS)
    v64 = np.asarray(v, dtype=np.float64)
    den64 = np.sqrt((v64 * v64).sum(1)) + EPS
    return float((np.abs(den32.astype(np.float64) - den64) / den64).max())


def _toward_zero(v):
    """fp32 -> fp16 by truncation"""
    with np.errstate(over="ignore", invalid="ignore"):
        h = v.astype(np.float16)
        over = np.abs(h.astype(np.float64)) > np.abs(v.astype(np.float64))
        h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h


def emulate(st, t, normalize, mutant=None, fp8_form="header"):
    """fp16 numpy [n, q]: the score expressions of include/openscene_amd.h in fp32 on the stored rows `st` (Stored) and fp16
    queries t (torch):
        fp16 bank   acc / (sqrtf(ss) + 1e-5f)                   | acc
        fp8 bank    acc / (sqrtf(ss) + 1e-5f / 2^e)             | acc * 2^e         (acc, ss over the code values)
    rounded to fp16 once; ss in the kernels' lane order.  mutant: one of MUTANTS, the same arithmetic with that one defect:
      round_toward_zero                  the last rounding truncates
      accumulator_rounded_to_fp16_first  acc goes through fp16 before the scale and the division
      fp16_accumulate                    the running sum of the contraction is fp16
      eps_missing                        no 1e-5 in the denominator
      eps_scaled_with_the_row (fp8)      acc / (sqrtf(ss) + 1e-5f): the 1e-5 on the wrong side of 2^e
      norm_squares_in_fp16               the squares and their sum in fp16
      norm_skips_tail_chunk              the sum of squares over whole 128-wide chunks only
      norm_of_neighbour_row              the denominator of row r ^ 1
      scale_of_neighbour_row (fp8)       the 2^e of row r ^ 1
      subnormal_inputs_flushed           fp16 subnormals of rows and queries read as zero
      tail_group_dropped                 the last 16-byte piece of a row left out of the contraction where d % 128 != 0
    fp8_form="scaled_denominator": acc * 2^e / (sqrtf(ss) * 2^e + 1e-5f), the fp8 expression before the contract (no mutant)."""
    assert mutant is None or mutant in MUTANTS
    fp8 = st.bank == "fp8"
    assert fp8 or mutant not in FP8_ONLY
    tq = t.float().numpy()
    if fp8:
        x = f8.code_values()[st.codes.long()].float().numpy()
        e = st.exps.double().numpy()
        scale, inv = np.exp2(e).astype(F4), np.exp2(-e).astype(F4)
    else:
        x = st.h.float().numpy()
    n, d = x.shape
    piece = 16 if fp8 else 8
    nb = np.minimum(np.arange(n) ^ 1, n - 1)
    if mutant == "subnormal_inputs_flushed":
        x, tq = _flush16(x), _flush16(tq)
    acc = contract_fp32(x, tq, fp16_acc=mutant == "fp16_accumulate",
                        drop_tail=piece if mutant == "tail_group_dropped" and d % 128 else 0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        if mutant == "accumulator_rounded_to_fp16_first":
            acc = acc.astype(np.float16).astype(F4)
        if fp8 and mutant == "scale_of_neighbour_row":
            scale, inv = scale[nb], inv[nb]
        if normalize:
            ss = norm_fp32(x, "lanes", 8 if fp8 else 16, fp16_squares=mutant == "norm_squares_in_fp16",
                           whole_chunks_only=mutant == "norm_skips_tail_chunk")
            root = np.sqrt(ss).astype(F4)
            eps = F4(0) if mutant == "eps_missing" else F4(EPS)
            if not fp8:
                den, num = root + eps, acc
            elif fp8_form == "scaled_denominator":
                assert mutant is None
                den, num = root * scale + eps, acc * scale[:, None]
            elif mutant == "eps_scaled_with_the_row":
                den, num = root + eps, acc
            else:
                assert fp8_form == "header"
                den, num = root + eps * inv, acc
            if mutant == "norm_of_neighbour_row":
                den = den[nb]
            v = (num / den[:, None]).astype(F4)
        else:
            v = (acc * scale[:, None]).astype(F4) if fp8 else acc
        return _toward_zero(v) if mutant == "round_toward_zero" else v.astype(np.float16)


def caught(mutant, case):
    """A mutant leaves the contract on a named case: some score outside in either mode."""
    bank, kind, d = CASES[case]
    st, t = stored(bank, kind, d), operands(bank, kind, d)[1]
    return any(outside(emulate(st, t, nz, mutant), reference(bank, kind, d, nz)).any() for nz in (0, 1))


# --------------------------------------------------------------------------------------------------- what the suite had before
LEGACY_TOL = 2e-3
LEGACY_D = {"fp16": (8, 136, 384), "fp8": (128, 272, 384, 512)}          # test_gpu_search_shared.py


def legacy_check(mutant):
    """True where the check of test_gpu_search_shared.py (its rows_with_edges input at n = 300, q = 65, NaN rows NaN, zero rows 0,
    abs <= 2e-3 against the float64 formulas) would have failed the emulation with `mutant`."""
    for bank in BANKS:
        if bank == "fp16" and mutant in FP8_ONLY:
            continue
        for d in LEGACY_D[bank]:
            for nz in (1, 0):
                g = torch.Generator().manual_seed(100 * d + 10 * nz + (bank == "fp8"))
                x = sr.unit_rows(300, d, g)
                zero, nan = [2, 299], [5, 200]
                x[zero] = 0
                for r in nan:
                    x[r, r % d] = float("nan")
                t = sr.text(65, d, g)
                ok = torch.ones(300, dtype=torch.bool)
                ok[nan] = False
                if bank == "fp16":
                    st = Stored(bank, x.half(), None, None)
                    refs = [sr.scores_f64(st.h, t, nz, round_normalised=r) for r in (False, True)]
                else:
                    st = Stored(bank, None, *f8.quantize(x))
                    refs = [f8.scores_f64(st.codes, st.exps, t, nz)]
                heat = torch.from_numpy(emulate(st, t, nz, mutant))
                if not (torch.isnan(heat[nan]).all() and not torch.isnan(heat[ok]).any() and bool((heat[zero] == 0).all())):
                    return True
                if max((heat.double() - ref)[ok].abs().max().item() for ref in refs) > LEGACY_TOL:
                    return True
    return False
