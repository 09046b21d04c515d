"""The contract of tests/search_bounds.py, proved on the CPU before a kernel is held to it: the header's score expressions in emulated
fp32 lie inside every interval, at a worst position <= 0.5; the same emulation with ONE defect (search_bounds.MUTANTS) leaves the
contract on exactly the cases search_bounds.CATCHES names; four of the eleven defects passed everything the suite had before
(NOT_CAUGHT_BEFORE); DELTA is measured here; the float64 reference alone names the best row of a scene for all but a few per cent of
the (scene, query) pairs; and the operands are what their names say.

The fp8 exponent rows.  The float64 score of every row of the "exponents" kind is finite and a cosine in [-1, 1] at every exponent
byte.  The expression the fp8 kernel had, acc * 2^e / (sqrtf(ss) * 2^e + 1e-5f), evaluated in fp32:
    e = 113    inside the contract on every row at every width here (||c|| <= 448 sqrt(768) < 2^14: nothing reaches 2^128 below e = 115)
    e = 120    outside on every row at every width, 42 of 42: the largest code of a row is above 224, so ||c|| 2^120 passes 2^128
               as soon as ||c|| reaches 256.  The score is +-0 where acc * 2^e stayed finite over the infinite denominator (about
               2340 of 2730 scores) and NaN where it did not (inf / inf).  On the device the parent commit gave the same zeros.
    rows of +-448 * 2^e at d = 768 (||c|| = 2^13.6): the first exponent that leaves the contract is e = 115.
The header's present form, acc / (sqrtf(ss) + 1e-5f / 2^e), is inside at every exponent, and gives the same bits wherever the old
one was inside (asserted on every fp8 case)."""
import numpy as np
import pytest
import torch

import query_bounds as qb
import search_bounds as sb
import search_fp8_reference as f8


def _cases(bank):
    return [(kind, d) for kind in sb.kinds(bank) for d in sb.WIDTHS[bank]]


# ------------------------------------------------------------------------------------------------- the emulation meets the contract
@pytest.mark.parametrize("bank", sb.BANKS)
def test_the_emulation_lies_inside_the_contract_on_every_case(bank):
    worst = 0.0
    for kind, d in _cases(bank):
        st, t = sb.stored(bank, kind, d), sb.operands(bank, kind, d)[1]
        for nz in (0, 1):
            ratio = sb.within(sb.emulate(st, t, nz), sb.reference(bank, kind, d, nz), "%s %s d=%d normalize=%d" % (bank, kind, d, nz))
            worst = max(worst, ratio)
    print("%s: worst position of the emulation %.3f" % (bank, worst))
    assert worst <= 0.5


def test_the_smaller_cases_are_slices_of_the_shared_reference():
    bank, kind, d = "fp16", "row_scales", 136
    t = sb.operands(bank, kind, d)[1]
    for n, q in ((1, 1), (129, 33)):
        ref = sb.interval(sb.values(sb.stored(bank, kind, d))[:n], t[:q].double().numpy(), 1)
        cut = sb.cut(sb.reference(bank, kind, d, 1), n, q)
        # (a BLAS product of fewer rows may sum in another order: the float64 values agree to rounding, the fp16 ends all but always)
        assert np.allclose(ref.centre, cut.centre, rtol=1e-12, atol=0, equal_nan=True)
        assert (ref.lo.view(np.uint16) != cut.lo.view(np.uint16)).mean() < 1e-3 and ref.zero.tolist() == cut.zero.tolist()


# ----------------------------------------------------------------------------------------------------------------- the mutants
def test_the_table_names_every_mutant():
    assert set(sb.CATCHES) == set(sb.MUTANTS) and all(sb.CATCHES[m] for m in sb.MUTANTS)
    assert all(set(sb.CATCHES[m]) <= set(sb.CASES) for m in sb.MUTANTS)
    assert all(all(sb.CASES[c][0] == "fp8" for c in sb.CATCHES[m]) for m in sb.FP8_ONLY)
    assert {sb.CASES[c][2] for c in sb.CASES} == set(sb.WIDTHS["fp16"]) | set(sb.WIDTHS["fp8"])      # every width has a named case


@pytest.mark.parametrize("mutant", sb.MUTANTS)
def test_mutant_leaves_the_contract_on_exactly_its_cases(mutant):
    possible = [c for c in sb.CASES if not (sb.CASES[c][0] == "fp16" and mutant in sb.FP8_ONLY)]
    got = tuple(c for c in possible if sb.caught(mutant, c))
    print("%-36s caught by %s" % (mutant, ", ".join(got)))
    assert set(got) == set(sb.CATCHES[mutant]), (mutant, sorted(set(got) ^ set(sb.CATCHES[mutant])))


def test_what_the_suite_had_before_could_not_see():
    assert not sb.legacy_check(None)                    # the right arithmetic passes the older check
    passed = tuple(m for m in sb.MUTANTS if not sb.legacy_check(m))
    print("not caught by unit_rows with abs <= %g: %s" % (sb.LEGACY_TOL, ", ".join(passed)))
    assert passed == sb.NOT_CAUGHT_BEFORE and len(passed) > 0
    assert all(sb.CATCHES[m] for m in passed)           # ... and every one of them leaves the contract


# ---------------------------------------------------------------------------------------------------------------------- DELTA
def test_delta_is_four_times_the_measured_error_of_the_denominator():
    worst = {}
    for bank, lanes in (("fp16", 16), ("fp8", 8)):
        for kind, d in _cases(bank):
            st = sb.stored(bank, kind, d)
            v = st.h.float().numpy() if bank == "fp16" else f8.code_values()[st.codes.long()].float().numpy()
            v = v[np.isfinite(v).all(1)]
            for order in ("lanes", "ascending"):
                e = sb.denominator_error(v, order, lanes)
                if e > worst.get((bank, order), (0.0,))[0]:
                    worst[bank, order] = (e, kind, d)
    for (bank, order), (e, kind, d) in sorted(worst.items()):
        print("DELTA %s rows, %-9s order: worst relative error %.3e (%s, d = %d)" % (bank, order, e, kind, d))
    top = max(e for e, _, _ in worst.values())
    print("four times the worst: %.3e; DELTA = %.3e; query_bounds.DELTA = %.3e" % (4 * top, sb.DELTA, qb.DELTA))
    assert 4 * top <= sb.DELTA <= 4 * top * 1.05        # rounded up, not padded
    assert sb.DELTA > qb.DELTA                          # (else that constant would have been imported)
    assert max(worst["fp16", "lanes"][0], worst["fp8", "lanes"][0]) < 3e-7      # the kernels' own order is far inside


# ------------------------------------------------------------------------------------------------------------------ top 1
def test_float64_alone_names_the_best_row_of_nearly_every_scene_and_query():
    worst = (-1.0, ())
    for bank in sb.BANKS:
        for kind, d in _cases(bank):
            for nz in (0, 1):
                if kind == "exponents" and not nz:
                    continue
                ref = sb.reference(bank, kind, d, nz)
                for n in sb.NS:
                    for q in sb.QS:
                        share = sb.undecided_share(sb.cut(ref, n, q), sb.offsets(n))
                        worst = max(worst, (share, (bank, kind, d, nz, n, q)))
                        assert share <= 0.05, (bank, kind, d, nz, n, q, share)
    print("largest undecided share %.3f at %r" % worst)


def test_top1_decided_on_a_hand_made_reference():
    lo = np.array([[1.0, 1.0, np.nan], [3.0, 2.0, 1.0], [2.0, 2.0, 0.25], [0.0, 5.0, 0.0]], dtype=np.float16)
    ref = sb.Ref(lo.astype(np.float64), None, None, lo, lo + np.float16(0.5), np.zeros(4, dtype=bool))
    (s0, w0, d0), (s1, w1, d1) = sb.top1_decided(ref, [0, 0, 3, 4])
    assert (s0, s1) == (1, 2)
    assert w0.tolist() == [1, 1, 1] and d0.tolist() == [True, False, True]      # 3 > 2.5; 2 vs 2.5; NaN ranks last
    assert w1.tolist() == [0, 0, 0] and d1.tolist() == [True, True, True]


# ---------------------------------------------------------------------------------------------------------- the fp8 exponent rows
def test_exponent_rows_quantise_to_the_planted_exponents_and_every_sweep_holds_two():
    for d in sb.WIDTHS["fp8"]:
        st = sb.stored("fp8", "exponents", d)
        want = torch.tensor([sb.EXPS[i % 7] for i in range(sb.N)], dtype=torch.int8)
        want[sb.PLANTED["zero"]] = 0
        assert torch.equal(st.exps, want)
    for kind, d in _cases("fp8"):
        e = sb.stored("fp8", kind, d).exps
        for n in (129, 300):
            for a in range(0, n, 32):
                assert len(set(e[a:min(a + 32, n)].tolist())) >= 2 or min(a + 32, n) - a < 2, (kind, d, n, a)
        assert (e[:-1] != e[1:]).float().mean() > 0.5       # most rows differ from their neighbour r ^ 1


def test_exponent_rows_float64_is_a_cosine_and_the_scaled_denominator_overflows():
    record = {}
    for d in sb.WIDTHS["fp8"]:
        st, t = sb.stored("fp8", "exponents", d), sb.operands("fp8", "exponents", d)[1]
        ref = sb.reference("fp8", "exponents", d, 1)
        assert np.isfinite(ref.centre).all() and np.abs(ref.centre).max() <= 1.0
        assert not sb.outside(sb.emulate(st, t, 1), ref).any()
        old = sb.emulate(st, t, 1, fp8_form="scaled_denominator")
        out = sb.outside(old, ref).any(1)
        for e in sb.EXPS:
            rows = np.nonzero(st.exps.numpy() == e)[0]
            record[d, e] = (int(out[rows].sum()), len(rows), int((old[rows][out[rows]] == 0).sum()), int(np.isnan(old[rows]).sum()))
            if e in (113, 120):
                print("acc * 2^e / (sqrtf(ss) * 2^e + 1e-5f) at d = %d, e = %d: %d of %d rows outside (%d scores 0, %d NaN)"
                      % ((d, e) + record[d, e]))
            if e < 115:
                assert record[d, e][0] == 0
    assert all(record[d, 120][0] >= 2 * record[d, 120][1] // 3 - 1 for d in sb.WIDTHS["fp8"])
    assert record[768, 120][2] > 0 and record[768, 120][3] > 0


def test_the_scaled_denominator_breaks_from_e_115_at_d_768_and_agrees_bit_for_bit_below():
    d = 768
    g = torch.Generator().manual_seed(5)
    t = qb.text("unit", 33, d, g).half()
    first = None
    for e in range(100, 120):
        x = torch.ldexp(torch.where(torch.rand(4, d, generator=g) < 0.5, -448.0, 448.0), torch.tensor(e))
        st = sb.Stored("fp8", None, *f8.quantize(x))
        assert st.exps.tolist() == [e] * 4
        ref = sb.interval(sb.values(st), t.double().numpy(), 1)
        new, old = sb.emulate(st, t, 1), sb.emulate(st, t, 1, fp8_form="scaled_denominator")
        assert not sb.outside(new, ref).any()
        if sb.outside(old, ref).any():
            first = e if first is None else first
        else:
            assert first is None and np.array_equal(new.view(np.uint16), old.view(np.uint16))
    print("rows of +-448 * 2^e at d = 768: the scaled denominator leaves the contract from e = %d" % first)
    assert first == 115


@pytest.mark.parametrize("kind,d", _cases("fp8"))
def test_the_two_fp8_forms_agree_bit_for_bit_where_the_scaled_one_is_inside(kind, d):
    st, t = sb.stored("fp8", kind, d), sb.operands("fp8", kind, d)[1]
    ref = sb.reference("fp8", kind, d, 1)
    new, old = sb.emulate(st, t, 1), sb.emulate(st, t, 1, fp8_form="scaled_denominator")
    inside = ~sb.outside(old, ref)
    assert np.array_equal(new.view(np.uint16)[inside], old.view(np.uint16)[inside])
    assert kind == "exponents" or inside.all()


# ------------------------------------------------------------------------------------------------ the operands are what they claim
def test_planted_rows_and_kinds_are_what_they_claim():
    P = sb.PLANTED
    for bank in sb.BANKS:
        for kind in sb.KINDS:
            for d in sb.WIDTHS[bank]:
                v = sb.values(sb.stored(bank, kind, d))
                norm = np.sqrt(np.nansum(v * v, axis=1))
                assert (v[P["zero"]] == 0).all() and (v[P["minus_zero"]] == 0).all() and np.signbit(v[P["minus_zero"]]).sum() == 1
                for name, want in (("norm_1e-7", 1e-7), ("norm_1e-5", 1e-5), ("norm_1e-3", 1e-3)):
                    assert 0.5 * want < norm[P[name]] < 2 * want, (bank, kind, d, name, norm[P[name]])
                sub = v[P["subnormals"]]
                assert (np.abs(sub) < 2.0 ** -14).all() if bank == "fp16" else (np.abs(sub) <= 2.0 ** -14).all()
                assert (sub != 0).sum() > d // 2
                assert (v[P["pos60000"]] > 5e4).all() and (v[P["neg60000"]] < -5e4).all()
                assert np.array_equal(v[P["twin_a"]], v[P["twin_b"]]) and P["twin_a"] // 128 != P["twin_b"] // 128
                assert np.isnan(v[P["one_nan"]]).any()
                assert (np.isinf(v[P["one_inf"]]).sum() == 1) if bank == "fp16" else np.isnan(v[P["one_inf"]]).all()
                for n in (129, 300):                     # at most one row of a scene can score +inf
                    o = sb.offsets(n)
                    assert o[1] <= P["pos60000"] < o[2] <= P["one_inf"] < o[3] and o[2] <= P["flat"]
                ref = sb.reference(bank, kind, d, 0)
                assert np.isinf(ref.lo[P["pos60000"]]).any() or d < 136          # raw scores overflow
    h = sb.stored("fp16", "wide_elements", 768).h
    ordinary = h[10:100]
    assert ((ordinary.abs() < 2.0 ** -14) & (ordinary != 0)).float().mean() > 0.2 and (ordinary == 0).float().mean() > 5e-4
    norms = sb.stored("fp16", "row_scales", 136).h[10:100].float().norm(dim=1)
    assert norms.max() / norms.min() > 1e5 and torch.isfinite(norms).all()      # many decades inside one 128-row tile
    x, t = sb.operands("fp16", "coherent", 768)
    assert (x[10:100] > 0).all() and (t >= 0).all()
    assert sb.fed_as_fp16("fp16", "unit") and not sb.fed_as_fp16("fp16", "half_ties") and not sb.fed_as_fp16("fp8", "unit")
    x = sb.operands("fp16", "half_ties", 136)[0][10:100]
    assert (x.half().float() != x).float().mean() > 0.3                          # the append has something to round
