"""Bank rows matched to exemplars on the device (csrc/match.hip: osn_bank_unit_rows, osn_bank_match and their _fp8 twins through
openscene_amd.match), under the conditions tests/match_reference.py states and tests/test_match_cpu.py holds a CPU evaluation to.

Operands: unit_rows bit for bit the Gram matrix's operand.  Bound: L = 300, k = 8, d in {24, 520, 768, 1024} (with an fp8 bank
on either side {16, 528, 768, 1024}: an fp8 row is a multiple of 16 wide) x M in {9, 129, 700, 4226} -- five query tiles with a
ragged last one; fewer exemplars than k + 1, one tile and a row, six tiles, 34 tiles cut into 34 parts -- S and A taken on
unit_rows' own bits of both sides.  Exact: small integers against a stable integer argsort, with many ties.  Purity, specials,
guards, and the planted scenes end to end.  The functional claim -- no L x M array -- is the workspace bound."""
import functools

import pytest
import torch

import gram_reference as gr
import match_reference as mr
import search_reference as sr

pytestmark = pytest.mark.gpu

KINDS = ("fp16", "fp8")


def dev():
    return torch.device("cuda", 0)


def make_bank(kind, scenes):
    from openscene_amd.search import FeatureBank
    bank = FeatureBank(scenes[0].shape[1], dev(), capacity_rows=8, dtype=kind)
    for i, f in enumerate(scenes):
        bank.add_scene("scene%d" % i, f.to(dev()))
    return bank


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    """two results equal bit for bit"""
    return (torch.equal(a.idx, b.idx) and torch.equal(bits(a.score), bits(b.score)) and torch.equal(a.count, b.count))


def rows_on_device(rows):
    return None if rows is None else torch.as_tensor(rows, dtype=torch.int64).to(dev())


def ws_bound(l, m, d, k, splits):
    from openscene_amd import ops
    got = ops.bank_match_ws_bytes(l, m, d, k, splits)
    parts = ops.BANK_MATCH_MAX_SPLITS if splits is None else splits
    assert got <= 8 * l * k * parts + 8192, (l, m, d, k, splits, got)
    return got


# ------------------------------------------------------------------------------------------------------------ operands
@pytest.mark.parametrize("kind,d", [("fp16", 24), ("fp16", 520), ("fp16", 1024), ("fp8", 16), ("fp8", 528), ("fp8", 1024)])
@pytest.mark.parametrize("normalize", [True, False])
def test_unit_rows_are_the_gram_matrixs_operands_bit_for_bit(kind, d, normalize):
    from openscene_amd.descriptors import PointGroups
    from openscene_amd.match import unit_rows
    from openscene_amd.pca import moments
    gen = torch.Generator().manual_seed(d + 3)
    bank = make_bank(kind, [sr.unit_rows(40, d, gen).half()])
    rows = torch.randperm(40, generator=gen).to(dev())
    groups = PointGroups(torch.arange(41).to(dev()), rows, n_entries=40)         # forty groups of one row each
    want = moments(bank, groups, normalize=normalize).sum
    got = unit_rows(bank, rows, normalize=normalize)
    assert got.dtype == torch.float16 and got.shape == (40, d)
    assert torch.equal(want.half().float(), want)                               # the sum of one operand is the operand
    assert sr.same_bits(got, want.half())
    assert sr.same_bits(unit_rows(bank, None, normalize=normalize)[rows], got)


# ------------------------------------------------------------------------------------------------------------ bound
@functools.lru_cache(maxsize=None)
def side(kind, d, m, which):
    """(bank, its operand image as float64 on the host) of the query rows (which = 0) or the exemplar rows (1) of a case"""
    from openscene_amd.match import unit_rows
    bank = make_bank(kind, [mr.rows_case(d, m)[which]])
    return bank, mr.operands_f64(unit_rows(bank))


@pytest.mark.parametrize("at", range(4))
@pytest.mark.parametrize("qkind,ekind", [(q, e) for q in KINDS for e in KINDS])
def test_scores_order_and_counts_against_float64(qkind, ekind, at):
    from openscene_amd.match import Exemplars, match
    d = (mr.DIMS_FP16 if (qkind, ekind) == ("fp16", "fp16") else mr.DIMS_FP8)[at]
    for m in mr.MS:
        qbank, a = side(qkind, d, m, 0)
        ebank, b = side(ekind, d, m, 1)
        ex = Exemplars(ebank)
        assert sr.same_bits(ex.image.cpu(), b.half())
        got = match(qbank, ex, k=mr.K)
        assert got.idx.dtype == torch.int32 and got.count.dtype == torch.int32
        s, aa = mr.scores(a, b)
        label = "%s x %s d=%d M=%d" % (qkind, ekind, d, m)
        worst, undecided = mr.check(got.idx, got.score, got.count, s, aa, mr.K, label=label)
        print("%s: worst err / limit %.3f, undecided rows %.4f" % (label, worst, undecided))
        assert undecided <= mr.UNDECIDED_MAX
        ws_bound(mr.L_ROWS, m, d, mr.K, None)


def test_the_workspace_never_grows_with_rows_times_exemplars():
    from openscene_amd import ops
    for l, m in ((150000, 150000), (1200000, 20000), (64, 150000), (1, 1), (300, 4226)):
        for k in (1, 8):
            for splits in (None, 1, 7, 64):
                ws_bound(l, m, 768, k, splits)
    assert ws_bound(150000, 150000, 768, 8, None) <= 8 * 150000 * 8 + 8192      # a full grid is not split: 9.6 MB, not 45 GB
    assert ops.BANK_MATCH_MAX_K == 8


# ------------------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("kind,d", [("fp16", 24), ("fp16", 520), ("fp16", 768), ("fp8", 16), ("fp8", 528), ("fp8", 768)])
def test_small_integers_give_the_stable_integer_argsort_bit_for_bit(kind, d):
    """|v| <= 8: every sum (at most 64 * 768 < 2^24) is an integer that float32 holds whatever the order; duplicated exemplars
    and zero rows make ties in every list -- a tile-edge, position or tie-rule error shows."""
    from openscene_amd.match import Exemplars, match
    for m in (1, 5, 127, 128, 129, 255, 256, 257, 700):                         # (the tile is 256 exemplars, a wave takes 64)
        xa, xb = mr.integer_case(d, m)
        qbank, ebank = make_bank(kind, [xa.half()]), make_bank(kind, [xb.half()])
        ex = Exemplars(ebank, normalize=False)
        assert torch.equal(ex.image.cpu().long(), xb)
        for k in (1, 8):
            got = match(qbank, ex, k=k)
            mr.check_exact(got.idx, got.score, got.count, xa, xb, k)


# ------------------------------------------------------------------------------------------------------------ purity
@pytest.mark.parametrize("kind,d,m", [("fp16", 768, 700), ("fp8", 528, 4226), ("fp16", 24, 129)])
def test_the_result_is_a_function_of_the_operand_rows_alone(kind, d, m):
    from openscene_amd.match import Exemplars, match
    qbank, _ = side(kind, d, m, 0)
    ebank, _ = side("fp16", d, m, 1)
    ex = Exemplars(ebank)
    got = match(qbank, ex, k=8)
    assert same(match(qbank, ex, k=8), got)                                     # two calls
    for splits in (1, 2, 7):                                                    # the split of the exemplars
        assert same(match(qbank, ex, k=8, splits=splits), got), splits
        ws_bound(mr.L_ROWS, m, d, 8, splits)
    three = match(qbank, ex, k=3)                                               # k
    assert torch.equal(three.idx, got.idx[:, :3]) and torch.equal(bits(three.score), bits(got.score[:, :3]))
    gen = torch.Generator().manual_seed(m)
    perm = torch.randperm(m, generator=gen).to(dev())                           # the exemplars' positions
    moved = match(qbank, Exemplars(ebank, rows=perm), k=8)
    assert torch.equal(bits(moved.score), bits(got.score)) and torch.equal(moved.rows, got.rows)
    qperm = torch.randperm(mr.L_ROWS, generator=gen).to(dev())                  # the query rows' positions
    assert same(match(qbank, ex, k=8, rows=qperm), type(got)(got.idx[qperm], got.score[qperm], got.count[qperm], ex))
    for n_rows in (1, 64, 65):                                                  # one tile, its edge, and a row more
        part = match(qbank, ex, k=8, rows=qperm[:n_rows])
        assert torch.equal(part.idx, got.idx[qperm[:n_rows]]) and torch.equal(bits(part.score), bits(got.score[qperm[:n_rows]]))
    for j in got.idx[0, :2].tolist() + [m - 1]:                                 # an exemplar alone
        alone = match(qbank, Exemplars(ebank, rows=rows_on_device([j])), k=1)
        held = got.idx == j
        assert bool(held.any(dim=1).sum() > 0) or j == m - 1
        assert torch.equal(bits(alone.score[:, 0][held.any(dim=1)]), bits(got.score[held]))


# ------------------------------------------------------------------------------------------------------------ specials
def test_a_nan_row_on_either_side_stays_in_its_own_list():
    from openscene_amd.match import Exemplars, match
    gen = torch.Generator().manual_seed(31)
    d, m, k = 64, 300, 8
    xq, xe = sr.unit_rows(100, d, gen).half(), sr.unit_rows(m, d, gen).half()
    ex = Exemplars(make_bank("fp16", [xe]))
    clean = match(make_bank("fp16", [xq]), ex, k=k)
    xq_nan = xq.clone()
    xq_nan[41, 7] = float("nan")
    got = match(make_bank("fp16", [xq_nan]), ex, k=k)
    assert bool(torch.isnan(got.score[41]).all()) and got.idx[41].tolist() == list(range(k))
    others = torch.arange(100) != 41
    assert torch.equal(got.idx.cpu()[others], clean.idx.cpu()[others])
    assert torch.equal(bits(got.score).cpu()[others], bits(clean.score).cpu()[others])
    # a NaN exemplar: last in a list that holds every exemplar, in no list otherwise; the other exemplars as without it
    at = 150
    xe_nan = xe.clone()
    xe_nan[at, 3] = float("nan")
    ebank = make_bank("fp16", [xe_nan])
    qbank = make_bank("fp16", [xq])
    few = match(qbank, Exemplars(ebank, rows=rows_on_device([2, at, 9, 4])), k=4)
    assert bool((few.idx[:, 3] == 1).all()) and bool(torch.isnan(few.score[:, 3]).all())
    assert not bool(torch.isnan(few.score[:, :3]).any())
    with_nan = match(qbank, Exemplars(ebank), k=k)
    keep = torch.cat([torch.arange(at), torch.arange(at + 1, m)]).to(dev())
    without = match(qbank, Exemplars(ebank, rows=keep), k=k)
    assert not bool((with_nan.idx == at).any())
    assert torch.equal(with_nan.rows, without.rows) and torch.equal(bits(with_nan.score), bits(without.score))


@pytest.mark.parametrize("kind", KINDS)
def test_a_zero_row_scores_plus_zero_and_takes_the_first_positions(kind):
    from openscene_amd.match import Exemplars, match
    gen = torch.Generator().manual_seed(37)
    d, k = 64, 8
    xq = sr.unit_rows(70, d, gen).half()
    xq[66] = 0
    ex = Exemplars(make_bank(kind, [sr.unit_rows(300, d, gen).half()]))
    got = match(make_bank(kind, [xq]), ex, k=k)
    assert got.idx[66].tolist() == list(range(k))
    assert bits(got.score[66]).tolist() == [0] * k                              # +0, never -0


# ------------------------------------------------------------------------------------------------------------ guards
@pytest.mark.parametrize("kind", KINDS)
def test_a_row_outside_the_bank_raises_and_leaves_the_bank_usable(kind):
    from openscene_amd.match import Exemplars, match, unit_rows
    from openscene_amd.search import search
    gen = torch.Generator().manual_seed(9)
    d = 64
    bank = make_bank(kind, [sr.unit_rows(70, d, gen).half(), sr.unit_rows(30, d, gen).half()])
    text = sr.text(3, d, gen).to(dev())
    before = search(bank, text, k=4, return_heat=True)
    rows = torch.arange(0, 100, 3)
    ex = Exemplars.from_scene(bank, 1)
    good = match(bank, ex, k=4, rows=rows.to(dev()))
    for at, bad_row in ((5, bank.rows), (20, -1)):
        r = rows.clone()
        r[at] = bad_row
        with pytest.raises(RuntimeError, match="osn_bank"):                     # the query side
            match(bank, ex, k=4, rows=r.to(dev()))
        assert int(bank._err_word().item()) == 0
        with pytest.raises(RuntimeError, match="osn_bank"):                     # the exemplar side
            Exemplars(bank, rows=r.to(dev()))
        assert int(bank._err_word().item()) == 0
        with pytest.raises(RuntimeError, match="osn_bank"):
            unit_rows(bank, r.to(dev()), normalize=False)
        assert int(bank._err_word().item()) == 0
    after = search(bank, text, k=4, return_heat=True)
    assert sr.same_bits(after.heat, before.heat) and torch.equal(after.topk_points, before.topk_points)
    assert same(match(bank, ex, k=4, rows=rows.to(dev())), good)


def test_bad_arguments_raise_before_any_launch():
    from openscene_amd import ops
    from openscene_amd.match import Exemplars, match, mutual
    gen = torch.Generator().manual_seed(11)
    bank = make_bank("fp16", [sr.unit_rows(50, 64, gen).half()])
    other = make_bank("fp8", [sr.unit_rows(50, 48, gen).half()])
    ex = Exemplars(bank)
    for k in (0, 9, -1):
        with pytest.raises(ValueError, match="k must be"):
            match(bank, ex, k=k)
        with pytest.raises(ValueError, match="k must be"):
            ops.bank_match(bank.features, ex.image, k=k)
    with pytest.raises(ValueError, match="features"):
        match(other, ex)
    with pytest.raises(ValueError):
        ops.bank_match_fp8(other.codes, other.exponents, ex.image)
    with pytest.raises(TypeError):
        match(bank, ex.image)
    with pytest.raises(TypeError):
        match(bank.features, ex)
    with pytest.raises(TypeError):
        match(bank, ex, rows=torch.arange(5, dtype=torch.int32).to(dev()))
    with pytest.raises(TypeError):
        ops.bank_match(bank.features, ex.image.float())
    with pytest.raises(TypeError):
        ops.bank_match(bank.features.float(), ex.image)
    with pytest.raises(ValueError, match="device"):
        ops.bank_match(bank.features, ex.image.cpu())
    with pytest.raises(ValueError, match="device"):
        match(bank, ex, rows=torch.arange(5))
    with pytest.raises(ValueError, match="splits"):
        ops.bank_match(bank.features, ex.image, splits=65)
    with pytest.raises(TypeError):
        Exemplars(bank, labels=torch.zeros(50))
    with pytest.raises(ValueError):
        Exemplars(bank, labels=torch.zeros(49, dtype=torch.int64))
    with pytest.raises(ValueError, match="k = 1"):
        mutual(match(bank, ex, k=2), match(bank, ex, k=1))
    assert int(bank._err_word().item()) == 0
    empty = match(bank, ex, k=2, rows=torch.zeros(0, dtype=torch.int64).to(dev()))
    assert empty.idx.shape == (0, 2) and empty.score.shape == (0, 2) and empty.count.shape == (0,)


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("kind", KINDS)
def test_labels_novelty_and_correspondences_on_the_planted_scenes(kind):
    from openscene_amd import ops
    from openscene_amd.match import Exemplars, match, mutual, novelty, transfer_labels, unit_rows
    p = gr.planted()
    bank = make_bank(kind, p["feats"])
    ex = Exemplars.from_scene(bank, 0, labels=p["cls"][0])
    assert torch.equal(ex.rows.cpu(), torch.arange(bank.offsets[1]))
    b = mr.operands_f64(ex.image)
    for scene in (1, 2):
        rows = torch.arange(bank.offsets[scene], bank.offsets[scene + 1]).to(dev())
        got = transfer_labels(bank, ex, k=mr.PLANT_K, rows=rows).cpu()
        want, sure = mr.planted_reference(mr.operands_f64(unit_rows(bank, rows)), b, p["cls"][0])
        accuracy = float((got == p["cls"][scene]).double().mean())
        print("%s scene %d: accuracy %.4f, decided rows %.4f" % (kind, scene, accuracy, float(sure.double().mean())))
        assert torch.equal(got[sure], want[sure])
        assert accuracy >= mr.PLANT_ACCURACY
        found = match(bank, ex, k=mr.PLANT_K, rows=rows)
        assert torch.equal(found.vote(), ops.knn_vote(ex.labels, found.idx, found.count))
        assert torch.equal(found.vote().cpu(), mr.vote(p["cls"][0], found.idx, found.count))
        assert torch.equal(found.rows, found.idx.long())                        # scene 0 starts the bank
        floor = float(found.score[:, 0].median())                               # a floor that cuts: the rows below it are filled
        cut = transfer_labels(bank, ex, k=mr.PLANT_K, rows=rows, min_score=floor, fill=-7).cpu()
        low = (found.score[:, 0] < floor).cpu()
        assert bool((cut[low] == -7).all()) and torch.equal(cut[~low], got[~low])
    # novelty of the exemplars' own scene: the best score is at least the row's score with itself, sum u^2, which the operand
    # rounding keeps within 2^-10 (two roundings of 2^-11) + 2 * 1e-5 / ||v|| (||v|| >= 0.2) + 64 * 2^-24 of 1
    own = novelty(bank, ex, rows=ex.rows)
    assert own.dtype == torch.float32 and own.shape == (bank.offsets[1],)
    own = own.cpu().double()
    s_self, a_self = (b * b).sum(1), (b.abs() * b.abs()).sum(1)
    assert bool((own <= (1 - s_self) + mr.C * a_self + 2.0 ** -23).all())
    assert float(own.max()) <= 2.0 ** -10 + 1e-4 + 64 * 2.0 ** -24 + mr.C
    # correspondences: a scene against a row-permuted copy of itself
    feats = p["feats"][0]
    perm = torch.randperm(feats.shape[0], generator=torch.Generator().manual_seed(3))
    a_bank, b_bank = make_bank(kind, [feats]), make_bank(kind, [feats[perm]])
    pairs = mutual(match(a_bank, Exemplars(b_bank)), match(b_bank, Exemplars(a_bank))).cpu()
    _, inverse, counts = torch.unique(feats.view(torch.int16), dim=0, return_inverse=True, return_counts=True)
    single = counts[inverse] == 1                                               # rows without duplicates
    partner = torch.empty_like(perm)
    partner[perm] = torch.arange(perm.shape[0])                                 # row i of the scene is row partner[i] of the copy
    lookup = torch.full((feats.shape[0],), -1, dtype=torch.int64)
    lookup[pairs[:, 0]] = pairs[:, 1]
    assert bool(single.any()) and torch.equal(lookup[single], partner[single])
