"""The fp8 bank on the device (csrc/search.hip: osn_bank_append_fp8, osn_bank_search_fp8).

Quantiser: codes and exponents bit for bit against the torch restatement of the format (tests/search_fp8_reference.py,
torch's own CPU float8_e4m3fn cast).
Heat-map: against the float64 evaluation of the score formulas on the stored values v = code * 2^e, abs <= 2e-3 -- the
bound of tests/test_gpu_search.py; its derivation carries over because e4m3 -> fp16 is exact, so the MFMA
sees the very values the formula is evaluated on, and 2^e is a power of two.  That 2e-3 is the distance to the REFERENCE's
expression, which rounds the normalised vector to fp16 first, on unit_rows whose exponents are nearly all equal; the kernel's own
arithmetic -- every exponent byte, a different one in the neighbouring row -- is held in tests/test_gpu_search_bounds.py.
Distance to the source rows (normalize = 0): |v_i - x_i| <= 2^-4 |x_i| for a normal code (half a unit of a 3-bit
mantissa), <= 2^-10 * 2^e for a subnormal one (half the code spacing 2^-9); Cauchy-Schwarz over the row gives
|score(v) - score(x)| <= 2^-4 |x| |t| + 2^-10 2^e sqrt(d) |t|, plus the 2e-3 above.
Selection: exact against tests/search_reference.select applied to the kernel's own heat-map."""
import pytest
import torch

import search_fp8_reference as f8
import search_reference as sr
from search_reference import check_selection, text, unit_rows

pytestmark = pytest.mark.gpu

TOL = 2e-3
WIDE = 2064                                                   # 129 groups of 16: past the 2048 columns a wave keeps in registers


def dev():
    return torch.device("cuda", 0)


def fp8_bank(scenes, d, capacity_rows=64):
    from openscene_amd.search import FeatureBank
    bank = FeatureBank(d, dev(), capacity_rows=capacity_rows, dtype="fp8")
    for i, f in enumerate(scenes):
        bank.add_scene("scene%04d" % i, f.to(dev()))
    return bank


# -------------------------------------------------------------------------------------------------------- quantiser
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("d", [16, 144, 768, WIDE])
def test_quantiser_equals_the_torch_restatement_bit_for_bit(d, dtype):
    from openscene_amd.search import FeatureBank
    g = torch.Generator().manual_seed(d)
    for n in (1, 63, 130):
        x = (torch.randn(n, d, generator=g) * torch.exp(3 * torch.randn(n, 1, generator=g))).to(dtype)
        inv = torch.randint(0, n, (2 * n + 1,), generator=g)             # repeats indices
        bank = FeatureBank(d, dev(), capacity_rows=8, dtype="fp8")
        bank.add_scene("plain", x.to(dev()))
        bank.add_scene("gathered", x.to(dev()), inv.to(dev()))
        assert bank.offsets == [0, n, 3 * n + 1]
        codes, exps = f8.quantize(torch.cat([x, x[inv]]))
        assert f8.same_codes(bank.codes, bank.exponents, codes, exps), (n, d, dtype)


def hand_placed_rows():
    d = 32
    g = torch.Generator().manual_seed(3)
    rows, name = [], []

    def add(what, r):
        rows.append(r.reshape(1, d).float())
        name.append(what)
    small = 0.01 * torch.randn(d, generator=g)
    add("zero", torch.zeros(d))
    r = torch.randn(d, generator=g); r[4] = -0.0
    add("minus zero", r)
    r = torch.zeros(d); r[7] = -0.0
    add("only a minus zero", r)
    add("tiny", torch.randn(d, generator=g) * 1e-30)
    add("huge", torch.randn(d, generator=g) * 1e30)
    add("below 448 * 2^-120", torch.randn(d, generator=g) * 1e-37)
    add("float32 subnormals", torch.randn(d, generator=g) * 1e-41)
    add("fp16 subnormals", torch.randint(-1023, 1024, (d,), generator=g).float() * 2.0 ** -24)
    for j in (-130, -20, -3, 0, 5, 100):
        edge = torch.tensor(448.0 * 2.0 ** j)
        for what, top in (("amax = 448 * 2^%d" % j, edge), ("the float above 448 * 2^%d" % j, torch.nextafter(edge, torch.tensor(float("inf"))))):
            r = small * 2.0 ** j; r[9] = -top
            add(what, r)
    r = small.clone(); r[9] = 448.25                          # the fp16 number above 448
    add("448.25", r)
    r = torch.zeros(d); r[0] = 448.0
    r[1:9] = torch.tensor([17.0, 19.0, -17.0, -19.0, 18.0, 21.0, 23.0, 416.0 + 16.0])      # ties: to the even mantissa
    r[9:20] = torch.tensor([2.0 ** -6, 2.0 ** -7, 3 * 2.0 ** -9, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9,
                            -(2.0 ** -10), 2.0 ** -11, 7.5 * 2.0 ** -9, 1.0001 * 2.0 ** -10])    # the codes' subnormal range
    add("ties and code subnormals", r)
    r = torch.randn(d, generator=g); r[30] = float("inf")
    add("inf", r)
    r = torch.randn(d, generator=g); r[0] = float("nan")
    add("nan", r)
    return torch.cat(rows), name


def test_quantiser_hand_placed_rows():
    x, name = hand_placed_rows()
    i = name.index
    for dtype in (torch.float32, torch.float16):
        xs = x.to(dtype)                                      # (fp16: tiny rows become zero or subnormal, huge ones inf -- all cases of the format)
        bank = fp8_bank([xs], x.shape[1])
        codes, exps = f8.quantize(xs)
        got_c, got_e = bank.codes.cpu(), bank.exponents.cpu()
        for r, what in enumerate(name):
            assert f8.same_codes(got_c[r:r + 1], got_e[r:r + 1], codes[r:r + 1], exps[r:r + 1]), (what, dtype)
        # the restatement itself says what the issue says
        assert got_e[i("zero")] == 0 and (got_c[i("zero")] == 0).all()
        assert got_c[i("minus zero"), 4] == 0x80 and got_c[i("only a minus zero"), 7] == 0x80 and got_e[i("only a minus zero")] == 0
        assert got_e[i("amax = 448 * 2^0")] == 0 and got_e[i("448.25")] == 1
        assert got_c[i("amax = 448 * 2^0"), 9] == 0xFE
        t = i("ties and code subnormals")
        assert got_e[t] == 0 and got_c[t, :5].tolist() == [0x7E, 0x58, 0x5A, 0xD8, 0xDA]        # 448, 17 -> 16, 19 -> 20
        assert got_c[t, 9:14].tolist() == [0x08, 0x04, 0x03, 0x01, 0x00]
        for bad in ("inf", "nan"):
            assert got_e[i(bad)] == 0 and ((got_c[i(bad)] & 0x7F) == 0x7F).all()
    assert bank.exponents.cpu()[i("huge")] == 0               # fp16: 1e30 is inf
    b32 = fp8_bank([x], x.shape[1])
    e32 = b32.exponents.cpu()
    assert e32[i("below 448 * 2^-120")] == -120 and e32[i("float32 subnormals")] == -120 and e32[i("amax = 448 * 2^-130")] == -120
    assert e32[i("the float above 448 * 2^0")] == 1 and e32[i("the float above 448 * 2^-20")] == -19 and e32[i("amax = 448 * 2^-20")] == -20
    assert e32[i("amax = 448 * 2^100")] == 100 and e32[i("the float above 448 * 2^100")] == 101


def test_bad_gather_index_raises_and_leaves_the_bank_as_it_was():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(300, 144, generator=g).to(dev())
    bank = fp8_bank([x], 144, capacity_rows=2000)
    codes, exps = bank._codes.clone(), bank._exps.clone()     # scratch rows included: a bad row writes nothing
    inv = torch.randint(0, 300, (700,), generator=g).to(dev())
    for dtype in (torch.float32, torch.float16):
        for bad in (-1, 300):
            inv_bad = inv.clone()
            inv_bad[311] = bad
            with pytest.raises(Exception, match="gather index"):
                bank.add_scene("bad", x.to(dtype), inv_bad)
            assert bank.rows == 300 and bank.offsets == [0, 300] and bank.names == ["scene0000"]
            assert torch.equal(bank.codes, codes[:300]) and torch.equal(bank.exponents, exps[:300])
            assert torch.equal(bank._codes[300 + 311], codes[300 + 311]) and bank._exps[300 + 311] == exps[300 + 311]
    bank.add_scene("after", x, inv)                           # the error word was cleared
    c, e = f8.quantize(x[inv])
    assert f8.same_codes(bank.codes[300:], bank.exponents[300:], c, e)


# --------------------------------------------------------------------------------------------------------- heat-map
@pytest.mark.parametrize("d", [16, 144, 768])
@pytest.mark.parametrize("normalize", [True, False])
def test_heat_map_matches_the_float64_formulas_on_the_stored_values(normalize, d):
    from openscene_amd.search import search
    g = torch.Generator().manual_seed(10 * d + int(normalize))
    worst = 0.0
    for n in (1, 127, 128, 129, 300):
        x = unit_rows(n, d, g)
        zero = [r for r in (2, 126, 128, 299) if r < n]
        nan = [r for r in (5, 200) if r < n]
        if zero:
            x[zero] = 0
        for r in nan:
            x[r, r % d] = float("nan")
        ok = torch.ones(n, dtype=torch.bool)
        ok[nan] = False
        bank = fp8_bank([x], d)
        codes, exps = bank.codes.cpu(), bank.exponents.cpu()
        for q in (1, 33, 65):
            t = text(q, d, g)
            heat = search(bank, t.to(dev()), k=4, normalize=normalize, return_heat=True).heat.cpu()
            assert heat.shape == (n, q) and heat.dtype == torch.float16
            assert torch.isnan(heat[nan]).all() and not torch.isnan(heat[ok]).any()
            assert (heat[zero] == 0).all()
            ref = f8.scores_f64(codes, exps, t, normalize)
            dev_ = (heat.double() - ref)[ok].abs().max().item() if ok.any() else 0.0
            print("fp8 heat-map normalize=%d n=%d d=%d q=%d: max abs deviation %.3e" % (normalize, n, d, q, dev_))
            worst = max(worst, dev_)
    assert worst <= TOL


@pytest.mark.parametrize("d", [16, 144, 768])
def test_raw_scores_stay_within_the_derived_distance_of_the_source_rows(d):
    from openscene_amd.search import search
    g = torch.Generator().manual_seed(77 + d)
    n, q = 300, 33
    x = unit_rows(n, d, g)
    x[:40] *= torch.exp(2 * torch.randn(40, 1, generator=g)).clamp(0.05, 1.0)      # smaller rows: other exponents
    t = text(q, d, g)
    bank = fp8_bank([x], d)
    heat = search(bank, t.to(dev()), k=4, normalize=False, return_heat=True).heat.cpu()
    ref = x.double() @ t.double().t()
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), bank.exponents.cpu().double())
    tn = t.double().norm(dim=1)
    bound = (2.0 ** -4 * x.double().norm(dim=1)[:, None] + 2.0 ** -10 * scale[:, None] * d ** 0.5) * tn[None, :] + TOL
    diff = (heat.double() - ref).abs()
    print("fp8 raw scores vs the float32 rows, d=%d: max |diff| %.3e, max diff / bound %.3f" % (d, diff.max().item(), (diff / bound).max().item()))
    assert (diff <= bound).all()


# -------------------------------------------------------------------------------------------------------- selection
def test_selection_is_exact_with_ties_an_empty_scene_and_k_past_a_scene():
    from openscene_amd.search import search
    d, k = 144, 64
    g = torch.Generator().manual_seed(21)
    a = unit_rows(700, d, g)
    a[60:660] = 0                                             # 600 zero rows, about 50 positive scores: the k-th score is a 0 among hundreds
    a[680] = float("nan")
    scenes = [a, torch.zeros(0, d), unit_rows(40, d, g)]      # the last one is shorter than k
    t = text(5, d, g).to(dev())
    bank = fp8_bank(scenes, d)
    heat = search(bank, t, k=k, return_heat=True).heat
    thr = torch.tensor([0.0, heat[3, 1].item(), 0.05, heat[720, 3].item(), -0.02])
    for normalize in (True, False):
        res = search(bank, t, k=k, thresholds=thr, normalize=normalize, return_heat=True)
        check_selection(res, res.heat, bank.offsets, k, thr.to(dev()))
        again = search(bank, t, k=k, thresholds=thr, normalize=normalize, return_heat=True)
        assert sr.same_bits(again.heat, res.heat) and sr.same_bits(again.topk_scores, res.topk_scores)
        assert torch.equal(again.topk_points, res.topk_points) and torch.equal(again.counts, res.counts)
        no_heat = search(bank, t, k=k, thresholds=thr, normalize=normalize)
        assert no_heat.heat is None and torch.equal(no_heat.topk_points, res.topk_points)
        # the hard cases really are in the data
        zeros = res.topk_scores[0, 0].float() == 0
        assert zeros.any() and (res.topk_scores[0, 0].float() >= 0).all()
        pts = res.topk_points[0, 0][zeros]
        assert pts.tolist() == list(range(60, 60 + pts.numel()))             # ties: the lowest indices
        assert res.counts[0, 0].item() >= 600
        assert (res.topk_points[1] == -1).all() and res.counts[1].tolist() == [0] * 5
        assert (res.topk_points[2, :, 40:] == -1).all() and (res.topk_points[2, :, :40] >= 0).all()
        for i, s in enumerate(scenes):                        # a scene alone scores and selects as beside its neighbours
            one = search(fp8_bank([s], d), t, k=k, thresholds=thr, normalize=normalize, return_heat=True)
            assert sr.same_bits(one.heat, res.scene_heat(i))
            assert sr.same_bits(one.topk_scores[0], res.topk_scores[i]) and torch.equal(one.topk_points[0], res.topk_points[i])
            assert torch.equal(one.counts[0], res.counts[i])


# ------------------------------------------------------------------------------------------------------------- bank
def test_bank_conversion_files_dequantize_and_size(tmp_path):
    from openscene_amd.search import FeatureBank, search
    d = 144
    g = torch.Generator().manual_seed(31)
    scenes = [unit_rows(70, d, g).half(), torch.zeros(0, d, dtype=torch.float16), (unit_rows(200, d, g) * 40).half()]
    half = FeatureBank(d, dev(), capacity_rows=16)
    for i, s in enumerate(scenes):
        half.add_scene("s%d" % i, s.to(dev()))
    bank = half.to_fp8()
    assert bank.dtype == "fp8" and bank.offsets == half.offsets and bank.names == half.names
    codes, exps = f8.quantize(half.features)
    assert f8.same_codes(bank.codes, bank.exponents, codes, exps)
    assert bank.nbytes == bank.rows * (d + 1) and half.nbytes == half.rows * d * 2
    v = f8.dequantize(codes, exps)
    assert torch.equal(bank.dequantize().cpu().double(), v) and bank.dequantize().dtype == torch.float32
    assert torch.equal(bank.dequantize("s2").cpu().double(), v[70:]) and bank.dequantize(1).shape == (0, d)
    with pytest.raises(TypeError, match="dequantize"):
        bank.features
    with pytest.raises(TypeError, match="dequantize"):
        bank.scene(0)
    path = str(tmp_path / "bank8.pt")
    bank.save(path)
    back = FeatureBank.load(path, dev())
    assert back.dtype == "fp8" and back.offsets == bank.offsets and back.names == bank.names
    assert torch.equal(back.codes, bank.codes) and torch.equal(back.exponents, bank.exponents)
    t = text(3, d, g).to(dev())
    assert sr.same_bits(search(back, t, return_heat=True).heat, search(bank, t, return_heat=True).heat)
    # a file in the layout the fp16 bank has always written (no "dtype" entry) still loads
    old = str(tmp_path / "bank16.pt")
    torch.save({"dim": d, "offsets": list(half.offsets), "names": list(half.names), "features": half.features.cpu().clone()}, old)
    back16 = FeatureBank.load(old, dev())
    assert back16.dtype == "fp16" and sr.same_bits(back16.features, half.features) and back16.offsets == half.offsets
    path16 = str(tmp_path / "bank16b.pt")
    half.save(path16)
    assert sr.same_bits(FeatureBank.load(path16, dev()).features, half.features)


# ---------------------------------------------------------------------------------------------------------- objects
def test_objects_of_an_fp8_search():
    from openscene_amd.objects import VoxelGrid, find_objects
    from openscene_amd.search import search
    d = 48
    g = torch.Generator().manual_seed(41)
    t = text(2, d, g)
    n = 400
    xyz = torch.rand(n, 3, generator=g)
    x = unit_rows(n, d, g)
    blob = (xyz - torch.tensor([0.3, 0.3, 0.3])).norm(dim=1) < 0.2
    x[blob] = t[0].float() + 0.02 * torch.randn(int(blob.sum()), d, generator=g)
    bank = fp8_bank([x[:250], x[250:]], d)
    grid = VoxelGrid(xyz.to(dev()), bank.offsets, voxel_size=0.1)
    res = search(bank, t.to(dev()), k=8, return_heat=True)
    thr = [0.6, 0.3]
    got = res.find_objects(grid, thr, return_point_ids=True)
    ref = find_objects(grid, res.heat, thr, return_point_ids=True)
    assert got.names == bank.names and got.n_objects[:, 0].sum().item() >= 1
    assert torch.equal(got.n_objects, ref.n_objects) and torch.equal(got.point_object, ref.point_object)
    for f in ("n_points", "n_voxels", "peak_point", "score_sum", "vox_sum", "box_min", "box_max"):
        assert torch.equal(getattr(got, f), getattr(ref, f)), f
    assert sr.same_bits(got.peak_score, ref.peak_score)
