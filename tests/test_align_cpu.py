"""The alignment contract on the CPU.  First the numpy restatement (tests/align_reference.py) against hand-made cases and the
planted problems the GPU test uses -- with the preconditions that test relies on -- then the host logic of
openscene_amd.align with the four ops entry points replaced by the restatement: argument errors, P = 0, all hypotheses
invalid, the monotone refine rule, the ICP loop and its stopping rule."""
import math
import types

import numpy as np
import pytest
import torch

import align_reference as ar

SEEDS = range(5)


# --------------------------------------------------------------------------------------------------------- the restatement
def test_the_boundary_pair_is_an_inlier_and_the_next_float_is_not():
    tau = np.float32(0.01)
    tau2 = ar.tau2_of(0.01)
    src = np.zeros((3, 3), dtype=np.float32)
    dst = np.array([[tau, 0, 0], [np.nextafter(tau, np.float32(1)), 0, 0], [np.nan, 0, 0]], dtype=np.float32)
    r2 = ar.residual2(ar.IDENTITY12, src, dst)
    assert r2[0] == tau2 and r2[1] > tau2 and np.isnan(r2[2])
    assert ar.score(src, dst, ar.IDENTITY12[None], tau2).tolist() == [1]
    assert ar.score(src, dst, ar.IDENTITY12[None], tau2, valid=np.array([False])).tolist() == [-1]


def test_the_residual_rounds_every_operation():
    """a case where the fused and the separately rounded forms differ: x = 1 + 2^-12, x * x + (-1) in float32"""
    x = np.float32(1 + 2.0 ** -12)
    xf = np.array([x, 0, 0, 0, 1, 0, 0, 0, 1, -1, 0, 0], dtype=np.float32)
    src = np.array([[x, 0, 0]], dtype=np.float32)
    dst = np.zeros((1, 3), dtype=np.float32)
    e0 = np.float32(x * x) + np.float32(-1)                    # the product rounded first: 2^-11, not 2^-11 + 2^-24
    assert e0 == np.float32(2.0 ** -11) and float(x) * float(x) - 1 != float(e0)
    assert ar.residual2(xf, src, dst)[0] == e0 * e0


def test_best_takes_the_lowest_hypothesis_among_equals():
    assert ar.best(np.array([-1, 3, 7, 7, 2], dtype=np.int32)) == (7, 2)
    assert ar.best(np.array([-1, -1], dtype=np.int32)) == (-1, 0)


def hand_triangles():
    src = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0, 0, 2], [0.5, 0.25, 1]], dtype=np.float32)
    rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float64)           # a quarter turn about z
    dst = (src.astype(np.float64) @ rz.T + np.array([1, 2, 3])).astype(np.float32)
    dst[5] = [9, 9, 9]                                                           # an outlier pair
    trip = np.array([[0, 1, 2], [2, 4, 1], [0, 0, 1], [0, 1, 3], [0, 1, 5], [0, 1, 6], [-1, 1, 2]], dtype=np.int32)
    return src, dst, trip, rz


def test_triplets_by_hand_a_quarter_turn_and_the_four_degenerate_kinds():
    src, dst, trip, rz = hand_triangles()
    xf, valid = ar.from_triplets(src, dst, trip, 0.01, ar.area2_min_of(0.01))
    assert valid.tolist() == [True, True, False, False, False, False, False]    # repeated, collinear, not congruent, out of range x 2
    want = np.concatenate([rz.reshape(9), [1, 2, 3]]).astype(np.float32)
    assert np.array_equal(xf[0], want) and np.allclose(xf[1], want, atol=1e-6)
    assert all(np.array_equal(xf[i], ar.IDENTITY12) for i in range(2, 7))
    assert ar.score(src, dst, xf, ar.tau2_of(0.01), valid).tolist() == [5, 5, -1, -1, -1, -1, -1]


def test_moments_are_the_correctly_rounded_sums_over_the_inliers_and_no_partner_is_infinitely_far():
    src, dst, inl = ar.planted_case(0)
    xf = np.concatenate([ar.PLANTED_R.reshape(9), ar.PLANTED_T]).astype(np.float32)
    got_inl, r2, m, mabs = ar.moments(src, dst, xf, ar.tau2_of(0.01))
    assert np.array_equal(got_inl, inl) and m[0] == inl.sum() == 240
    s, d = src[inl].astype(np.float64), dst[inl].astype(np.float64)
    assert np.allclose(m[1:4], s.sum(0)) and np.allclose(m[4:7], d.sum(0)) and np.allclose(m[7:].reshape(3, 3), s.T @ d)
    assert (mabs >= np.abs(m)).all()
    idx = np.arange(400, dtype=np.int32)
    idx[[3, 5]] = [-1, 400]
    inl2, r22, m2, _ = ar.moments(src, dst, xf, ar.tau2_of(0.01), dst_idx=idx)
    assert np.isinf(r22[[3, 5]]).all() and not inl2[[3, 5]].any()
    keep = np.ones(400, dtype=bool)
    keep[[3, 5]] = False
    assert np.array_equal(inl2[keep], inl[keep]) and np.array_equal(r22[keep].view(np.uint32), r2[keep].view(np.uint32))


def test_kabsch_returns_the_planted_rotation_and_never_a_reflection():
    rng = np.random.default_rng(3)
    s = rng.random((50, 3)).astype(np.float32)
    d = (s.astype(np.float64) @ ar.PLANTED_R.T + ar.PLANTED_T).astype(np.float32)
    m = np.array([math_sum(t) for t in ar.moment_terms(s, d, np.ones(50, dtype=bool))])
    xf = ar.kabsch(m).astype(np.float64)
    assert np.abs(xf[:9].reshape(3, 3) - ar.PLANTED_R).max() < 1e-6 and np.abs(xf[9:] - ar.PLANTED_T).max() < 1e-6
    flat = s.copy()
    flat[:, 2] = 0                                            # a planar set mirrored: the best rotation, not the mirror
    mirrored = flat * np.array([1, 1, -1], dtype=np.float32) * np.array([-1, 1, 1], dtype=np.float32)
    m = np.array([math_sum(t) for t in ar.moment_terms(flat, mirrored, np.ones(50, dtype=bool))])
    r = ar.kabsch(m)[:9].reshape(3, 3).astype(np.float64)
    assert abs(np.linalg.det(r) - 1) < 1e-6


def math_sum(t):
    return math.fsum(t.tolist())


@pytest.mark.parametrize("seed", SEEDS)
def test_the_planted_problem_meets_the_preconditions_of_the_device_test(seed):
    src, dst, inl = ar.planted_case(seed)
    assert src.shape == (400, 3) and inl.sum() == 240
    trip = draw(400, 512, seed)
    tau2 = ar.tau2_of(ar.PLANTED_THRESHOLD)
    xf, valid = ar.from_triplets(src, dst, trip, ar.PLANTED_THRESHOLD, ar.area2_min_of(ar.PLANTED_THRESHOLD))
    clean = inl[trip].all(1)
    assert (valid & clean).any()                              # at least one all-inlier triplet is valid
    print("seed %d: %d valid hypotheses of 512, %d of them clean" % (seed, valid.sum(), (valid & clean).sum()))
    fit = ar.estimate_rigid(src, dst, ar.PLANTED_THRESHOLD, trip)
    r2 = fit["residual2"]
    assert not ((r2 >= tau2 / 2) & (r2 <= 2 * tau2)).any()    # no pair near the threshold: one ulp of the transform moves no count
    assert fit["ok"] and np.array_equal(fit["inliers"], inl) and fit["count"] == 240
    assert fit["counts"][fit["hypothesis"]] == fit["counts"].max() <= fit["count"]
    truth = np.concatenate([ar.PLANTED_R.reshape(9), ar.PLANTED_T])
    assert np.abs(ar.apply12(fit["xf12"], ar.corners()) - ar.apply12(truth, ar.corners())).max() < 1e-3      # 2 mm of noise over 240 pairs


def draw(p, h, seed):
    from openscene_amd.align import draw_triplets
    return draw_triplets(p, h, seed).numpy()


def room(n=3000):
    from openscene_amd.synthetic import room_points
    return room_points(0, n_pts=n)


def test_the_icp_case_reaches_the_twin_pairing_and_exercises_the_loop():
    b, a, twin = ar.icp_case(room())
    first = ar.nearest(b, a, ar.tau2_of(ar.ICP_VOXEL))
    assert 0.5 < (first == twin).mean() < 0.97                # the identity pairs most, not all, points with their twins
    fit = ar.refine_icp(b, a, ar.IDENTITY12, ar.ICP_VOXEL, iterations=10)
    assert np.array_equal(fit["neighbors"], twin) and fit["count"] == 1500 and 2 <= fit["iterations"] < 10
    gap = np.abs(ar.apply12(fit["xf12"], a) - b[twin].astype(np.float64))
    print("icp: %d iterations, worst gap / bound %.3f" % (fit["iterations"], (gap / ar.twin_bound(fit["xf12"], a)).max()))
    assert (gap <= ar.twin_bound(fit["xf12"], a)).all()


# ------------------------------------------------------------------------------------- the host logic over the restatement
@pytest.fixture()
def ref_ops(monkeypatch):
    """openscene_amd.ops' four rigid entry points computed by the restatement on CPU tensors; -> the list of calls made"""
    from openscene_amd import ops
    calls = []

    def np_(t):
        return t.numpy()

    def from_triplets(src, dst, triplets, threshold, area2_min=0.0):
        calls.append("from_triplets")
        xf, valid = ar.from_triplets(np_(src), np_(dst), np_(triplets), threshold, area2_min)
        return torch.from_numpy(xf), torch.from_numpy(valid)

    def score(src, dst, xf, tau2, valid=None):
        calls.append("score")
        return torch.from_numpy(ar.score(np_(src), np_(dst), np_(xf), tau2, None if valid is None else np_(valid)))

    def best(counts):
        calls.append("best")
        return torch.tensor(ar.best(np_(counts)), dtype=torch.int32)

    def moments(src, dst, xf12, tau2, dst_idx=None):
        calls.append("moments")
        inl, r2, m, _ = ar.moments(np_(src), np_(dst), np.asarray(xf12, dtype=np.float32), tau2, None if dst_idx is None else np_(dst_idx))
        return torch.from_numpy(inl), torch.from_numpy(r2), torch.from_numpy(m)

    monkeypatch.setattr(ops, "rigid_from_triplets", from_triplets)
    monkeypatch.setattr(ops, "rigid_score", score)
    monkeypatch.setattr(ops, "rigid_best", best)
    monkeypatch.setattr(ops, "rigid_moments", moments)
    return calls


def planted_tensors(seed):
    src, dst, inl = ar.planted_case(seed)
    return torch.from_numpy(src), torch.from_numpy(dst), inl


def test_rigid_transform_algebra():
    from openscene_amd.align import RigidTransform
    t = RigidTransform(ar.PLANTED_R, ar.PLANTED_T)
    x = np.random.default_rng(0).random((10, 3))
    assert np.allclose(t.inverse().apply(t.apply(x)), x) and np.allclose(t.compose(t.inverse()).matrix(), np.eye(4))
    assert np.allclose(t.matrix() @ np.append(x[0], 1), np.append(t.apply(x)[0], 1))
    assert np.allclose(t.compose(t).apply(x), t.apply(t.apply(x)))
    f = t.float32()
    assert f.dtype == np.float32 and f.shape == (12,) and np.array_equal(RigidTransform.from_float32(f).float32(), f)
    got = t.apply(torch.from_numpy(x).float())
    assert got.dtype == torch.float64 and np.allclose(got.numpy(), t.apply(x.astype(np.float32)))
    with pytest.raises(ValueError):
        RigidTransform(np.eye(4), np.zeros(3))
    with pytest.raises(ValueError):
        t.apply(np.zeros((3, 2)))
    with pytest.raises(TypeError):
        t.compose(np.eye(4))


@pytest.mark.parametrize("seed", (0, 3))
def test_estimate_rigid_is_the_reference_pipeline_with_one_call_per_stage(ref_ops, seed):
    from openscene_amd.align import estimate_rigid
    src, dst, inl = planted_tensors(seed)
    fit = estimate_rigid(src, dst, ar.PLANTED_THRESHOLD, hypotheses=512, seed=seed)
    ref = ar.estimate_rigid(src.numpy(), dst.numpy(), ar.PLANTED_THRESHOLD, draw(400, 512, seed))
    assert ref_ops[:3] == ["from_triplets", "score", "best"] and set(ref_ops[3:]) == {"moments"} and len(ref_ops) <= 3 + 1 + 3
    assert np.array_equal(fit.transform.float32().view(np.uint32), ref["xf12"].view(np.uint32))
    assert fit.ok and fit.count == ref["count"] == 240 and fit.hypothesis == ref["hypothesis"]
    assert np.array_equal(fit.inliers.numpy(), inl) and np.array_equal(fit.residual2.numpy().view(np.uint32), ref["residual2"].view(np.uint32))
    assert np.array_equal(fit.counts.numpy(), ref["counts"])
    passed = estimate_rigid(src.double(), dst.double(), ar.PLANTED_THRESHOLD, triplets=torch.from_numpy(draw(400, 512, seed)).long())
    assert np.array_equal(passed.transform.float32(), fit.transform.float32())


def test_estimate_rigid_argument_errors(ref_ops):
    from openscene_amd.align import estimate_rigid
    src, dst, _ = planted_tensors(0)
    with pytest.raises(TypeError):
        estimate_rigid(src.numpy(), dst, 0.01)
    with pytest.raises(TypeError):
        estimate_rigid(src.long(), dst, 0.01)
    with pytest.raises(ValueError, match=r"\(400, 2\)"):
        estimate_rigid(src[:, :2], dst, 0.01)
    with pytest.raises(ValueError, match=r"\(399, 3\)"):
        estimate_rigid(src, dst[:399], 0.01)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="threshold"):
            estimate_rigid(src, dst, bad)
    for bad in (0, 65537):
        with pytest.raises(ValueError, match="hypotheses"):
            estimate_rigid(src, dst, 0.01, hypotheses=bad)
    with pytest.raises(ValueError, match="refine"):
        estimate_rigid(src, dst, 0.01, refine=-1)
    with pytest.raises(TypeError):
        estimate_rigid(src, dst, 0.01, triplets=torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r"\(4, 2\)"):
        estimate_rigid(src, dst, 0.01, triplets=torch.zeros(4, 2, dtype=torch.int32))
    assert ref_ops == []                                      # every check came before the first kernel


def test_no_pairs_and_no_valid_hypothesis_give_the_identity_and_not_ok(ref_ops):
    from openscene_amd.align import estimate_rigid
    empty = torch.zeros(0, 3)
    fit = estimate_rigid(empty, empty, 0.01, hypotheses=8)
    assert not fit.ok and fit.count == 0 and fit.hypothesis == -1 and fit.inliers.shape == (0,) and fit.residual2.shape == (0,)
    assert fit.counts.tolist() == [-1] * 8 and np.array_equal(fit.transform.float32(), ar.IDENTITY12) and ref_ops == []
    line = torch.arange(12, dtype=torch.float32).reshape(4, 3)                    # collinear points: every triplet is degenerate
    fit = estimate_rigid(line, line + 1, 0.01, hypotheses=16)
    assert not fit.ok and fit.hypothesis == -1 and fit.counts.tolist() == [-1] * 16
    assert np.array_equal(fit.transform.float32(), ar.IDENTITY12) and fit.count == 0 and not fit.inliers.any()
    assert ref_ops == ["from_triplets", "score", "best", "moments"]              # the mask and residuals are the identity's
    two = estimate_rigid(line[:2], line[:2], 0.01, hypotheses=4)                  # fewer than three pairs: nothing to draw
    assert not two.ok and two.counts.tolist() == [-1] * 4 and two.count == 2      # (the identity does fit them)


def test_a_refine_round_that_loses_inliers_is_not_kept(ref_ops, monkeypatch):
    from openscene_amd import align
    src, dst, inl = planted_tensors(1)
    raw = align.estimate_rigid(src, dst, ar.PLANTED_THRESHOLD, hypotheses=512, seed=1, refine=0)
    assert ref_ops.count("moments") == 1 and raw.count == raw.counts.max().item()
    shifted = raw.transform.float32().copy()
    shifted[9] += np.float32(0.008)                           # 8 mm off: some inliers leave
    real = align.kabsch
    monkeypatch.setattr(align, "kabsch", lambda m: shifted)
    kept = align.estimate_rigid(src, dst, ar.PLANTED_THRESHOLD, hypotheses=512, seed=1, refine=3)
    assert ref_ops.count("moments") == 1 + 2                  # the start, one losing round, and the loop ends
    assert np.array_equal(kept.transform.float32(), raw.transform.float32()) and kept.count == raw.count
    assert np.array_equal(kept.inliers.numpy(), raw.inliers.numpy())
    monkeypatch.setattr(align, "kabsch", real)
    for refine in (1, 2, 3):                                  # the real rounds: the count never falls
        assert align.estimate_rigid(src, dst, ar.PLANTED_THRESHOLD, hypotheses=512, seed=1, refine=refine).count >= raw.count


class FakeIndex:
    """A PointIndex over CPU points whose search is the brute force of the restatement."""

    def __init__(self, points):
        self.grid = types.SimpleNamespace(xyz=torch.from_numpy(points), device=torch.device("cpu"), voxel_size=ar.ICP_VOXEL)
        self.searches = 0

    def knn(self, query_xyz, k, radius=None, scene=0):
        assert k == 1 and query_xyz.dtype == torch.float64
        self.searches += 1
        idx = ar.nearest(self.grid.xyz.numpy(), query_xyz.float().numpy(), ar.tau2_of(self.grid.voxel_size if radius is None else radius))
        return types.SimpleNamespace(idx=torch.from_numpy(idx)[:, None], count=torch.from_numpy((idx >= 0).astype(np.int32)))


def test_refine_icp_loops_until_the_neighbour_list_repeats(ref_ops, monkeypatch):
    from openscene_amd import align
    monkeypatch.setattr(align, "PointIndex", FakeIndex)
    b, a, twin = ar.icp_case(room())
    index = FakeIndex(b)
    fit = align.refine_icp(index, torch.from_numpy(a), align.RigidTransform(), iterations=10, radius=ar.ICP_VOXEL)
    ref = ar.refine_icp(b, a, ar.IDENTITY12, ar.ICP_VOXEL, iterations=10)
    assert np.array_equal(fit.transform.float32().view(np.uint32), ref["xf12"].view(np.uint32))
    assert fit.iterations == ref["iterations"] and index.searches == fit.iterations + 1 == ref_ops.count("moments")
    assert fit.ok and fit.count == 1500 and np.array_equal(fit.neighbors.numpy(), twin) and fit.inliers.all()
    capped = align.refine_icp(FakeIndex(b), torch.from_numpy(a), align.RigidTransform(), iterations=1, radius=ar.ICP_VOXEL)
    assert capped.iterations == 1 and capped.count == int(capped.inliers.sum())   # the count is the returned transform's
    al = align.Alignment(fit, None, None)
    assert al.overlap(FakeIndex(b), torch.from_numpy(a), radius=ar.ICP_VOXEL) == 1.0
    assert align.Alignment(align.RigidFit(align.RigidTransform(t=[0, 0, 5]), 0, None, None), None, None).overlap(
        FakeIndex(b), torch.from_numpy(a), radius=ar.ICP_VOXEL) == 0.0            # (moved out of the room)
    with pytest.raises(TypeError):
        align.refine_icp(b, torch.from_numpy(a), align.RigidTransform())
    with pytest.raises(TypeError):
        align.refine_icp(index, torch.from_numpy(a), np.eye(4))
    with pytest.raises(ValueError, match="iterations"):
        align.refine_icp(index, torch.from_numpy(a), align.RigidTransform(), iterations=-1)
