"""Two scans in one frame: the rigid motion between them from feature matches, polished on the voxel index.

`match.mutual` answers "which point of the other scan is this one" with index pairs; `neighbors.transfer`, `PointIndex.knn`,
`fill_missing` and `VoxelGrid` all assume the other scan is already in this scan's frame.  Two captures of one room never
are.  This module connects the two:

    RigidTransform      R, t in float64 on the host; .apply, .matrix, .inverse, .compose, .float32 (what the kernels see)
    estimate_rigid      RANSAC over triplets of correspondences + monotone Kabsch rounds -> RigidFit
    align_scenes        two banks and their positions: match both ways, mutual, estimate_rigid -> Alignment (.overlap)
    refine_icp          point-to-point ICP of a scan onto a PointIndex, from a transform -> RigidFit

A pair (s, d) is an inlier of a transform when its float32 residual r2 = |R s + t - d|^2 -- a stated sequence of separately
rounded operations, include/openscene_amd.h -- is <= tau2 = float32(threshold)^2: counts and masks are exact integers, the
same bits as the numpy restatement of tests/align_reference.py.  A RigidFit's count, inliers and residual2 are always those
of the float32 transform it returns.

Kernels: csrc/align.hip through ops.rigid_from_triplets / rigid_score / rigid_best / rigid_moments; the search of an ICP
round is ops.knn_grid unchanged.  H x P residuals are scored without a temporary.  The 3 x 3 Kabsch step (an SVD of the
float64 moments the kernel sums) runs on the host.  No CPU path for the kernels.
"""
import numpy as np
import torch

from . import ops
from .match import Exemplars, match, mutual
from .neighbors import PointIndex

MAX_HYPOTHESES = 65536


class RigidTransform:
    """x -> R x + t: R float64 [3, 3], t float64 [3] on the host (numpy)."""

    def __init__(self, R=None, t=None):
        R = np.eye(3) if R is None else np.array(R.detach().cpu().numpy() if isinstance(R, torch.Tensor) else R, dtype=np.float64)
        t = np.zeros(3) if t is None else np.array(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)
        if R.shape != (3, 3) or t.shape != (3,):
            raise ValueError("R must be [3, 3] and t [3] (got %s and %s)" % (R.shape, t.shape))
        self.R, self.t = R, t

    @classmethod
    def from_float32(cls, xf12):
        """The transform of 12 values (R row-major, then t), widened exactly."""
        x = np.asarray(xf12, dtype=np.float64).reshape(-1)
        if x.shape[0] != 12:
            raise ValueError("12 values: R row-major, then t (got %d)" % x.shape[0])
        return cls(x[:9].reshape(3, 3), x[9:])

    def float32(self):
        """float32 [12] (numpy): R row-major, then t, each rounded once -- the values the kernels see."""
        return np.concatenate([self.R.reshape(9), self.t]).astype(np.float32)

    def apply(self, xyz):
        """R x + t of every row of xyz [N, 3], in float64: a tensor gives a float64 tensor on its device, else numpy."""
        if isinstance(xyz, torch.Tensor):
            if xyz.dim() != 2 or xyz.shape[1] != 3:
                raise ValueError("xyz must be [N, 3] (got %s)" % (tuple(xyz.shape),))
            R = torch.from_numpy(self.R).to(xyz.device)
            return xyz.double() @ R.T + torch.from_numpy(self.t).to(xyz.device)
        xyz = np.asarray(xyz, dtype=np.float64)
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError("xyz must be [N, 3] (got %s)" % (xyz.shape,))
        return xyz @ self.R.T + self.t

    def matrix(self):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = self.R, self.t
        return m

    def inverse(self):
        return RigidTransform(self.R.T, -(self.R.T @ self.t))

    def compose(self, other):
        """self after other: x -> self(other(x))."""
        if not isinstance(other, RigidTransform):
            raise TypeError("compose takes a RigidTransform")
        return RigidTransform(self.R @ other.R, self.R @ other.t + self.t)


class RigidFit:
    """What a fit returns.  transform: the float32 transform, widened (its .float32() is what was scored); count int; inliers
    bool [P] and residual2 float32 [P] on the device, of that transform; hypothesis: the winning triplet's number (-1: none)
    and counts int32 [H]: every hypothesis' inliers, -1 for an invalid one (both None from refine_icp); ok: at least 3 inliers
    (and, from estimate_rigid, a valid hypothesis).  refine_icp adds neighbors int32 [P] and iterations."""

    def __init__(self, transform, count, inliers, residual2, hypothesis=None, counts=None, ok=False, neighbors=None, iterations=None):
        self.transform, self.count, self.inliers, self.residual2 = transform, int(count), inliers, residual2
        self.hypothesis, self.counts, self.ok = hypothesis, counts, bool(ok)
        self.neighbors, self.iterations = neighbors, iterations


def kabsch(moments):
    """moments float64 [16] (n, sum s, sum d, sum s d^T over n >= 3 pairs) -> float32 [12]: the least-squares rigid motion.
    H = sum s d^T - sum s sum d^T / n = U S V^T;  R = V diag(1, 1, det(V U^T)) U^T (a rotation, never a reflection);
    t = mean d - R mean s.  float64, rounded once."""
    m = np.asarray(moments, dtype=np.float64)
    n = m[0]
    ss, sd, sdt = m[1:4], m[4:7], m[7:16].reshape(3, 3)
    hm = sdt - np.outer(ss, sd) / n
    u, _s, vt = np.linalg.svd(hm)
    v = vt.T
    sign = 1.0 if np.linalg.det(v @ u.T) >= 0 else -1.0
    r = v @ np.diag([1.0, 1.0, sign]) @ u.T
    t = sd / n - r @ (ss / n)
    return np.concatenate([r.reshape(9), t]).astype(np.float32)


def draw_triplets(n_pairs, hypotheses, seed=0):
    """int32 [hypotheses, 3] on the host: three pair numbers each, uniform from a torch.Generator seeded with `seed` (a
    triplet that repeats a number is left in: the kernel marks it invalid)."""
    gen = torch.Generator().manual_seed(int(seed))
    return torch.randint(0, max(int(n_pairs), 1), (int(hypotheses), 3), generator=gen, dtype=torch.int64).to(torch.int32)


def area2_min_of(threshold):
    """A triangle whose |a x b| is below (2 threshold)^2 -- two sides of twice the threshold at right angles -- fixes no
    rotation to within the threshold; |a x b|^2 <= this is invalid."""
    return (2.0 * float(threshold)) ** 4


def _tau2(threshold):
    t = np.float32(threshold)
    return float(t * t)                                       # float32(threshold) * float32(threshold), one float32 rounding


def _positions(xyz, name, dev=None):
    if not isinstance(xyz, torch.Tensor) or not xyz.dtype.is_floating_point:
        raise TypeError("%s must be a float tensor" % name)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("%s must be [P, 3] (got %s)" % (name, tuple(xyz.shape)))
    if dev is not None and xyz.device != dev:
        raise ValueError("%s must be on the device of the other points (%s, got %s)" % (name, dev, xyz.device))
    return xyz.detach().float().contiguous()


def _threshold(threshold):
    threshold = float(threshold)
    if not (0.0 < threshold < float("inf")):
        raise ValueError("threshold must be positive and finite (got %r)" % (threshold,))
    return threshold


def estimate_rigid(src_xyz, dst_xyz, threshold, hypotheses=4096, seed=0, refine=3, triplets=None):
    """The rigid motion that takes src_xyz onto dst_xyz (float [P, 3] on one device: pair p says src_xyz[p] is dst_xyz[p];
    some pairs may be wrong) -> RigidFit.

    `hypotheses` triplets of pairs are drawn on the host (`draw_triplets`, seeded) or passed (int [H, 3]); each gives the
    motion of its triangle (invalid when degenerate or when the two triangles are not congruent to 2 * threshold), every
    motion is scored against every pair, and the best (lowest number among equals) is read back: one synchronisation.  Then
    `refine` rounds: the moments of the inliers, float64 Kabsch on the host, a recount under the rounded result -- kept only
    if its count is not lower, so the count never falls."""
    src = _positions(src_xyz, "src_xyz")
    dev = src.device
    dst = _positions(dst_xyz, "dst_xyz", dev)
    if dst.shape[0] != src.shape[0]:
        raise ValueError("src_xyz and dst_xyz must hold a row per pair (got %s and %s)" % (tuple(src.shape), tuple(dst.shape)))
    threshold = _threshold(threshold)
    refine = int(refine)
    if refine < 0:
        raise ValueError("refine must be >= 0 (got %d)" % refine)
    p = src.shape[0]
    if triplets is None:
        hypotheses = int(hypotheses)
        if not 1 <= hypotheses <= MAX_HYPOTHESES:
            raise ValueError("hypotheses must be in 1 .. %d (got %d)" % (MAX_HYPOTHESES, hypotheses))
        triplets = draw_triplets(p, hypotheses, seed)
    else:
        if not isinstance(triplets, torch.Tensor) or triplets.dtype not in (torch.int32, torch.int64):
            raise TypeError("triplets must be an int32 or int64 tensor")
        if triplets.dim() != 2 or triplets.shape[1] != 3 or not 1 <= triplets.shape[0] <= MAX_HYPOTHESES:
            raise ValueError("triplets must be [H, 3], 1 <= H <= %d (got %s)" % (MAX_HYPOTHESES, tuple(triplets.shape)))
    triplets = triplets.to(device=dev, dtype=torch.int32).contiguous()
    tau2 = _tau2(threshold)
    identity = RigidTransform().float32()
    if p == 0:
        counts = torch.full((triplets.shape[0],), -1, dtype=torch.int32, device=dev)
        return RigidFit(RigidTransform(), 0, torch.zeros(0, dtype=torch.bool, device=dev), torch.zeros(0, dtype=torch.float32, device=dev),
                        hypothesis=-1, counts=counts, ok=False)
    xf, valid = ops.rigid_from_triplets(src, dst, triplets, threshold, area2_min_of(threshold))
    counts = ops.rigid_score(src, dst, xf, tau2, valid)
    best = ops.rigid_best(counts)
    row = xf.index_select(0, best[1:2].long()).reshape(12)
    head = torch.cat([best.double(), row.double()]).cpu().numpy()           # the one synchronisation of the search
    top, hyp = int(head[0]), int(head[1])
    found = top >= 0
    cur = head[2:].astype(np.float32) if found else identity
    inl, r2, mom = ops.rigid_moments(src, dst, cur, tau2)
    m = mom.cpu().numpy()
    for _round in range(refine if found else 0):
        if m[0] < 3:
            break
        new = kabsch(m)
        if np.array_equal(new.view(np.uint32), cur.view(np.uint32)):
            break
        inl2, r22, mom2 = ops.rigid_moments(src, dst, new, tau2)
        m2 = mom2.cpu().numpy()
        if m2[0] < m[0]:
            break
        cur, inl, r2, m = new, inl2, r22, m2
    return RigidFit(RigidTransform.from_float32(cur), int(m[0]), inl, r2, hypothesis=hyp if found else -1, counts=counts,
                    ok=found and m[0] >= 3)


class Alignment:
    """What `align_scenes` returns: fit (RigidFit: A's frame -> B's frame over the matched positions), pairs int64 [P, 2]
    (row of A's list, row of B's list), scores float32 [P] (the feature score of every pair)."""

    def __init__(self, fit, pairs, scores):
        self.fit, self.pairs, self.scores = fit, pairs, scores

    def overlap(self, index_b, xyz_a, radius=None, scene=0):
        """The fraction of A's points (float [N, 3], A's frame) that have a point of B's index within `radius` after the
        alignment: what says whether `novelty` between the scans means anything.  Synchronises."""
        if not isinstance(index_b, PointIndex):
            raise TypeError("index_b must be a PointIndex")
        xyz_a = _positions(xyz_a, "xyz_a", index_b.grid.device)
        if xyz_a.shape[0] == 0:
            return 0.0
        count = index_b.knn(self.fit.transform.apply(xyz_a), 1, radius=radius, scene=scene).count
        return float((count > 0).double().mean().item())


def align_scenes(bank_a, xyz_a, bank_b, xyz_b, threshold, rows_a=None, rows_b=None, min_score=None, **fit_args):
    """Align scan A to scan B from their features.  bank_a / bank_b: FeatureBanks (fp16 or fp8, of one dim, on one device);
    rows_a / rows_b: the bank rows of the two scans (int64, None: every row); xyz_a / xyz_b float [len(rows), 3]: their
    positions, each scan in its own frame.  The rows are matched both ways with k = 1 (`match.match`), the mutual best
    (`match.mutual`) with a score of at least `min_score` are the pairs, and `estimate_rigid(..., threshold, **fit_args)`
    fits them -> Alignment."""
    ex_a, ex_b = Exemplars(bank_a, rows_a), Exemplars(bank_b, rows_b)
    dev = ex_a.device
    xyz_a, xyz_b = _positions(xyz_a, "xyz_a", dev), _positions(xyz_b, "xyz_b", dev)
    if xyz_a.shape[0] != len(ex_a) or xyz_b.shape[0] != len(ex_b):
        raise ValueError("a position per row: %d rows of A with %s, %d rows of B with %s"
                         % (len(ex_a), tuple(xyz_a.shape), len(ex_b), tuple(xyz_b.shape)))
    m_ab = match(bank_a, ex_b, k=1, rows=rows_a)
    m_ba = match(bank_b, ex_a, k=1, rows=rows_b)
    pairs = mutual(m_ab, m_ba)
    scores = m_ab.score[pairs[:, 0], 0]
    if min_score is not None:
        keep = scores >= float(min_score)                     # (a NaN score fails)
        pairs, scores = pairs[keep], scores[keep]
    fit = estimate_rigid(xyz_a[pairs[:, 0]], xyz_b[pairs[:, 1]], threshold, **fit_args)
    return Alignment(fit, pairs, scores)


def refine_icp(index_b, xyz_a, transform, iterations=10, radius=None, scene=0, reach=None):
    """Point-to-point ICP of xyz_a (float [M, 3], A's frame) onto the points of index_b (a PointIndex of scan B), starting
    from `transform` -> RigidFit (.neighbors int32 [M]: the final partner of every point, -1 without one; .iterations: the
    Kabsch steps taken).

    A round: index_b.knn(transform.apply(xyz_a), 1, radius, scene); the moments of the pairs (a, its neighbour) under the
    float32 transform with tau2 = float32(radius)^2, straight from the neighbour list (no gathered copy of B); Kabsch on the
    host.  It stops when the neighbour list repeats, after `iterations` steps, or with fewer than 3 pairs.  radius: at most
    (and by default) the grid's voxel size.

    reach (cells): every round's knn runs its second stage (PointIndex.knn), so a point whose 27 cells are empty is paired
    with a point around the nearest occupied cell within `reach` cells -- the nearest of a stated candidate set, not the exact
    metric nearest neighbour; radius, and with it tau2, is then at most and by default (reach + 1) voxel sizes."""
    if not isinstance(index_b, PointIndex):
        raise TypeError("index_b must be a PointIndex")
    if not isinstance(transform, RigidTransform):
        raise TypeError("transform must be a RigidTransform")
    grid = index_b.grid
    src = _positions(xyz_a, "xyz_a", grid.device)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("iterations must be >= 0 (got %d)" % iterations)
    if reach is None:
        tau2 = _tau2(grid.voxel_size if radius is None else radius)
        search = dict(radius=radius, scene=scene)
    else:
        tau2 = _tau2((ops.reach_value(reach) + 1) * grid.voxel_size if radius is None else radius)
        search = dict(radius=radius, scene=scene, reach=reach)
    cur = transform.float32()
    prev = None
    for it in range(iterations + 1):
        idx = index_b.knn(RigidTransform.from_float32(cur).apply(src), 1, **search).idx[:, 0].contiguous()
        inl, r2, mom = ops.rigid_moments(src, grid.xyz, cur, tau2, dst_idx=idx)
        m = mom.cpu().numpy()
        if it == iterations or m[0] < 3 or (prev is not None and torch.equal(idx, prev)):
            break
        prev = idx
        cur = kabsch(m)
    return RigidFit(RigidTransform.from_float32(cur), int(m[0]), inl, r2, ok=m[0] >= 3, neighbors=idx, iterations=it)
