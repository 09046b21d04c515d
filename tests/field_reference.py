"""numpy restatements of the point <-> voxel operations (helper of test_field_cpu.py and test_gpu_field.py, not a test).

DESIGN.md section 4, operation by operation, in float32 -- bit for bit what the kernels of csrc/field.hip compute -- plus float64
forms the tests hold the float32 results to.  Semantics recalled from MinkowskiEngine v0.5.4, parity unpinned like oracle/.

  quantise   cell = floorf of every float32 position; voxel rows in first-occurrence order (oracle.coords.unique_first);
             sum: a voxel's point rows added one by one in ascending point index from +0; avg: that sum / float32(cnt);
             first: the first point's row.  Backward: gy[inverse[i]], gy[inverse[i]] / float32(cnt), gy[u] to the first point.
  slice      F[i] = x[inv_s[i]], inv_s = inverse composed with the parent maps; backward = the ordered sum.
  interpolate  q = p / float32(s), f = floorf(q), base = int(f) s, t = q - f, a[0] = 1 - t, a[1] = t; corner k = dx + 2 dy + 4 dz
             at base + s (dx, dy, dz), w[k] = (ax[dx] ay[dy]) az[dz]; y[m] = sum over the present k ascending from +0 of
             w[k, m] x[nbr[k, m]]; gx[v] = sum over the pairs e = k M + m with nbr[k, m] = v, ascending e, from +0, of w[e] gy[m].
             Invalid rows (not finite, batch outside [0, 65535), base or base + s outside (-32767, 32767)): no corner, weight +0.
  network    chain64: the test chain field -> sparse -> two convolutions -> interpolate in float64 torch autograd.
"""
import numpy as np
import torch

from oracle import coords as oc
from oracle import sparse_ops as so

F32 = np.float32
LIM = 32767


# ---- ordered sums ------------------------------------------------------------------------------------------------------------
def csr(seg, n_seg):
    """(order, offsets, cnt) of the rows of every segment in ascending row index."""
    seg = np.asarray(seg, np.int64)
    order = np.argsort(seg, kind="stable")
    cnt = np.bincount(seg, minlength=n_seg).astype(np.int64)
    return order, np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), cnt


def ordered_sum(x, seg, n_seg):
    """float32 [n_seg, c]: y[u] = the rows of x with seg == u added one by one in ascending row index from +0 (the j-th row of
    every segment in one vector operation: the order inside a segment is the sequential one)."""
    x = np.ascontiguousarray(x, dtype=F32)
    order, offsets, cnt = csr(seg, n_seg)
    y = np.zeros((n_seg, x.shape[1]), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(int(cnt.max()) if cnt.size else 0):
            sel = np.nonzero(cnt > j)[0]
            y[sel] = y[sel] + x[order[offsets[sel] + j]]
    return y


# ---- quantisation ----------------------------------------------------------------------------------------------------------------
def cells(positions):
    """int32 [N, 4]: floorf of every float32 coordinate."""
    return np.floor(np.asarray(positions, F32)).astype(np.int32)


def quantize_map(positions):
    """(voxel coords int32 [U, 4] in first-occurrence order, inverse [N], first [U], cnt [U])."""
    c = cells(positions)
    if c.shape[0] == 0:
        z = np.zeros(0, np.int64)
        return c, z, z, z
    uniq, inv, first = oc.unique_first(c)
    return uniq, inv.astype(np.int64), first.astype(np.int64), np.bincount(inv, minlength=uniq.shape[0]).astype(np.int64)


def quantize_fwd(x, inv, first, cnt, mode):
    x = np.ascontiguousarray(x, dtype=F32)
    if mode == "first":
        return x[first]
    y = ordered_sum(x, inv, cnt.shape[0])
    if mode == "avg":
        with np.errstate(invalid="ignore", over="ignore"):
            y = y / cnt.astype(F32)[:, None]
    return y


def quantize_bwd(gy, inv, first, cnt, mode):
    gy = np.ascontiguousarray(gy, dtype=F32)
    if mode == "first":
        gx = np.zeros((inv.shape[0], gy.shape[1]), F32)
        gx[first] = gy
        return gx
    if mode == "sum":
        return gy[inv]
    with np.errstate(invalid="ignore", over="ignore"):
        return gy[inv] / cnt.astype(F32)[inv][:, None]


def quantize_dense(positions):
    """float64 [U, N]: Q[u, i] = 1 where point i falls into voxel u -- from the cells alone (a dict), without unique_first."""
    c = cells(positions)
    where, rows = {}, []
    for i, r in enumerate(c):
        rows.append(where.setdefault(tuple(int(v) for v in r), len(where)))
    Q = np.zeros((len(where), c.shape[0]))
    Q[rows, np.arange(c.shape[0])] = 1.0
    return Q


def strided_inverse(coords1, inv, stride):
    """(coords of the stride's map, inverse of the points into it): the parent maps composed down from stride 1."""
    cur, s = np.asarray(coords1), 1
    while s < stride:
        s *= 2
        cur, parent = oc.stride_map(cur, s)
        inv = parent.astype(np.int64)[inv]
    return cur, inv


# ---- interpolation ---------------------------------------------------------------------------------------------------------------
def interp_geometry(positions, s):
    """(valid bool [M], batch int64 [M], base int64 [M, 3], t float32 [M, 3]) of float32 positions [M, 4] at tensor stride s."""
    p = np.ascontiguousarray(positions, dtype=F32).reshape(-1, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        q = p[:, 1:] / F32(s)
        f = np.floor(q)
        t = (q - f).astype(F32)
        valid = np.isfinite(p).all(1) & (p[:, 0] >= 0) & (p[:, 0] < 65535)
        valid &= ((f > -32768) & (f < 32768)).all(1)
        fi = np.where(np.isfinite(f) & (np.abs(f) < 32768), f, 0).astype(np.int64)
    base = fi * s
    valid &= ((base > -LIM) & (base + s < LIM)).all(1)
    batch = np.where(valid, p[:, 0], 0).astype(np.int64)
    return valid, batch, base, t


def interp_map(coords_s, positions, s):
    """-> (nbr int32 [8, M], w float32 [8, M], number of invalid rows, t float32 [M, 3], valid)."""
    valid, batch, base, t = interp_geometry(positions, s)
    M = valid.shape[0]
    where = {tuple(int(v) for v in r): i for i, r in enumerate(np.asarray(coords_s))}
    nbr = np.full((8, M), -1, np.int32)
    w = np.zeros((8, M), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.stack([(F32(1) - t).astype(F32), t], 0)                      # a[d][m, axis]
        for k in range(8):
            dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
            wk = ((a[dx][:, 0] * a[dy][:, 1]).astype(F32) * a[dz][:, 2]).astype(F32)
            w[k] = np.where(valid, wk, F32(0))
            for m in np.nonzero(valid)[0]:
                key = (int(batch[m]), int(base[m, 0] + s * dx), int(base[m, 1] + s * dy), int(base[m, 2] + s * dz))
                nbr[k, m] = where.get(key, -1)
    return nbr, w, int((~valid).sum()), t, valid


def weights64(t, valid):
    """float64 [8, M]: the exact trilinear weights of the float32 t."""
    t = t.astype(np.float64)
    a = np.stack([1.0 - t, t], 0)
    w = np.stack([a[k & 1][:, 0] * a[(k >> 1) & 1][:, 1] * a[k >> 2][:, 2] for k in range(8)], 0)
    return np.where(valid[None], w, 0.0)


def interp_fwd(x, nbr, w):
    x = np.ascontiguousarray(x, dtype=F32)
    y = np.zeros((nbr.shape[1], x.shape[1]), F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(8):
            m = nbr[k] >= 0
            y[m] = y[m] + (w[k][m][:, None] * x[nbr[k][m]]).astype(F32)
    return y


def interp_pairs(nbr):
    """(e, m, v): the present corners in ascending e = k M + m, their position row and voxel row."""
    M = nbr.shape[1]
    flat = nbr.reshape(-1).astype(np.int64)
    e = np.nonzero(flat >= 0)[0]
    return e, e % max(M, 1), flat[e]


def interp_bwd(gy, nbr, w, n_in):
    gy = np.ascontiguousarray(gy, dtype=F32)
    e, m, v = interp_pairs(nbr)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = (w.reshape(-1)[e][:, None] * gy[m]).astype(F32)
    return ordered_sum(terms, v, n_in)


def interp_fwd64(x, nbr, w64):
    """(y float64, abs-sum float64): sum_k w_k x_k and sum_k w_k |x_k| over the present corners."""
    x = np.asarray(x, np.float64)
    y = np.zeros((nbr.shape[1], x.shape[1]))
    s = np.zeros_like(y)
    for k in range(8):
        m = nbr[k] >= 0
        y[m] += w64[k][m][:, None] * x[nbr[k][m]]
        s[m] += np.abs(w64[k][m])[:, None] * np.abs(x[nbr[k][m]])
    return y, s


def interp_bwd64(gy, nbr, w64, n_in):
    """(gx float64, abs-sum float64, list length per voxel row)."""
    gy = np.asarray(gy, np.float64)
    e, m, v = interp_pairs(nbr)
    gx = np.zeros((n_in, gy.shape[1]))
    s = np.zeros_like(gx)
    np.add.at(gx, v, w64.reshape(-1)[e][:, None] * gy[m])
    np.add.at(s, v, np.abs(w64.reshape(-1)[e])[:, None] * np.abs(gy[m]))
    return gx, s, np.bincount(v, minlength=n_in)


# ---- the test chain in float64 ----------------------------------------------------------------------------------------------
def chain64(feats, pos, w1, w2):
    """The test's chain in float64 torch: average quantisation (index_add_), the two convolutions (oracle.sparse_ops), the
    interpolation as a gather of eight clamped rows times mask times the exact weights of the float32 t."""
    uniq, inv, first, cnt = quantize_map(pos)
    x = torch.zeros((uniq.shape[0], feats.shape[1]), dtype=torch.float64).index_add_(0, torch.from_numpy(inv), feats) / torch.from_numpy(cnt)[:, None]
    h = so.sparse_conv(x, w1, oc.kernel_map(uniq, uniq, oc.kernel_offsets(3, 1)))
    coords_s, s = uniq, 1
    if w2 is not None:
        coords_s, _ = oc.stride_map(uniq, 2)
        h = so.sparse_conv(h, w2, oc.kernel_map(uniq, coords_s, oc.kernel_offsets(2, 1)))
        s = 2
    nbr, _, _, t, valid = interp_map(coords_s, pos, s)
    w64 = torch.from_numpy(weights64(t, valid))
    y = sum(w64[k][:, None] * h[torch.from_numpy(nbr[k].astype(np.int64)).clamp(min=0)] * torch.from_numpy(nbr[k] >= 0)[:, None] for k in range(8))
    return y, h, x
