"""numpy / torch restatements of the sparse pooling layers (helper of test_pooling_cpu.py and test_gpu_pooling.py, not a test).

Semantics as DESIGN.md section 4 states them (recalled from MinkowskiEngine v0.5.4, parity unpinned like oracle/):

  local   over a k-major neighbour table nbr[K, n_out] (oracle.coords: kernel_offsets, kernel_map, transpose_table), -1 = absent.
          float32, terms added one by one in ascending k from +0: bit for bit what the kernels compute.
          sum, avg (the sum / float32(cnt), cnt = present neighbours; 0 without one), max (ties to the lowest k, +0 == -0, the
          first NaN in k order wins and stays; arg = the input row, -1 without a neighbour).
          Backward: a gather through the inverse table in ascending FORWARD offset (flip: the forward table of an odd stride-1
          kernel read mirrored), avg terms divided before they are added, max terms selected by arg.
  global  one row per distinct batch index, ascending.  float64 sums (the kernels' order inside a chunk is theirs; the tests hold
          them to a bound), exact maxima with the lowest row among ties and NaNs first; float32 backward (each element is one
          selected value or one division).
  broadcast  y[i] = x[i] (+ | *) g[rank[i]].
  network  a float64 torch-autograd restatement of the small classifier of test_gpu_pooling.py (pooled_net_forward).
"""
import numpy as np
import torch

from oracle import coords as oc
from oracle import sparse_ops as so

F32 = np.float32


# ---- tables -------------------------------------------------------------------------------------------------------------
def tables(in_coords, out_coords, ksize, tensor_stride=1, dilation=1):
    """(nbr_fwd [K, n_out], nbr_bwd [K, n_in], flip) as CoordinateManager.kmap hands them out: an odd kernel over the rows'
    own map is its own mirror (the same table both ways, flip); every other map comes with its transposed table."""
    off = oc.kernel_offsets(ksize, tensor_stride, dilation)
    nbr = oc.kernel_map(in_coords, out_coords, off)
    if in_coords is out_coords and ksize % 2 == 1:
        return nbr, nbr, True
    return nbr, oc.transpose_table(nbr, np.asarray(in_coords).shape[0]), False


def dense_operator(in_coords, out_coords, ksize, tensor_stride=1, dilation=1):
    """float64 [n_out, n_in]: P[o, i] = 1 where in[i] = out[o] + an offset of the kernel -- from the coordinates alone (a dict
    lookup per output row and offset), without kernel_map, transpose_table or the mirror rule."""
    off = oc.kernel_offsets(ksize, tensor_stride, dilation)
    where = {tuple(int(v) for v in r): i for i, r in enumerate(np.asarray(in_coords))}
    out = np.asarray(out_coords)
    P = np.zeros((out.shape[0], len(where)))
    for o, r in enumerate(out):
        for d in off:
            i = where.get((int(r[0]), int(r[1] + d[0]), int(r[2] + d[1]), int(r[3] + d[2])))
            if i is not None:
                P[o, i] += 1.0
    return P


# ---- local pooling, float32, ascending k -----------------------------------------------------------------------------------
def local_fwd(x, nbr, mode):
    """-> (y float32 [n_out, c], arg int32 [n_out, c] or None, cnt int32 [n_out])."""
    x = np.ascontiguousarray(x, dtype=F32)
    K, n_out = nbr.shape
    c = x.shape[1]
    cnt = (nbr >= 0).sum(0).astype(np.int32)
    y = np.zeros((n_out, c), F32)
    if mode in ("sum", "avg"):
        for k in range(K):
            m = nbr[k] >= 0
            y[m] = y[m] + x[nbr[k][m]]
        if mode == "avg":
            has = cnt > 0
            y[has] = y[has] / cnt[has].astype(F32)[:, None]
            y[~has] = 0
        return y, None, cnt
    assert mode == "max"
    arg = np.full((n_out, c), -1, np.int32)
    with np.errstate(invalid="ignore"):
        for k in range(K):
            m = nbr[k] >= 0
            v, cur, a = x[nbr[k][m]], y[m], arg[m]
            take = (a < 0) | (~np.isnan(cur) & (np.isnan(v) | (v > cur)))
            y[m] = np.where(take, v, cur)
            arg[m] = np.where(take, nbr[k][m][:, None], a)
    return y, arg, cnt


def local_bwd(gy, nbr_bwd, flip, mode, cnt=None, arg=None):
    """gx float32 [n_in, c]: the terms of the forward offsets k = 0 .. K - 1, in that order, from +0."""
    gy = np.ascontiguousarray(gy, dtype=F32)
    K, n_in = nbr_bwd.shape
    gx = np.zeros((n_in, gy.shape[1]), F32)
    rows = np.arange(n_in)
    for k in range(K):
        t = nbr_bwd[K - 1 - k if flip else k]
        m = t >= 0
        o = t[m]
        if mode == "sum":
            gx[m] = gx[m] + gy[o]
        elif mode == "avg":
            gx[m] = gx[m] + gy[o] / cnt[o].astype(F32)[:, None]
        else:
            gx[m] = np.where(arg[o] == rows[m][:, None], gx[m] + gy[o], gx[m])
    return gx


# ---- global pooling ------------------------------------------------------------------------------------------------------------
def batch_index(b):
    """(ids ascending, rank [n], counts [B]) of a batch column."""
    ids, rank, counts = np.unique(np.asarray(b), return_inverse=True, return_counts=True)
    return ids, rank.reshape(-1), counts


def global_fwd64(x, b, mode):
    """-> (y float64 [B, c] (max: the selected float32 values), arg int32 [B, c] or None, counts [B])."""
    x = np.asarray(x)
    ids, rank, counts = batch_index(b)
    B, c = ids.shape[0], x.shape[1]
    y = np.zeros((B, c))
    arg = np.full((B, c), -1, np.int32) if mode == "max" else None
    for j in range(B):
        rows = np.nonzero(rank == j)[0]                       # ascending row index
        v = x[rows].astype(np.float64)
        if mode == "sum":
            y[j] = v.sum(0)
        elif mode == "avg":
            y[j] = v.sum(0) / counts[j]
        else:
            nan = np.isnan(v)
            first_nan = np.argmax(nan, 0)                     # (the first True; 0 when there is none)
            with np.errstate(invalid="ignore"):
                best = np.argmax(np.where(nan, -np.inf, v), 0)     # first occurrence: the lowest row among equals, +0 == -0
            pick = np.where(nan.any(0), first_nan, best)
            arg[j] = rows[pick]
            y[j] = v[pick, np.arange(c)]
    return y, arg, counts


def global_bwd(gy, b, mode, arg=None):
    """gx float32 [n, c]: every element one selected value (sum, max) or one division (avg)."""
    gy = np.ascontiguousarray(gy, dtype=F32)
    ids, rank, counts = batch_index(b)
    g = gy[rank]
    if mode == "sum":
        return g.copy()
    if mode == "avg":
        return g / counts[rank].astype(F32)[:, None]
    return np.where(arg[rank] == np.arange(rank.shape[0])[:, None], g, F32(0))


def broadcast_fwd(x, g, b, op):
    x, g = np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(g, dtype=F32)
    rank = batch_index(b)[1]
    return x + g[rank] if op == "add" else x * g[rank]


def broadcast_bwd64(gy, x, g, b, op):
    """(gx float32 -- streaming: gy, or gy * g[rank] --, gg float64 [B, c], abs-sum float64 [B, c] of gg's terms)."""
    gy, x, g = np.ascontiguousarray(gy, dtype=F32), np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(g, dtype=F32)
    ids, rank, counts = batch_index(b)
    gx = gy.copy() if op == "add" else gy * g[rank]
    term = gy.astype(np.float64) if op == "add" else gy.astype(np.float64) * x.astype(np.float64)
    gg, mag = np.zeros((ids.shape[0], gy.shape[1])), np.zeros((ids.shape[0], gy.shape[1]))
    np.add.at(gg, rank, term)
    np.add.at(mag, rank, np.abs(term))
    return gx, gg, mag


def sum_bound(abs_sum, counts, G):
    """First-order bound of a chunked fp32 sum against the exact one: any order inside a chunk of G rows, then p ordered adds of the
    partials: |err| <= (G + p + 1) * 2^-24 * sum |x|, p = the batch's chunks."""
    p = (np.asarray(counts) + G - 1) // G
    return (G + p + 1)[:, None] * 2.0 ** -24 * abs_sum


# ---- the small classifier of test_gpu_pooling.py, float64 torch autograd ------------------------------------------------------
def _pool_matrix(nbr, n_in, avg):
    """The local sum / average pooling of a table as a float64 [n_out, n_in] matrix."""
    K, n_out = nbr.shape
    P = torch.zeros((n_out, n_in), dtype=torch.float64)
    for k in range(K):
        o = np.nonzero(nbr[k] >= 0)[0]
        P[torch.from_numpy(o), torch.from_numpy(nbr[k][o].astype(np.int64))] += 1.0
    if avg:
        P = P / P.sum(1, keepdim=True).clamp(min=1.0)
    return P


def pooled_net_forward(p, feats, coords4, relu_masks=None):
    """conv3(3 -> 32) - BN - ReLU - AvgPooling(2, 2) - BasicBlock(32 -> 64, 1x1 conv + BN shortcut) - [GlobalAvgPooling -
    Linear(64, 64) - BroadcastMultiplication] - GlobalAvgPooling - Linear(64, 4) -> logits float64 [B, 4], training-mode batch
    norm.  p: the module tree's state_dict in float64 (names: conv, bn, block, se, final).  relu_masks: prescribed activation
    patterns, one per ReLU in call order (oracle.sparse_ops.unet_forward's rule)."""
    cm = oc.CoordinateManager(np.asarray(coords4))
    masks = list(relu_masks) if relu_masks is not None else None

    def act(y):
        if masks is None:
            return torch.relu(y)
        return y * masks.pop(0).to(y.dtype)

    def bn(x, name):
        return so.batch_norm(x, p, name + ".bn", True)

    x = act(bn(so.sparse_conv(feats, p["conv.kernel"], cm.kmap(1, 1, 3)), "bn"))
    x = _pool_matrix(cm.kmap(1, 2, 2), x.shape[0], avg=True) @ x
    t = cm.kmap(2, 2, 3)
    ident = np.arange(x.shape[0], dtype=np.int32)[None]
    y = act(bn(so.sparse_conv(x, p["block.conv1.kernel"], t), "block.norm1"))
    y = bn(so.sparse_conv(y, p["block.conv2.kernel"], t), "block.norm2")
    res = bn(so.sparse_conv(x, p["block.downsample.0.kernel"], ident), "block.downsample.1")
    x = act(y + res)
    ids, rank, counts = batch_index(cm.level(2)[:, 0])
    M = torch.zeros((ids.shape[0], x.shape[0]), dtype=torch.float64)          # the global average as a matrix
    M[torch.from_numpy(rank), torch.arange(x.shape[0])] = 1.0
    M = M / M.sum(1, keepdim=True)
    g = (M @ x) @ p["se.linear.weight"].t() + p["se.linear.bias"]
    x = x * g[torch.from_numpy(rank)]
    return (M @ x) @ p["final.linear.weight"].t() + p["final.linear.bias"]
