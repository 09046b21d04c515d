"""Cost of the point <-> voxel kernels (csrc/field.hip) against the same operations composed in torch on the same index tensors and
the same device.  The S100k scene as points: synthetic.room_points(0), 120 000 points at 2 cm, quantised by the field itself.

    python tools/micro_field.py [rounds] [--out FILE]

Variants are interleaved: every round times the kernel, then the torch route, each over a window of back-to-back calls of at least
20 ms after a warm-up; `rounds` rounds (default 7).  One JSON object per line:
  op=map              osn_field_map of the field's own points at stride 1 (no torch route: torch has no hash probe)
  op=interp_fwd/bwd   at 3, 32, 96 columns (forward also 768).  torch forward: a gather of the eight clamped rows ([8, M, c]) times
                      mask times weight and a sum over k; torch backward: index_add_ of w * gy over the present pairs.
  op=quantize_fwd/bwd the average quantisation.  torch forward: index_add_ of the points and a division; backward: a gather and a division.
  op=slice_fwd/bwd    forward (also 768): torch row indexing; backward: index_add_.
  us, us_min, us_max            median, minimum and maximum of the rounds, one call of the ops wrapper (allocations included)
  torch_us, ...                 the same for the torch route;  speedup = torch_us / us
  bytes                         compulsory traffic: every input row, index or table entry and output element once; hbm_share =
                                bytes / us over 8 TB/s.  The calls repeat on the same arrays: what fits the 256 MB last-level cache
                                can come from there, and hbm_share is then no share of HBM bandwidth.
The index tensors of the torch routes and the backward plan are built outside the timed region."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import ops, synthetic as syn                     # noqa: E402
from openscene_amd.field import InterpolationMap, TensorField        # noqa: E402

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = None
if "--out" in sys.argv:
    OUT = sys.argv[sys.argv.index("--out") + 1]
    ARGS = [a for a in ARGS if a != OUT]
ROUNDS = int(ARGS[0]) if ARGS else 7
WINDOW_MS = 20.0
HBM_PEAK = 8.0e12
dev = torch.device("cuda", 0)
_lines = []


def window(f, iters):
    """(us per call, calls for the next window): device events around back-to-back calls, at least WINDOW_MS long."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while True:
        a.record()
        for _ in range(iters):
            f()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= WINDOW_MS:
            return ms * 1e3 / iters, iters
        iters = int(iters * 1.2 * WINDOW_MS / max(ms, 1e-3)) + 1


def compare(kernel, torch_route):
    """Interleaved rounds of the variants (torch_route may be None) -> lists of us per call."""
    routes = [f for f in (kernel, torch_route) if f is not None]
    for f in routes:
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    times, iters = [[] for _ in routes], [3 for _ in routes]
    for _ in range(ROUNDS):
        for v, f in enumerate(routes):
            us, iters[v] = window(f, iters[v])
            times[v].append(us)
    return times[0], (times[1] if len(times) > 1 else None)


def emit(kernel_us, torch_us, nbytes, **kw):
    us = statistics.median(kernel_us)
    d = dict(kw, us=us, us_min=min(kernel_us), us_max=max(kernel_us), bytes=nbytes, hbm_share=nbytes / us * 1e6 / HBM_PEAK, rounds=ROUNDS)
    if torch_us is not None:
        tus = statistics.median(torch_us)
        d.update(torch_us=tus, torch_us_min=min(torch_us), torch_us_max=max(torch_us), speedup=tus / us)
    line = json.dumps(d)
    print(line, flush=True)
    _lines.append(line)


def agree(got, want, what):
    if not torch.allclose(got, want, rtol=1e-4, atol=1e-4):
        raise SystemExit("%s: the kernel and the torch route disagree" % what)


def main():
    gen = torch.Generator(device=dev).manual_seed(37)
    pts = syn.room_points(0)
    p = pts / 0.02
    p -= np.floor(p).min(0)                               # the grid of synthetic.grid_voxels: 100 999 voxels
    pos = np.concatenate([np.zeros((pts.shape[0], 1)), p], 1).astype(np.float32)
    field = TensorField(torch.zeros(pos.shape[0], 1, device=dev), torch.from_numpy(pos).to(dev))
    cm = field.coordinate_manager
    index = cm.point_index(1)
    N, U = pos.shape[0], cm.size(1)
    size = dict(points=N, voxels=U)
    inv, cntf = index.rank.long(), index.cnt.float()[:, None]

    emit(*compare(lambda: ops.field_map(cm._tables[1], field.C, 1), None), 4 * (4 + 16) * N, op="map", **size)
    imap = InterpolationMap(cm, 1, field.C)
    plan = imap.plan()
    P = plan.pair.shape[0]
    present = imap.nbr >= 0
    idx = imap.nbr.clamp(min=0).long()
    wm = (imap.w * present)[:, :, None]
    e_of = plan.pair.long()
    v_of, m_of, w_of = imap.nbr.reshape(-1)[e_of].long(), e_of % N, imap.w.reshape(-1)[e_of][:, None]

    for c in (3, 32, 96, 768):
        x = torch.randn(U, c, generator=gen, device=dev)

        def t_interp():
            return (x[idx] * wm).sum(0)
        agree(ops.interp_fwd(x, imap.nbr, imap.w), t_interp(), "interp_fwd c=%d" % c)
        emit(*compare(lambda: ops.interp_fwd(x, imap.nbr, imap.w), t_interp), 4 * (U * c + 16 * N + N * c), op="interp_fwd", c=c, **size)
        emit(*compare(lambda: ops.segment_expand(x, index.rank), lambda: x[inv]), 4 * (U * c + N + N * c), op="slice_fwd", c=c, **size)
        if c == 768:
            continue
        gy = torch.randn(N, c, generator=gen, device=dev)

        def t_interp_bwd():
            return torch.zeros(U, c, device=dev).index_add_(0, v_of, w_of * gy[m_of])
        agree(ops.interp_bwd(gy, plan, imap.w, U), t_interp_bwd(), "interp_bwd c=%d" % c)
        emit(*compare(lambda: ops.interp_bwd(gy, plan, imap.w, U), t_interp_bwd), 4 * (N * c + 2 * P + U * c) + 8 * (U + 1), op="interp_bwd",
             c=c, pairs=P, **size)

        def t_sum():
            return torch.zeros(U, c, device=dev).index_add_(0, inv, gy)
        agree(ops.segment_reduce(gy, index.order, index.offsets, "sum"), t_sum(), "slice_bwd c=%d" % c)
        csr_bytes = 4 * (N * c + N + U * c) + 8 * (U + 1)
        emit(*compare(lambda: ops.segment_reduce(gy, index.order, index.offsets, "sum"), t_sum), csr_bytes, op="slice_bwd", c=c, **size)
        agree(ops.segment_reduce(gy, index.order, index.offsets, "avg"), t_sum() / cntf, "quantize_fwd c=%d" % c)
        emit(*compare(lambda: ops.segment_reduce(gy, index.order, index.offsets, "avg"), lambda: t_sum() / cntf), csr_bytes, op="quantize_fwd",
             c=c, **size)
        emit(*compare(lambda: ops.segment_expand(x, index.rank, index.offsets, "avg"), lambda: (x / cntf)[inv]), csr_bytes, op="quantize_bwd",
             c=c, **size)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
