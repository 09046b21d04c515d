"""Cost of the sparse pooling kernels (csrc/pooling.hip) against the same reductions composed in torch on the same tables and the same
device.  The S100k scene (synthetic.room_points(0) at 2 cm, 100 999 voxels; its stride-2 level has 47 618) and the 8-scene batch.

    python tools/micro_pooling.py [rounds] [--out FILE]

Variants are interleaved: every round times the kernel, then the torch route, each over a window of back-to-back calls of at least
20 ms after a warm-up; `rounds` rounds (default 7).  One JSON object per line:
  kind=local    map k2s2 (100 999 -> 47 618 rows) at 32 and 96 channels, k3s1 (the 47 618-row self map) at 96; mode sum / avg / max;
                pass fwd / bwd.  torch forward: a gather of the clamped table ([K, n_out, c]), the absent entries masked, sum / amax over
                k (avg: divided by the count); torch backward: index_add_ of the gathered output gradients over the map's pairs
                (avg: divided first; max: a flat index_add_ on arg).  The index tensors are built outside the timed region.
  kind=global   sum / max over 100 999 x 96 (one scene) and over the 8-scene batch; torch: index_add_ / scatter_reduce(amax).
  us, us_min, us_max            median, minimum and maximum of the rounds, one call of the ops wrapper (allocations included)
  torch_us, ...                 the same for the torch route;  speedup = torch_us / us
  bytes                         compulsory traffic: every input row, table entry and output element once (arg / cnt where read or
                                written); hbm_share = bytes / us over 8 TB/s.  The calls repeat on the same arrays: what fits the
                                256 MB last-level cache can come from there, and hbm_share is then no share of HBM bandwidth."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openscene_amd import ops, synthetic as syn                     # noqa: E402
from openscene_amd.sparse import CoordinateManager                   # noqa: E402

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
    """Interleaved rounds of the two variants -> two lists of us per call."""
    for f in (kernel, torch_route):
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    times, iters = ([], []), [3, 3]
    for _ in range(ROUNDS):
        for v, f in enumerate((kernel, torch_route)):
            us, iters[v] = window(f, iters[v])
            times[v].append(us)
    return times


def emit(kernel_us, torch_us, nbytes, **kw):
    us, tus = statistics.median(kernel_us), statistics.median(torch_us)
    line = json.dumps(dict(kw, us=us, us_min=min(kernel_us), us_max=max(kernel_us), torch_us=tus, torch_us_min=min(torch_us),
                           torch_us_max=max(torch_us), speedup=tus / us, bytes=nbytes, hbm_share=nbytes / us * 1e6 / HBM_PEAK,
                           rounds=ROUNDS))
    print(line, flush=True)
    _lines.append(line)


def local_case(name, cm, s_in, s_out, ksize, c, gen):
    nbr, nbr_bwd, flip = cm.kmap(s_in, s_out, ksize)
    K, n_out = nbr.shape
    n_in = cm.size(s_in)
    x = torch.randn(n_in, c, generator=gen, device=dev)
    gy = torch.randn(n_out, c, generator=gen, device=dev)
    cnt = cm.pool_counts(s_in, s_out, ksize)
    present = nbr >= 0
    idx = nbr.clamp(min=0).long()
    k_of, o_of = present.nonzero(as_tuple=True)
    i_of = nbr[k_of, o_of].long()
    cntf = cnt.float()[:, None]
    cols = torch.arange(c, device=dev)[None]
    for mode in ops.POOL_MODES:
        y, arg = ops.pool_fwd(x, nbr, mode)

        def torch_fwd():
            g = x[idx]
            if mode == "max":
                return g.masked_fill(~present[:, :, None], float("-inf")).amax(0)
            s = (g * present[:, :, None]).sum(0)
            return s / cntf if mode == "avg" else s
        want = torch_fwd()
        if not torch.allclose(y, want, rtol=1e-4, atol=1e-4):
            raise SystemExit("%s %s: the kernel and the torch route disagree" % (name, mode))
        fwd_bytes = 4 * (n_in * c + K * n_out + n_out * c * (2 if mode == "max" else 1))
        emit(*compare(lambda: ops.pool_fwd(x, nbr, mode), torch_fwd), fwd_bytes, kind="local", map=name, n_in=n_in, n_out=n_out, K=K,
             c=c, mode=mode, **{"pass": "fwd"})
        flat = (arg.long() * c + cols).reshape(-1) if mode == "max" else None

        def torch_bwd():
            gx = torch.zeros(n_in, c, device=dev)
            if mode == "max":
                return gx.view(-1).index_add_(0, flat, gy.reshape(-1)).view(n_in, c)
            return gx.index_add_(0, i_of, (gy / cntf if mode == "avg" else gy)[o_of])
        got = ops.pool_bwd(gy, nbr_bwd, flip, mode, cnt=cnt, arg=arg)
        if not torch.allclose(got, torch_bwd(), rtol=1e-4, atol=1e-4):
            raise SystemExit("%s %s backward: the kernel and the torch route disagree" % (name, mode))
        bwd_bytes = 4 * (n_out * c * (2 if mode == "max" else 1) + K * n_in + n_in * c + (n_out if mode == "avg" else 0))
        emit(*compare(lambda: ops.pool_bwd(gy, nbr_bwd, flip, mode, cnt=cnt, arg=arg), torch_bwd), bwd_bytes, kind="local", map=name,
             n_in=n_in, n_out=n_out, K=K, c=c, mode=mode, **{"pass": "bwd"})
        del y, arg, want, got


def global_case(name, cm, c, gen):
    index = cm.batch_index(1)
    n, B = cm.size(1), index.ids.shape[0]
    x = torch.randn(n, c, generator=gen, device=dev)
    rank = index.rank.long()
    rank_c = rank[:, None].expand(-1, c)
    for mode in ("sum", "max"):
        def torch_route():
            if mode == "sum":
                return torch.zeros(B, c, device=dev).index_add_(0, rank, x)
            return torch.zeros(B, c, device=dev).scatter_reduce(0, rank_c, x, "amax", include_self=False)
        y = ops.gpool_fwd(x, index.order, index.offsets, mode)[0]
        if not torch.allclose(y, torch_route(), rtol=1e-4, atol=1e-2):
            raise SystemExit("%s %s: the kernel and the torch route disagree" % (name, mode))
        nbytes = 4 * (n * c + n + B * c * (2 if mode == "max" else 1))
        emit(*compare(lambda: ops.gpool_fwd(x, index.order, index.offsets, mode), torch_route), nbytes, kind="global", case=name, n=n,
             batches=B, c=c, mode=mode, chunk=ops.GPOOL_CHUNK)


def main():
    gen = torch.Generator(device=dev).manual_seed(36)
    vox = [syn.shuffled(syn.grid_voxels(syn.room_points(b), 0.02), b) for b in range(8)]
    one = CoordinateManager(torch.from_numpy(syn.batch_coords(vox[:1])).to(dev))
    local_case("k2s2", one, 1, 2, 2, 32, gen)
    local_case("k2s2", one, 1, 2, 2, 96, gen)
    local_case("k3s1", one, 2, 2, 3, 96, gen)
    global_case("one_scene", one, 96, gen)
    del one
    global_case("eight_scenes", CoordinateManager(torch.from_numpy(syn.batch_coords(vox)).to(dev)), 96, gen)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
