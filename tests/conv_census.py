"""Which convolution kernel INSTANCES run (plain helper module; imported by test_conv_census_cpu.py).

Every convolution family is a grid of compile-time instances, picked by the host code from the channel counts, the row counts and the
tile height.  With the library re-linked against the null HIP runtime of tools/dryrun every launch becomes a log line that carries the
kernel's mangled name, template arguments included, so the instances of any code path can be listed without a GPU.  Two sides:

  * network_instances(): a training step and the evaluation forwards (three precisions) of a MinkUNet variant on a synthetic room,
    through the module path and through the executor;
  * case_instances(): one conv_bounds case through the very Launch / PiecesLaunch object the GPU tests run -- forward cases once per
    operand-piece count, as test_gpu_conv_pieces.py does.

Normalisation (key(), the only place): an instance's key is  name<template arguments>  with
  * EPI dropped: an epilogue instance has no ops.* entry and is held bitwise to its twin + bn_apply by test_gpu_unet.py;
  * PROF dropped (the tools' timer instances; never launched by the product library);
  * the `_pieces_kernel` templates folded into the name of their three-piece kernel and their leading NP argument written as
    ` pieces=NP` behind the key; a three-piece launch is ` pieces=3`.  Families without reduced instances carry no suffix.
"""
import re

import torch

# kernel template -> names of its template parameters, in order (csrc/*.hip); a name not listed here is no convolution kernel
TEMPLATES = {
    "spconv_tl_kernel": ("NW", "KS", "RAGGED", "PROF", "OCC", "BUFG", "EPI"),
    "spconv_tl_pieces_kernel": ("NP", "NW", "KS", "RAGGED", "PROF", "OCC", "BUFG", "EPI"),
    "tl_reduce_parts_kernel": ("EPI",),
    "spconv_ws_kernel": ("NW", "KS", "EPI"),
    "spconv_ws_pieces_kernel": ("NP", "NW", "KS", "EPI"),
    "spconv_ws_reduce_kernel": ("KT", "EPI"),
    "spconv_rg_kernel": ("KS", "NCB", "HALVES", "OCC", "BD", "EPI"),
    "spconv_rg_pieces_kernel": ("NP", "KS", "NCB", "HALVES", "OCC", "BD", "EPI"),
    "dense_kernel": ("KS", "EPI"),
    "dense_pieces_kernel": ("NP", "KS", "EPI"),
    "spconv_fwd_x6_kernel": ("WM", "WN", "TN"),
    "spconv_fwd_kernel": ("WM", "WN", "TN", "BK"),
    "spconv_fwd_pipe_kernel": ("WM", "WN", "TN"),
    "reduce_partial_rows_kernel": (),
    "fixup_units_kernel": (),
    "wgrad_tl_kernel": ("MB", "NB", "BUFG"),
    "wgrad_tl_reduce_kernel": (),
    "wgrad_tl_reduce_batch_kernel": (),
    "spconv_wgrad_kernel": ("T", "AVEC", "GVEC"),
    "reduce_items_kernel": (),
    "stem_fwd_kernel": ("EPI",),
    "stem_fwd4_kernel": ("EPI",),
    "stem_mfma_fwd_kernel": ("EPI",),
    "stem_wgrad_kernel": (),
    "stem_wgrad_reduce_kernel": (),
    "stem_mfma_wgrad_kernel": (),
    "stem_wgrad_reduce2_kernel": (),
}
REDUCED = ("spconv_tl_kernel", "spconv_ws_kernel", "spconv_rg_kernel", "dense_kernel")     # families with `_pieces_kernel` twins
DROPPED = ("EPI", "PROF")
# a launched kernel whose name matches this and is in neither table is a convolution kernel the census does not know: it fails
CONV_LIKE = re.compile(r"conv|wgrad|stem|dense|_tl_|_ws_|_rg_|x6")
# ... these match CONV_LIKE and are no convolution arithmetic: map, list and plan builders, weight images
NOT_CONV = re.compile(r"^(wgrad_plan_kernel|weight_prep\w*|weight_transpose\w*|pair_\w+|tile_lists\w*|kmap_\w+)$")


def parse(symbol):
    """(kernel name, template arguments as a tuple of ints) of a mangled kernel symbol as the null runtime logs it, e.g.
    _ZN3osn16spconv_tl_kernelILi3ELi3ELb0ELb0ELi3ELb1ELb0EEEvPKf... -> ("spconv_tl_kernel", (3, 3, 0, 0, 3, 1, 0)); None if the
    symbol is no mangled function name.  (Read here because c++filt does not demangle the bf16 vector type of the parameter lists.)"""
    m = re.match(r"_ZN?", symbol)
    if m is None:
        return None
    rest, name = symbol[m.end():], None
    while True:                                   # the nested name's components: <length><identifier>, the kernel's own last
        n = re.match(r"\d+", rest)
        if n is None:
            break
        name = rest[n.end():n.end() + int(n.group())]
        rest = rest[n.end() + int(n.group()):]
    if name is None:
        return None
    name = name.replace("__device_stub__", "")
    args = []
    if rest.startswith("I"):
        pos = 1
        while True:
            a = re.match(r"L([ib])(n?)(\d+)E", rest[pos:])
            if a is None:
                break
            args.append(-int(a.group(3)) if a.group(2) else int(a.group(3)))
            pos += a.end()
        assert rest[pos] == "E", "template arguments of %s are not all integers / booleans" % symbol
    return name, tuple(args)


def key(name, args):
    """The census key of a launched kernel (module docstring); None for a kernel that is no convolution kernel."""
    if name not in TEMPLATES:
        assert not CONV_LIKE.search(name) or NOT_CONV.match(name), "kernel %s is not classified (conv_census.TEMPLATES / NOT_CONV)" % name
        return None
    params = TEMPLATES[name]
    assert len(params) == len(args), "%s has template arguments %s, conv_census.TEMPLATES says %s" % (name, args, params)
    vals = dict(zip(params, args))
    base = name.replace("_pieces_kernel", "_kernel")
    shown = ",".join("%s=%d" % (p, vals[p]) for p in TEMPLATES[base] if p not in DROPPED)
    suffix = " pieces=%d" % vals.get("NP", 3) if base in REDUCED else ""
    return "%s<%s>%s" % (base, shown, suffix)


def log_keys(log):
    """The set of census keys in a raw log of the null runtime."""
    keys = set()
    for sym in set(re.findall(r"^K (\S+)", log, flags=re.M)):
        p = parse(sym)
        if p is not None:
            k = key(*p)
            if k is not None:
                keys.add(k)
    return keys


class Recorder:
    """with Recorder(lib) as r: ...  -> r.keys, the instances launched inside."""

    def __init__(self, lib):
        self.lib, self.keys = lib, set()

    def __enter__(self):
        self.lib.osn_dry_reset()
        return self

    def __exit__(self, *exc):
        self.keys = log_keys(self.lib.osn_dry_log().decode())
        self.lib.osn_dry_reset()
        return False


# ----------------------------------------------------------------------------------------------------------- the network side
def room(points, voxel, dims=(4.8, 3.6, 2.4)):
    """(coords int32 [N, 4], features [N, 3]) of one synthetic room of `dims` metres."""
    from openscene_amd import synthetic as syn
    vox = syn.shuffled(syn.grid_voxels(syn.room_points(0, n_pts=points, dims=dims), voxel), 0)
    coords = torch.from_numpy(syn.batch_coords([vox]))
    return coords, torch.ones(coords.shape[0], 3)


def network_instances(lib, model, cm, feats, setattr_):
    """Instances launched by `model` on the prebuilt coordinate manager `cm`: one training step (forward + backward) and one
    evaluation forward per precision mode, each through the module path and through the executor.  -> {pass name: set of keys}"""
    import openscene_amd
    from openscene_amd import executor
    from openscene_amd.sparse import SparseTensor
    out = {}
    for path, on in (("modules", False), ("executor", True)):
        setattr_(executor, "ENABLED", on)
        model.train()
        with Recorder(lib) as r:
            y = model(SparseTensor(feats, coordinate_manager=cm))
            model.zero_grad(set_to_none=True)
            y.sum().backward()
        out["train/" + path] = r.keys
        model.eval()
        for mode in ("bf16x6", "bf16x3", "bf16x1"):
            with Recorder(lib) as r, torch.no_grad(), openscene_amd.conv_precision(mode):
                model(SparseTensor(feats, coordinate_manager=cm))
            out["eval-%s/%s" % (mode, path)] = r.keys
    return out


# -------------------------------------------------------------------------------------------------------------- the case side
def case_instances(lib, case, device=None):
    """Instances launched by one conv_bounds case through the Launch / PiecesLaunch object the GPU tests use, with zero operands of
    the case's shapes (no kernel reads them here): a weight-gradient case once, a forward case of a family with reduced instances
    once per piece count, a batched case through conv_bounds.batched_wgrad."""
    import conv_bounds as cb
    import conv_pieces as cp
    device = torch.device("cpu") if device is None else device
    rc, nbr = cb.resolve(case)
    feats = torch.zeros(rc.n_in, rc.cin, device=device)
    with Recorder(lib) as r:
        if rc.op == "wgrad":
            run = cb.Launch(rc, nbr, device)
            run.wgrad(feats, torch.zeros(rc.n_out, rc.cout, device=device))
        else:
            w = torch.zeros(rc.K, rc.cin, rc.cout, device=device)
            if case in cp.FWD_CASES:
                run = cp.PiecesLaunch(rc, nbr, device)
                for pieces in (3, 2, 1):
                    run.fwd(feats, w, pieces)
            else:
                cb.Launch(rc, nbr, device).fwd(feats, w)
    return r.keys


def batched_instances(lib, device=None):
    """Instances of the batched weight-gradient reduction as test_gpu_wgrad_batch.py calls it."""
    import conv_bounds as cb
    device = torch.device("cpu") if device is None else device

    def launch_of(case):
        rc, nbr = cb.resolve(case)
        return rc, nbr, cb.Launch(rc, nbr, device)
    with Recorder(lib) as r:
        cb.batched_wgrad(cb.batch_entries(launch_of, lambda t: t.to(device), zeros=True), device)
    return r.keys
