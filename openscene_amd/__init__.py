"""openscene_amd -- MI355X (gfx950) implementation of ONE hot path of
pengsongyou/openscene: hash voxelisation, coordinate / kernel maps, the MinkUNet
sparse-conv backbone (forward + backward) and the per-point feature x CLIP-text
query, as hand-written HIP kernels behind a C ABI (include/openscene_amd.h).

Python surface (mirrors the reference's own, file:line in each module):
    openscene_amd.minkowski        the MinkowskiEngine symbols the reference imports
    openscene_amd.field            points in and out: TensorField, .sparse(), SparseTensor.slice / .interpolate (also exported here:
                                   TensorField, SparseTensorQuantizationMode, InterpolationMap, MinkowskiInterpolation)
    openscene_amd.mink_unet        models/mink_unet.py  (MinkUNet14A..34C, `mink_unet` factory)
    openscene_amd.disnet           models/disnet.py     (DisNet)
    openscene_amd.voxelizer        dataset/voxelizer.py (Voxelizer)
    openscene_amd.query            run/evaluate.py:283-324 (distill / fusion / ensemble query)
    openscene_amd.search           README "Applications": a bank of scenes searched by text or image embedding
    openscene_amd.objects          the same, as objects: connected components of a heat-map, ranked per scene
    openscene_amd.descriptors      and back: scenes, objects and regions of the bank as descriptors (the next query)
    openscene_amd.pca              the features themselves: second moments of a bank, principal feature directions, feature colours
    openscene_amd.match            bank rows matched to exemplar rows: label by example, correspondences, novelty
    openscene_amd.regions          scenes cut into regions of agreeing features before any prompt: label, list, query by region
    openscene_amd.merge            ... and merged again by mean feature: region adjacency, star contraction of adjacent regions
    openscene_amd.render           views of a scene on the GPU: point-splat z-buffer -> heat-map / label / colour pictures, depth for fusion
    openscene_amd.neighbors        results on other points: k-nearest search on the voxel grid, transfer, fill of unseen rows, smoothing
    openscene_amd.reach            nearest sources at any range: exact distance fields on the voxel grid, "A near B", wide holes
    openscene_amd.align            two scans in one frame: rigid RANSAC over feature matches, ICP on the voxel index, overlap
    install_minkowski_alias()      make `import MinkowskiEngine` resolve to openscene_amd.minkowski
    conv_precision(name)           context: the convolutions of inference passes in "bf16x6" (default), "bf16x3" or "bf16x1"
                                   (openscene_amd.precision; set_conv_precision for the process, OSN_INFER_PRECISION at start)
    train_precision(name)          context: the same three modes for TRAINING passes, forward and backward (set_train_precision,
                                   OSN_TRAIN_PRECISION); independent of conv_precision

There is no CPU fallback: every op raises if libopenscene_amd.so is missing or
the tensors are not on a gfx950 device.
"""
import os
import sys
import types

from .precision import conv_precision, get_conv_precision, set_conv_precision  # noqa: F401  (inference arithmetic: bf16x6 / x3 / x1)
from .precision import train_precision, get_train_precision, set_train_precision  # noqa: F401  (training arithmetic, independent)

__version__ = "0.1.0"

HW_QUEUES_TUNED = 3


def configure_hw_queues(n=HW_QUEUES_TUNED, log=True):
    """Cap the HIP hardware queues of THIS PROCESS (``GPU_MAX_HW_QUEUES``; read once, when the HIP runtime initialises -- call
    this before the first device call).  Opt-in: importing openscene_amd no longer touches the environment (it used to).

    Why 3: the training step runs on three streams (main, weight gradients, next batch's maps); a fourth ACTIVE hardware
    queue -- RCCL's stream in a multi-GPU run -- slowed every launch on this part: 13.4 ms per step against 10.1 ms with the
    cap at 3 and 20 ms with 8, measured with a ONE-rank RCCL group (profiles/r03_s12_hw_queues.txt).  Streams beyond the cap
    share a queue.  Its effect on an 8-rank all-reduce is unmeasured; `OSN_HW_QUEUES=default` (or any number) overrides.
    -> the value in force (None = the runtime's default)."""
    want = os.environ.get("OSN_HW_QUEUES")
    if want is not None:
        n = None if want.strip().lower() in ("default", "", "0") else int(want)
    if "GPU_MAX_HW_QUEUES" in os.environ:               # an explicit setting of the user's wins
        val = os.environ["GPU_MAX_HW_QUEUES"]
        src = "environment"
    elif n is None:
        val, src = None, "runtime default"
    else:
        val = os.environ["GPU_MAX_HW_QUEUES"] = str(int(n))
        src = "openscene_amd.configure_hw_queues"
    if log:
        print("[openscene_amd] GPU_MAX_HW_QUEUES=%s (%s)" % (val if val is not None else "unset", src), file=sys.stderr, flush=True)
    return None if val is None else int(val)


def accelerate(target):
    """Route a MinkUNet's passes through the network executor: `target` is a MinkUNet class, an instance of one -- e.g. of the
    reference's own models/mink_unet.py:28 class built on the alias -- or a module containing one (DisNet).  See drop_in.py."""
    from .drop_in import accelerate as f
    return f(target)


def pool(bank, groups, weights=None, normalize=True):
    """Descriptors of point sets over a FeatureBank (openscene_amd.descriptors.pool)."""
    from .descriptors import pool as f
    return f(bank, groups, weights=weights, normalize=normalize)


def describe_scenes(bank, normalize=True):
    """One descriptor per scene of a FeatureBank (openscene_amd.descriptors.describe_scenes)."""
    from .descriptors import describe_scenes as f
    return f(bank, normalize=normalize)


def moments(bank, groups=None, normalize=True):
    """Count, sum and Gram matrix of a FeatureBank's rows per point set (openscene_amd.pca.moments)."""
    from .pca import moments as f
    return f(bank, groups, normalize=normalize)


def feature_colors(bank, per_scene=False):
    """Every bank row coloured by its first three principal feature directions (openscene_amd.pca.feature_colors)."""
    from .pca import feature_colors as f
    return f(bank, per_scene=per_scene)


def match_exemplars(bank, exemplars, k=1, rows=None):
    """For each bank row the k most similar exemplar rows (openscene_amd.match.match; the submodule keeps the short name)."""
    from .match import match as f
    return f(bank, exemplars, k=k, rows=rows)


def transfer_labels(bank, exemplars, k=1, rows=None, min_score=None, fill=-1):
    """Labels of the most similar exemplars for every bank row (openscene_amd.match.transfer_labels)."""
    from .match import transfer_labels as f
    return f(bank, exemplars, k=k, rows=rows, min_score=min_score, fill=fill)


def segment(bank, grid, similarity=0.9, min_points=1, names=None):
    """Regions of a grid's scenes by feature similarity of neighbouring voxels, no prompt needed (openscene_amd.regions.segment)."""
    from .regions import segment as f
    return f(bank, grid, similarity=similarity, min_points=min_points, names=names)


def merge_regions(bank, grid, regions, similarity=0.8, min_contact=1, max_rounds=64):
    """Adjacent regions of a RegionResult merged while their mean features agree (openscene_amd.merge.merge_regions)."""
    from .merge import merge_regions as f
    return f(bank, grid, regions, similarity=similarity, min_contact=min_contact, max_rounds=max_rounds)


_FIELD_NAMES = {"TensorField": "field", "SparseTensorQuantizationMode": "field", "InterpolationMap": "field",
                "MinkowskiInterpolation": "minkowski"}


def __getattr__(name):
    """The field names, resolved on first use (importing the package stays light: torch is not imported for them)."""
    if name in _FIELD_NAMES:
        import importlib
        return getattr(importlib.import_module("." + _FIELD_NAMES[name], __name__), name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def install_minkowski_alias(force=False, accelerate=True):
    """Register ``MinkowskiEngine`` (+ ``.modules.resnet_block``, ``.utils``) in
    ``sys.modules`` so the reference's imports (models/mink_unet.py:25-26,
    models/resnet_base.py:27-28, run/distill.py:18, run/evaluate.py:18) resolve to
    the HIP implementation without editing the reference.

    accelerate (default): also arrange for the reference's ``models/mink_unet.py`` -- whenever it gets imported -- to run its
    forward / backward passes through the network executor (``openscene_amd.drop_in``: the class's ``forward`` becomes a
    dispatcher that falls back to the original, module-by-module code for every pass the executor does not compile)."""
    if accelerate:
        from .drop_in import install_import_hook
        install_import_hook()
    if "MinkowskiEngine" in sys.modules and not force:
        mod = sys.modules["MinkowskiEngine"]
        if getattr(mod, "__openscene_amd__", False):
            return mod
        raise RuntimeError("a different MinkowskiEngine is already imported; pass force=True to shadow it")
    from . import minkowski as mk

    me = types.ModuleType("MinkowskiEngine")
    me.__openscene_amd__ = True
    me.__version__ = mk.__version__
    for name in ("SparseTensor", "CoordinateManager", "cat", "MinkowskiConvolution", "MinkowskiConvolutionTranspose",
                 "MinkowskiBatchNorm", "MinkowskiReLU", "MinkowskiSumPooling", "MinkowskiAvgPooling", "MinkowskiMaxPooling",
                 "MinkowskiGlobalSumPooling", "MinkowskiGlobalAvgPooling", "MinkowskiGlobalMaxPooling",
                 "MinkowskiBroadcastAddition", "MinkowskiBroadcastMultiplication", "MinkowskiLinear", "MinkowskiInterpolation",
                 "TensorField", "SparseTensorQuantizationMode"):
        setattr(me, name, getattr(mk, name))
    modules = types.ModuleType("MinkowskiEngine.modules")
    resnet_block = types.ModuleType("MinkowskiEngine.modules.resnet_block")
    resnet_block.BasicBlock = mk.BasicBlock
    resnet_block.Bottleneck = mk.Bottleneck
    modules.resnet_block = resnet_block
    utils = types.ModuleType("MinkowskiEngine.utils")
    utils.kaiming_normal_ = mk.kaiming_normal_
    utils.batched_coordinates = mk.batched_coordinates
    utils.sparse_collate = mk.sparse_collate
    me.modules = modules
    me.utils = utils
    sys.modules["MinkowskiEngine"] = me
    sys.modules["MinkowskiEngine.modules"] = modules
    sys.modules["MinkowskiEngine.modules.resnet_block"] = resnet_block
    sys.modules["MinkowskiEngine.utils"] = utils
    return me
