"""Mint tests/golden/ref_loops.npz: the reference's run/distill.py and run/evaluate.py executed UNMODIFIED (tests/ref_loops.py)
on the CPU test backend, plus the top-2 margins of a CPU replay (which labels are stable enough to compare across engines).

Authoring container only (needs /root/reference):   python tests/golden/make_golden_loops.py
    --check [REFERENCE_ROOT]: run the reference's loops again and assert that they reproduce the stored fixture (nothing written)
"""
import contextlib
import io
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_loops as RL  # noqa: E402


def check(got, g):
    """A fresh run of the reference's loops (`got`) against the stored fixture `g`."""
    # the loops' own outputs: losses per iteration, the learning-rate schedule, the epoch mean, validate()'s four numbers
    assert np.allclose(got["train_loss_batch"], g["train_loss_batch"], rtol=0, atol=1e-6)
    assert np.allclose(got["train_loss_epoch"], g["train_loss_epoch"], rtol=0, atol=1e-6)
    assert np.array_equal(got["train_lr"], g["train_lr"])
    assert np.allclose(got["val"], g["val"], rtol=1e-5, atol=1e-6)
    # the batches its loaders produced (voxeliser + augmentation + collate under the run's own seeds) and the in-loop shift
    for k in g:
        if k.endswith(("_coords", "_mask", "_labels", "_code", "_inds")):
            assert np.array_equal(got[k], g[k]), k
    # the checkpoint it wrote: epoch, the full key list of models/mink_unet.py through the alias, two Adam steps
    assert int(got["ckpt_epoch"]) == 1 and float(got["optimizer_steps"]) == 2.0
    assert got["ckpt_keys"].tolist() == g["ckpt_keys"].tolist()
    from openscene_amd.disnet import DisNet
    import types
    mine = DisNet(types.SimpleNamespace(arch_3d=RL.ARCH, feature_2d_extractor="openseg"))
    assert list(mine.state_dict().keys()) == g["ckpt_keys"].tolist()
    for k in g:
        if k.startswith("ckpt:"):
            assert np.allclose(got[k], g[k], rtol=1e-6, atol=1e-8), k
    # evaluate(): predictions and mean IoU of both modes and both repeats
    for mode in ("distill", "ensemble"):
        assert int(got["eval_%s_reps" % mode]) == 2
        for rep in range(2):
            k = "eval_%s_rep%d_" % (mode, rep)
            assert np.array_equal(got[k + "gt"], g[k + "gt"])
            assert float((got[k + "pred"] == g[k + "pred"]).mean()) >= 0.9999, k
            assert abs(float(got[k + "miou"]) - float(g[k + "miou"])) <= 1e-6, k


def main():
    args = [a for a in sys.argv[1:] if a != "--check"]
    if args:
        RL.REFERENCE = args[0]
    if "--check" in sys.argv[1:]:
        g = dict(np.load(os.path.join(HERE, "ref_loops.npz")))
        root = tempfile.mkdtemp(prefix="osn_loops_")
        mp = pytest.MonkeyPatch()
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                got = RL.run_reference(root, mp)
        finally:
            mp.undo()
            shutil.rmtree(root, ignore_errors=True)
        check(got, g)
        print("the reference's loops reproduce ref_loops.npz")
        return
    root = tempfile.mkdtemp(prefix="osn_loops_")
    mp = pytest.MonkeyPatch()
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            gold = RL.run_reference(root, mp)
    finally:
        mp.undo()
        shutil.rmtree(root, ignore_errors=True)
    mp = pytest.MonkeyPatch()
    try:
        import cpu_backend
        cpu_backend.install(mp)
        import torch
        rep = RL.replay(gold, torch.device("cpu"))
    finally:
        mp.undo()
    for k, v in rep.items():
        if k.endswith("margin") or k.endswith("took_fusion"):
            gold["replay:" + k] = v
    margins = {k[len("replay:"):]: v for k, v in gold.items() if k.startswith("replay:")}
    dev = RL.compare(gold, rep, margins, what="CPU replay vs the reference run")
    print({k: (round(v, 6) if isinstance(v, float) else v) for k, v in dev.items()})
    gold.pop("pred_cloud_colors", None)
    np.savez_compressed(os.path.join(HERE, "ref_loops.npz"), **gold)
    print("wrote ref_loops.npz: %d KB" % (os.path.getsize(os.path.join(HERE, "ref_loops.npz")) // 1024))


if __name__ == "__main__":
    main()
