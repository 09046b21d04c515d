"""Shared body of the Point3DLoader tests: write the scenes of tests/golden/loader_point.npz (inputs and outputs of the
reference's REAL Point3DLoader, minted by make_golden_point_loader.py) back to disk in the reference's format, run
openscene_amd.loader.PointLoader + point_collate on them with the same seeds, and compare bit for bit."""
import os
import random

import numpy as np

# (tag, dataset, split, aug, input_color, eval_all) -- the cases of make_golden_point_loader.py
CASES = (("aug_ones", "room", "train", True, False, False),
         ("aug_color", "room", "train", True, True, False),
         ("val_all", "room", "val", False, True, True),
         ("lidar_aug", "lidar", "train", True, False, False),
         ("lidar_color", "lidar", "train", False, True, False))


def load(golden_dir):
    return np.load(os.path.join(golden_dir, "loader_point.npz"))


def write_scenes(d, root):
    """The fixture's scenes as the reference stores them (colours in [-1, 1] or the scalar 0; labels with -100)."""
    from openscene_amd import io
    for name in ("room0", "room1", "lidar0"):
        ds = name.rstrip("0123456789")
        colors = d["%s_colors" % name] if "%s_colors" % name in d.files else 0
        for split in (("train", "val") if ds == "room" else ("train",)):
            os.makedirs(os.path.join(root, ds, split), exist_ok=True)
            io.save_scene(os.path.join(root, ds, split, name + ".pth"), d["%s_xyz" % name], colors, d["%s_labels" % name])


def run(d, root, device, case):
    from openscene_amd.loader import PointLoader, point_collate
    tag, ds, split, aug, input_color, eval_all = case
    loader = PointLoader(datapath_prefix=os.path.join(str(root), ds), voxel_size=0.05, split=split, aug=aug,
                         memcache_init=False, eval_all=eval_all, input_color=input_color, device=device)
    seed = int(d["%s_seed" % tag])
    np.random.seed(seed)
    random.seed(seed)
    return point_collate([loader[i] for i in range(len(loader))])


def check(d, got, case):
    tag, eval_all = case[0], case[5]
    names = ["coords", "feats", "labels"] + (["inds_recons"] if eval_all else [])
    assert len(got) == len(names)
    for nm, g in zip(names, got):
        want = d["%s_%s" % (tag, nm)]
        g = g.cpu().numpy()
        assert g.shape == want.shape and g.dtype == want.dtype, (tag, nm, g.shape, g.dtype, want.shape, want.dtype)
        assert np.array_equal(g, want), (tag, nm, int((g != want).sum()))
