"""Mint tests/golden/reference_model_file.npz: the REFERENCE's own models/mink_unet.py, unmodified, imported through
openscene_amd's MinkowskiEngine alias and run on the CPU test backend (tests/cpu_backend.py) -- what
tests/test_host_logic.py::test_reference_model_file_runs_unchanged compares our mirror against.

Authoring container only (needs the reference tree; its root is the first argument):
    python tests/golden/make_golden_model_file.py REFERENCE_ROOT
Stored:
  keys, shapes              the state_dict layout of mink_unet(3, 10, 3, "MinkUNet14A")
  init_sum, init_sq         per state_dict entry: sum and sum of squares (float64) of its values after torch.manual_seed(0)
  coords, feats             the input (two batches of a random cloud, float64 features)
  out_eval, out_train       the float64 model's output in eval mode, then in train mode (batch statistics)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def cloud(seed=0, n=260, extent=11, batch=2):
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(batch):
        g = np.unique(rng.integers(0, extent, (n, 3)), axis=0)
        g = g[rng.permutation(g.shape[0])]
        rows.append(np.concatenate([np.full((g.shape[0], 1), b), g], 1))
    return torch.from_numpy(np.concatenate(rows, 0).astype(np.int32))


def main():
    import pytest
    import cpu_backend
    import openscene_amd
    mp = pytest.MonkeyPatch()
    try:
        cpu_backend.install(mp)
        openscene_amd.install_minkowski_alias()
        sys.path.insert(0, sys.argv[1])
        from models.mink_unet import mink_unet as theirs            # the reference file, unmodified
        import MinkowskiEngine as ME
        assert ME.__openscene_amd__
        torch.manual_seed(0)
        model = theirs(3, 10, 3, "MinkUNet14A").double().eval()
        sd = model.state_dict()
        layout = dict(keys=np.array(list(sd.keys())), shapes=np.array([str(tuple(v.shape)) for v in sd.values()]),
                      init_sum=np.array([float(v.double().sum()) for v in sd.values()]),
                      init_sq=np.array([float(v.double().square().sum()) for v in sd.values()]))
        coords = cloud(5)
        feats = torch.rand(coords.shape[0], 3, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
        out_eval = model(ME.SparseTensor(feats, coords)).detach()
        model.train()
        out_train = model(ME.SparseTensor(feats, coords)).detach()
    finally:
        mp.undo()
    path = os.path.join(HERE, "reference_model_file.npz")
    np.savez_compressed(path, coords=coords.numpy(), feats=feats.numpy(), out_eval=out_eval.numpy(), out_train=out_train.numpy(),
                        **layout)
    print("wrote %s: %d entries, %d voxels, %.1f KB" % (path, len(sd), coords.shape[0], os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
