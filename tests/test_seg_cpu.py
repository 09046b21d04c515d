"""Host logic of the supervised-baseline pieces on the CPU: openscene_amd.optim.FlatSGD with the kernel behind osn_sgd_step
replaced by a numpy restatement of its update rule (float32, on the pointers the wrapper passes) -- parameter order, the
flat layout, frozen parameters, torch.optim.SGD's checkpoint layout both ways, learning-rate changes -- and the forms of
nn.CrossEntropyLoss that SegmentationLoss refuses."""
import ctypes

import numpy as np
import pytest
import torch


class _FakeLib:
    """osn_sgd_step in numpy, same argument list as include/openscene_amd.h."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _arr(ptr, n):
        return np.ctypeslib.as_array((ctypes.c_float * n).from_address(ptr))

    def osn_sgd_step(self, p, g, buf, n, lr, momentum, dampening, wd, nesterov, first, stream):
        self.calls.append(dict(lr=lr, momentum=momentum, first=first, buf=buf))
        f = np.float32
        p, g = self._arr(p, n), self._arr(g, n)
        d = g + f(wd) * p if wd else g.copy()
        if momentum != 0:
            b = self._arr(buf, n)
            if first:
                b[:] = d
            else:
                b[:] = f(momentum) * b + f(1.0 - dampening) * d
            d = d + f(momentum) * b if nesterov else b.copy()
        p -= f(lr) * d
        return 0


@pytest.fixture()
def fake_sgd(monkeypatch):
    from openscene_amd import ops
    lib = _FakeLib()
    monkeypatch.setattr(ops, "_prep", lambda dev: lib)
    monkeypatch.setattr(ops, "_stream", lambda dev: None)

    class NoDev:
        def __init__(self, dev):
            pass

        def __enter__(self):
            pass

        def __exit__(self, *a):
            pass
    monkeypatch.setattr(ops, "_Dev", NoDev)
    return lib


SETTINGS = [dict(momentum=0.0), dict(momentum=0.9, weight_decay=1e-4), dict(momentum=0.9, dampening=0.1),
            dict(momentum=0.9, nesterov=True, weight_decay=1e-4)]


@pytest.mark.parametrize("kw", SETTINGS)
def test_flat_sgd_follows_torch_sgd_with_lr_changes(fake_sgd, kw):
    from openscene_amd.optim import FlatSGD
    g = torch.Generator().manual_seed(2)
    shapes = [(7, 3, 5), (13,), (3, 3), (1,)]
    init = [torch.randn(s, generator=g) for s in shapes]
    ref_p = [torch.nn.Parameter(t.clone()) for t in init]
    our_p = [torch.nn.Parameter(t.clone()) for t in init]
    ref = torch.optim.SGD(ref_p, lr=0.1, **kw)
    ours = FlatSGD(our_p, lr=0.1, **kw)
    assert ours.offsets == [0, 108, 124, 136] and ours.total == 140
    assert (ours.momentum_buffer is None) == (kw["momentum"] == 0)
    for step in range(5):
        for grp in (ref.param_groups[0], ours.param_groups[0]):
            grp["lr"] = 0.1 * (1 - step / 5) ** 0.9                      # poly_learning_rate, run/train_mink.py:303-306
        for p, q in zip(ref_p, our_p):
            p.grad = torch.randn(p.shape, generator=g)
            q.grad = p.grad.clone()
        before = [q._version for q in our_p]
        ref.step()
        ours.step()
        assert all(q._version > b for q, b in zip(our_p, before))
        for p, q in zip(ref_p, our_p):
            assert torch.allclose(q.detach(), p.detach(), rtol=1e-6, atol=1e-7)
    assert [c["first"] for c in fake_sgd.calls] == ([1, 0, 0, 0, 0] if kw["momentum"] else [1] * 5)
    assert abs(fake_sgd.calls[-1]["lr"] - 0.1 * (1 - 4 / 5) ** 0.9) < 1e-9
    assert all((c["buf"] is None) == (kw["momentum"] == 0) for c in fake_sgd.calls)


def test_flat_sgd_checkpoints_round_trip_with_torch_sgd_on_a_model(fake_sgd):
    """The flat layout follows the network executor (kernels first, batch-norm pairs after), the checkpoint follows
    model.parameters() order, frozen parameters included: torch.optim.SGD's state dict loads into FlatSGD and back with every
    momentum buffer on its own parameter, and both continue to the same parameters."""
    from openscene_amd import executor as E
    from openscene_amd.mink_unet import mink_unet
    from openscene_amd.optim import FlatSGD
    torch.manual_seed(5)
    model_a = mink_unet(3, 20, 3, "MinkUNet14A")
    model_b = mink_unet(3, 20, 3, "MinkUNet14A")
    model_b.load_state_dict(model_a.state_dict())
    frozen = [n for n, _ in model_a.named_parameters()][3]
    for m in (model_a, model_b):
        dict(m.named_parameters())[frozen].requires_grad_(False)
    kw = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
    ref = torch.optim.SGD(model_a.parameters(), **kw)
    ours = FlatSGD(model_b, **kw)
    ex = E.for_model(model_b)
    assert [id(p) for p in ours._params] == [id(p) for p in ex.program.params if p.requires_grad]
    assert [id(p) for p in ours._params] != [id(p) for p in model_b.parameters() if p.requires_grad]
    assert ours.state_dict()["state"] == {}                         # no buffer before the first step, as torch
    g = torch.Generator().manual_seed(8)

    def grads():
        gs = {n: torch.randn(p.shape, generator=g) for n, p in model_a.named_parameters() if p.requires_grad}
        for m in (model_a, model_b):
            for n, p in m.named_parameters():
                if p.requires_grad:
                    p.grad = gs[n].clone()
    for _ in range(2):
        grads()
        ref.step()
        ours.step()
    ref_sd, sd = ref.state_dict(), ours.state_dict()
    assert sorted(sd["state"]) == sorted(ref_sd["state"]) and sd["param_groups"][0]["params"] == ref_sd["param_groups"][0]["params"]
    names = [n for n, _ in model_a.named_parameters()]
    for i, n in enumerate(names):
        if n == frozen:
            assert i not in sd["state"]
            continue
        assert torch.allclose(sd["state"][i]["momentum_buffer"], ref_sd["state"][i]["momentum_buffer"], rtol=1e-6, atol=1e-7), n
    # torch -> FlatSGD and FlatSGD -> torch, then one more step each: all four agree
    model_c = mink_unet(3, 20, 3, "MinkUNet14A")
    model_c.load_state_dict(model_b.state_dict())
    dict(model_c.named_parameters())[frozen].requires_grad_(False)
    from_torch = FlatSGD(model_c, lr=1.0)
    from_torch.load_state_dict(ref_sd)
    assert from_torch.param_groups[0]["lr"] == 0.01 and from_torch.param_groups[0]["momentum"] == 0.9
    model_d = mink_unet(3, 20, 3, "MinkUNet14A")
    model_d.load_state_dict(model_b.state_dict())
    dict(model_d.named_parameters())[frozen].requires_grad_(False)
    to_torch = torch.optim.SGD(model_d.parameters(), lr=1.0)
    to_torch.load_state_dict(sd)
    gs = {n: torch.randn(p.shape, generator=g) for n, p in model_a.named_parameters() if p.requires_grad}
    for m in (model_a, model_b, model_c, model_d):
        for n, p in m.named_parameters():
            if p.requires_grad:
                p.grad = gs[n].clone()
    for o in (ref, ours, from_torch, to_torch):
        o.step()
    for n, p in model_a.named_parameters():
        for m in (model_b, model_c, model_d):
            assert torch.allclose(dict(m.named_parameters())[n].detach(), p.detach(), rtol=1e-6, atol=1e-7), n
    # a state dict of a different model is refused instead of mis-assigned
    other = torch.optim.SGD(mink_unet(3, 20, 3, "MinkUNet18A").parameters(), lr=1e-3, momentum=0.9).state_dict()
    with pytest.raises(ValueError):
        ours.load_state_dict(other)


def test_flat_sgd_rejects_what_torch_rejects():
    from openscene_amd.optim import FlatSGD
    ps = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError):
        FlatSGD(ps, lr=0.1, nesterov=True)                  # Nesterov without momentum
    with pytest.raises(ValueError):
        FlatSGD(ps, lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)
    with pytest.raises(ValueError):
        FlatSGD(ps, lr=-1.0)


@pytest.mark.parametrize("kw", [dict(weight=torch.ones(3)), dict(label_smoothing=0.1), dict(reduction="sum"),
                                dict(reduction="none"), dict(size_average=False), dict(reduce=False)])
def test_segmentation_loss_refuses_unsupported_options(kw):
    from openscene_amd.losses import SegmentationLoss
    with pytest.raises(NotImplementedError):
        SegmentationLoss(ignore_index=255, **kw)


def test_segmentation_loss_refuses_unsupported_inputs():
    """Shapes and dtypes nn.CrossEntropyLoss accepts but the kernels do not compute are refused before any device work."""
    from openscene_amd.losses import SegmentationLoss, segmentation_loss
    crit = SegmentationLoss(ignore_index=255)
    assert crit.ignore_index == 255 and SegmentationLoss().ignore_index == -100      # torch's default
    x = torch.randn(6, 4)
    y = torch.tensor([0, 1, 2, 3, 255, 1])
    with pytest.raises(NotImplementedError):
        crit(torch.randn(2, 4, 3), torch.zeros(2, 3, dtype=torch.int64))            # extra dimensions
    with pytest.raises(NotImplementedError):
        crit(x, torch.softmax(x, 1))                                                 # probability targets
    with pytest.raises(NotImplementedError):
        crit(x.double(), y)
    with pytest.raises(NotImplementedError):
        crit(x, y.int())
    with pytest.raises(NotImplementedError):                                         # a gathered loss has no backward pass
        segmentation_loss(x.requires_grad_(), y, rows=torch.arange(6))
