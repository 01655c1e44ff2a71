"""Host-side tests of the VoxNet pieces: the float64 closed form the kernels implement equals the source's op sequence (tests/voxnet_ref.py),
the occupancy grid's host twin equals the source's triple loop, the voxel loader and the dispatcher follow the source, and a VoxNet's
parameters round-trip through the source's .pdparams names."""
import random

import numpy as np
import pytest
import torch

from papc_amd import _lib
from papc_amd import datasets as D
from tests import voxnet_ref as R


def _leaf(P):
    return {k: v.clone().requires_grad_(True) for k, v in P.items()}


@pytest.mark.parametrize("E", [12, 15, 16])
@pytest.mark.parametrize("B", [1, 3])
def test_closed_form_equals_literal(E, B):
    g = torch.Generator().manual_seed(100 * E + B)
    x = torch.randn(B, 1, E, E, E, generator=g, dtype=torch.float64)
    keep = (torch.rand(B, 128, generator=g) >= 0.2)
    gout = torch.randn(B, 10, generator=g, dtype=torch.float64)
    Pa, Pb = _leaf(R.params(E, 7 + E)), _leaf(R.params(E, 7 + E))
    la, sa = R.literal(Pa, x, keep=keep)
    lb, sb = R.closed(Pb, x, dec=(None, None, None, keep))
    e1, _, ep = R.edges(E)
    assert sb["y1"].shape == (B * e1 ** 3, 32) and sb["flat"].shape == (B, 32 * ep ** 3) and sb["win"].shape == (B * ep ** 3, 32)
    assert int(sb["win"].max()) <= 7
    for k in ("flat", "mean", "var"):
        assert torch.allclose(sa[k], sb[k], rtol=1e-11, atol=1e-12), k
    assert torch.allclose(la, lb, rtol=1e-11, atol=1e-12)
    la.backward(gout)
    lb.backward(gout)
    for k in Pa:
        # (conv1's bias feeds a train-mode norm: its gradient is rounding noise around 0, read on the scale of its weight's gradient)
        scale = float(Pa["backbone.0.weight" if k == "backbone.0.bias" else k].grad.abs().max())
        assert scale > 1e-6, k
        assert float((Pa[k].grad - Pb[k].grad).abs().max()) <= 1e-10 * scale, k
    # a bias under a train-mode norm: no gradient beyond rounding
    assert float(Pb["backbone.0.bias"].grad.abs().max()) <= 1e-12 * float(Pb["backbone.0.weight"].grad.abs().max())


def test_closed_form_eval_stats_and_pinned_decisions():
    """eval mode (given statistics) agrees too, and pinning the closed form's own decisions changes nothing"""
    E, B = 12, 2
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 1, E, E, E, generator=g, dtype=torch.float64)
    P = R.params(E, 3)
    stats = (0.1 * torch.randn(32, generator=g, dtype=torch.float64), 0.5 + torch.rand(32, generator=g, dtype=torch.float64))
    la, _ = R.literal(P, x, stats=stats)
    lb, bb = R.closed(P, x, stats=stats)
    assert torch.allclose(la, lb, rtol=1e-11, atol=1e-12)
    lc, _ = R.closed(P, x, dec=(bb["win"], bb["sign1"], None, None), stats=stats)
    assert torch.equal(lb, lc)


def test_occupancy_grid_np_equals_the_source_loop():
    from papc_amd import voxnet
    pts = R.occupancy_fixture()
    s = R.straddlers()
    assert len(s) >= 8                                      # the fixture does hold coordinates whose fp32 and float64 indices differ
    h = np.float32(15.5)
    assert all(int(float(c) * 15.5 + 15.5) != int(np.float32(c * h + h)) for c in s)
    assert (pts == -1.0).any() and (pts == 0.0).any() and (pts == 1.0).any()
    got = voxnet.occupancy_grid_np(pts)
    assert got.dtype == np.float32 and got.shape == (2, 1, 32, 32, 32)
    assert np.array_equal(got, R.occupancy_loop(pts))
    assert got[0, 0, 0, 15, 31] == 1.0 and got[1, 0, 31, 31, 31] == 1.0 and got[1, 0, 0, 0, 0] == 1.0
    small = voxnet.occupancy_grid_np(pts, edge=12)
    assert np.array_equal(small, R.occupancy_loop(pts, edge=12))
    for bad in (np.float32(1.0000001), np.float32(-1.5), np.float32("nan")):
        p = pts.copy()
        p[1, 5, 2] = bad
        with pytest.raises(_lib.PapcError, match="outside"):
            voxnet.occupancy_grid_np(p)


def _write_lists(tmp_path, n=5):
    rng = np.random.default_rng(1)
    grids, names = [], []
    for i in range(n):
        gr = (rng.random((32, 32, 32)) < 0.02).astype(np.float32)
        name = D.categoryList[(3 * i) % 10]
        (tmp_path / name).mkdir(exist_ok=True)
        np.save(tmp_path / name / ("m%d.npy" % i), gr)
        grids.append(gr)
        names.append(name)
    for split in ("train.txt", "test.txt"):
        with open(tmp_path / split, "w") as f:
            for i, name in enumerate(names):
                # (absolute paths in one list, paths relative to the data directory in the other)
                f.write("%s %s\n" % (str(tmp_path / name / ("m%d.npy" % i)) if split == "train.txt" else "%s/m%d.npy" % (name, i), name))
    return np.stack(grids), np.asarray([D.category[n_] for n_ in names])


def test_vox_loader(tmp_path):
    grids, labels = _write_lists(tmp_path)
    assert D.category == {n: i for i, n in enumerate(D.categoryList)} and len(D.categoryList) == 10
    gen = D.VoxDataLoader(1024, 2, str(tmp_path), "test")
    for _ in range(2):                                      # test mode: list order, every epoch
        batches = list(gen())
        assert [b[0].shape for b in batches] == [(2, 1, 32, 32, 32), (2, 1, 32, 32, 32), (1, 1, 32, 32, 32)]      # the short last batch is kept
        assert [b[1].shape for b in batches] == [(2, 1), (2, 1), (1, 1)]
        assert all(b[0].dtype == np.float32 and b[1].dtype == np.int64 for b in batches)
        assert np.array_equal(np.concatenate([b[0] for b in batches])[:, 0], grids)
        assert np.array_equal(np.concatenate([b[1] for b in batches]).reshape(-1), labels)
    gen = D.VoxDataLoader(1024, 2, str(tmp_path), "train")
    random.seed(11)
    order = list(range(5))
    want = []
    for _ in range(2):                                      # train mode: the source shuffles the previous epoch's order in place
        random.shuffle(order)
        want.append(list(order))
    random.seed(11)
    for ep in range(2):
        batches = list(gen())
        assert np.array_equal(np.concatenate([b[0] for b in batches])[:, 0], grids[want[ep]])
        assert np.array_equal(np.concatenate([b[1] for b in batches]).reshape(-1), labels[want[ep]])
    assert want[0] != list(range(5)) or want[1] != list(range(5))


def test_dispatcher_returns_the_vox_loader(tmp_path):
    grids, _ = _write_lists(tmp_path)
    gen = D.DataLoader("voxnet", 1024, 4, str(tmp_path), "clas", "test")
    assert gen.__name__ == "VoxDataGenerator"
    x, y = next(iter(gen()))
    assert x.shape == (4, 1, 32, 32, 32) and y.shape == (4, 1) and np.array_equal(x[:, 0], grids[:4])
    with pytest.raises(SystemExit):
        D.DataLoader("voxnet", 1024, 4, str(tmp_path), "seg", "test")


def test_pdparams_round_trip(tmp_path):
    from papc_amd import checkpoint
    from papc_amd.models import VoxNet
    torch.manual_seed(3)
    a = VoxNet(num_classes=10)
    with torch.no_grad():
        a.backbone[1].running_mean.normal_()
        a.backbone[1].running_var.uniform_(0.5, 2.0)
    names = [k for k, _ in a.named_parameters()]
    assert names == ["backbone.0.weight", "backbone.0.bias", "backbone.1.weight", "backbone.1.bias", "backbone.3.weight", "backbone.3.bias",
                     "head.0.weight", "head.0.bias", "head.3.weight", "head.3.bias"]
    state = checkpoint.export_state(a)
    assert set(state) == set(names) | {"backbone.1._mean", "backbone.1._variance"}
    assert state["backbone.0.weight"].shape == (32, 1, 5, 5, 5) and state["backbone.3.weight"].shape == (32, 32, 3, 3, 3)
    assert state["head.0.weight"].shape == (6912, 128) and state["head.3.weight"].shape == (128, 10)      # Paddle's Linear is [in, out]
    assert np.array_equal(state["head.0.weight"], a.head[0].weight.detach().numpy().T)
    checkpoint.save_pdparams(a, str(tmp_path / "v.pdparams"))
    b = VoxNet(num_classes=10)
    missing, unexpected = checkpoint.import_state(b, checkpoint.load_pdparams(str(tmp_path / "v.pdparams")), strict=True)
    assert not missing and not unexpected
    for (k, ta), (_, tb) in zip(a.state_dict().items(), b.state_dict().items()):
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(ta, tb), k
