"""Host checks of the KD-Net pieces that need no GPU: the closed form of a level's index arithmetic against the source's literal reshape /
index_select sequence, the kd-tree loader on a synthetic opener and against the reference builder's recorded output
(tests/golden/kdtree_n1024.npz), and a checkpoint round trip of the model."""
import os

import numpy as np
import pytest
import torch

from tests import kdnet_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kdtree_n1024.npz")


@pytest.mark.parametrize("dim", [1024, 512, 8, 4, 2])
def test_closed_form_matches_the_literal_op_sequence(dim):
    g = torch.Generator().manual_seed(dim)
    B, cin, f = 2, 5, 4
    x = torch.randn(B, cin, dim, generator=g, dtype=torch.float64)
    w = torch.randn(3 * f, cin, generator=g, dtype=torch.float64)
    b = torch.randn(3 * f, generator=g, dtype=torch.float64)
    sel = torch.randint(0, 3, (dim,), generator=g)
    lit = kdnet_ref.level_literal(x, sel, w, b, dim)                                  # [B, F, dim/2]
    rows = x.transpose(1, 2).reshape(B * dim, cin)
    out, win, alive = kdnet_ref.level(rows, sel.numpy(), w, b, B, dim)
    assert float((out.view(B, dim // 2, f).transpose(1, 2) - lit).abs().max()) <= 1e-12
    # the properties the kernels lean on: the plane is non-decreasing in n; a source point feeds at most one row per plane
    k, p = kdnet_ref.closed_form(sel.numpy(), dim)
    assert (np.diff(k) >= 0).all() and k.min() >= 0 and k.max() <= 2
    for q in range(3):
        assert len(set(p[k == q])) == int((k == q).sum())


def _opener(n_clouds, n_points, seed):
    rng = np.random.default_rng(seed)

    def opener(path):
        return {"data": rng.normal(size=(n_clouds, n_points, 3)).astype(np.float32), "label": rng.integers(0, 10, size=(n_clouds, 1))}
    return opener


def test_loader_on_a_synthetic_opener():
    from papc_amd import kdnet
    from papc_amd.datasets import KDClasDataLoader
    gen = KDClasDataLoader(max_point=1024, batchsize=3, path="shapenet", mode="test", opener=_opener(2, 1100, 7))     # 2 files x 2 clouds
    batches = list(gen())
    assert [b[1].shape[0] for b in batches] == [3, 1]
    (pts, split), label = batches[0]
    assert pts.shape == (3, 3, 1024) and pts.dtype == np.float32
    assert split.shape == (3, kdnet.PACKED) and split.dtype == np.int32
    assert label.shape == (3, 1) and label.dtype == np.int64
    assert split.min() >= 0 and split.max() <= 2
    for o, d in zip(kdnet.OFFSETS, kdnet.DIMS):                    # every node's split dim is written twice
        lv = split[:, o:o + d]
        assert (lv[:, 0::2] == lv[:, 1::2]).all()
    # the points are the first max_point points of each cloud in another order
    src = _opener(2, 1100, 7)("x")["data"][0, :1024]
    assert np.array_equal(np.sort(pts[0].T, axis=0), np.sort(src, axis=0))
    # batchsize=1: the source's one cloud per step
    one = next(iter(KDClasDataLoader(max_point=1024, batchsize=1, path="shapenet", mode="test", opener=_opener(2, 1100, 7))()))
    assert one[0][0].shape == (1, 3, 1024) and np.array_equal(one[0][0][0], pts[0]) and np.array_equal(one[0][1][0], split[0])


def test_tree_matches_the_reference_builder():
    from papc_amd.datasets import kd_split_dims
    with np.load(GOLDEN) as z:
        cloud, leaf_points = z["cloud"], z["leaf_points"]
        want = [z["split_%d" % i] for i in range(10)]
    dims, order = kd_split_dims(cloud, 10)
    assert [len(v) for v in dims] == [1024 >> i for i in range(10)]
    for got, ref in zip(dims, want):
        assert np.array_equal(got, ref.astype(np.int64))
    assert np.array_equal(cloud[order], leaf_points)


def test_checkpoint_round_trip():
    from papc_amd import checkpoint
    from papc_amd.models import KDNet
    torch.manual_seed(3)
    a, b = KDNet(num_classes=10), KDNet(num_classes=10)
    assert [n for n, _ in a.named_children()] == ["conv%d" % i for i in range(1, 11)] + ["fc"]
    state = checkpoint.export_state(a)
    assert state["conv1.weight"].shape == (96, 3, 1) and state["conv10.weight"].shape == (384, 512, 1) and state["fc.weight"].shape == (128, 10)
    missing, unexpected = checkpoint.import_state(b, state, strict=True)
    assert not missing and not unexpected
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(va, vb), k
