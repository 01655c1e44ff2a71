"""Host checks of the KDUNet pieces that need no GPU: the closed forms csrc/kdbn.hip computes (the BatchNorm statistics of all 3F conv
channels and the dense part of the BatchNorm backward, both from the moments of the Cin-wide input rows) against autograd of the source's
literal op sequence in float64, the model's checkpoint names, and the segmentation kd-tree loader on a synthetic opener."""
import numpy as np
import torch

from tests import kdunet_ref


def test_closed_forms_match_autograd_of_the_literal_op_sequence():
    g = torch.Generator().manual_seed(11)
    B, dim, cin, f = 3, 8, 5, 4
    M = B * dim
    f64 = dict(generator=g, dtype=torch.float64)
    x = torch.randn(B, cin, dim, **f64).requires_grad_(True)
    w = torch.randn(3 * f, cin, **f64).requires_grad_(True)
    b = torch.randn(3 * f, **f64).requires_grad_(True)
    gamma = (torch.rand(3 * f, **f64) + 0.5).requires_grad_(True)
    beta = (torch.randn(3 * f, **f64) * 0.2).requires_grad_(True)
    sel = torch.randint(0, 3, (B, dim), generator=g)                                        # one split vector per cloud
    gout = torch.randn(B, f, dim // 2, **f64)
    lit, mean_lit, var_lit = kdunet_ref.level_literal(x, sel, w, b, gamma, beta, dim)
    lit.backward(gout)

    # the same level on rows agrees with the literal sequence, and yields the decisions
    rows = x.detach().transpose(1, 2).reshape(M, cin)
    W, bb, ga, be = w.detach(), b.detach(), gamma.detach(), beta.detach()
    out, win, alive, _, _, zhat_sel = kdunet_ref.level(rows, sel.numpy(), W, bb, ga, be, B, dim)
    assert float((out.view(B, dim // 2, f).transpose(1, 2) - lit.detach()).abs().max()) <= 1e-12

    # ---- the closed forms, from the input rows' moments
    xm = rows.mean(0)
    xt = rows - xm
    C = xt.t() @ xt
    mu = W @ xm + bb
    var = torch.clamp(torch.einsum("oc,cd,od->o", W, C, W) / M, min=0.0)
    assert float((mu - mean_lit.detach()).abs().max()) <= 1e-12 and float((var - var_lit.detach()).abs().max()) <= 1e-12
    sigma = torch.sqrt(var + kdunet_ref.EPS)
    r = ga / sigma
    # g [M, 3F]: gout where (point, channel) was selected, won its pair and a > 0
    k, p = (3 * np.arange(dim) + sel.numpy()) // dim, (3 * np.arange(dim) + sel.numpy()) % dim
    G = torch.zeros(M, 3 * f, dtype=torch.float64)
    go = gout.transpose(1, 2).reshape(M // 2, f)
    for bi in range(B):
        for n in range(dim):
            m = (bi * dim + n) // 2
            for fi in range(f):
                if bool(alive[m, fi]) and int(win[m, fi]) == n % 2:
                    G[bi * dim + p[bi, n], 3 * fi + k[bi, n]] = go[m, fi]
    zhat = (xt @ W.t()) / sigma
    dbeta = G.sum(0)
    dgamma = (G * zhat).sum(0)
    dW = r.view(-1, 1) * (G.t() @ rows - (dbeta / M).view(-1, 1) * rows.sum(0).view(1, -1) - (dgamma / (M * sigma)).view(-1, 1) * (W @ C))
    v = ((r * dbeta / M).view(-1, 1) * W).sum(0)
    A = W.t() @ torch.diag(r * dgamma / (M * sigma)) @ W
    dX = (G * r) @ W - v - xt @ A
    want_dx = x.grad.transpose(1, 2).reshape(M, cin)
    for name, got, ref in (("dbeta", dbeta, beta.grad), ("dgamma", dgamma, gamma.grad), ("dW", dW, w.grad), ("dX", dX, want_dx),
                           ("d bias", torch.zeros(3 * f, dtype=torch.float64), b.grad)):
        assert float((got - ref).abs().max()) <= 1e-12, name
    assert float((dX.abs() > 0).all(1).float().mean()) == 1.0          # unlike kdconv, no point has a zero input gradient


def test_checkpoint_names_and_round_trip():
    from papc_amd import checkpoint
    from papc_amd.models import KDUNet
    torch.manual_seed(3)
    a, b = KDUNet(), KDUNet()
    state = checkpoint.export_state(a)
    want = []
    for i, (cin, f) in enumerate(((3, 32), (32, 64), (64, 256), (256, 512), (512, 1024))):
        want += [("downsample.convbnrelu%d._conv.weight" % (i + 1), (3 * f, cin, 1)), ("downsample.convbnrelu%d._conv.bias" % (i + 1), (3 * f,))]
        want += [("downsample.convbnrelu%d._batch_norm.%s" % (i + 1, k), (3 * f,)) for k in ("weight", "bias", "_mean", "_variance")]
    for i, (cin, cup, ccat, cout) in enumerate(((1024, 512, 1024, 512), (512, 512, 768, 512), (512, 256, 320, 256), (256, 256, 288, 128),
                                                (128, 128, 131, 128))):
        want += [("upsample.deconv%d.weight" % (i + 1), (cin, cup, 2)), ("upsample.deconv%d.bias" % (i + 1), (cup,))]
        blocks = [("0", ccat, cout)] + ([("1", cout, cout)] if i < 4 else [])
        for j, ci, co in blocks:
            n = "upsample.doubleconv%d.%s" % (i + 1, j)
            want += [(n + "._conv.weight", (co, ci, 1)), (n + "._conv.bias", (co,))]
            want += [(n + "._batch_norm." + k, (co,)) for k in ("weight", "bias", "_mean", "_variance")]
    want += [("upsample.doubleconv5.1.weight", (50, 128, 1)), ("upsample.doubleconv5.1.bias", (50,))]
    assert {k: tuple(v.shape) for k, v in state.items()} == dict(want)
    assert state["downsample.convbnrelu3._batch_norm._variance"].shape == (768,) and state["upsample.deconv1.weight"].shape == (1024, 512, 2)
    missing, unexpected = checkpoint.import_state(b, state, strict=True)
    assert not missing and not unexpected
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(va, vb), k


def _opener(n_clouds, n_points, seed):
    rng = np.random.default_rng(seed)

    def opener(path):
        return {"data": rng.normal(size=(n_clouds, n_points, 3)).astype(np.float32), "pid": rng.integers(0, 50, size=(n_clouds, n_points))}
    return opener


def test_seg_loader_on_a_synthetic_opener():
    from papc_amd import kdnet
    from papc_amd.datasets import KDSegDataLoader
    gen = KDSegDataLoader(max_point=1024, batchsize=3, path="shapenet", mode="test", opener=_opener(2, 1100, 7))      # 2 files x 2 clouds
    batches = list(gen())
    assert [b[1].shape[0] for b in batches] == [3, 1]
    (pts, split), label = batches[0]
    assert pts.shape == (3, 3, 1024) and pts.dtype == np.float32
    assert split.shape == (3, kdnet.PACKED) and split.dtype == np.int32 and split.min() >= 0 and split.max() <= 2
    assert label.shape == (3, 1024, 1) and label.dtype == np.int64
    # points and labels are permuted together: every output point is found in the input cloud, carrying that point's label
    src = _opener(2, 1100, 7)("x")
    for c in range(2):                                                  # the first file's two clouds are the batch's first two
        cloud, pid = src["data"][c, :1024], src["pid"][c, :1024]
        where = {tuple(pt): i for i, pt in enumerate(cloud)}
        idx = np.array([where[tuple(pt)] for pt in pts[c].T])
        assert sorted(idx) == list(range(1024))
        assert np.array_equal(label[c, :, 0], pid[idx])
    # the split dims are the classifier loader's for the same cloud
    from papc_amd.datasets import kd_split_dims
    dims, order = kd_split_dims(src["data"][0, :1024], 10)
    assert np.array_equal(split[0], np.concatenate(dims)) and np.array_equal(pts[0].T, src["data"][0, :1024][order])
    # batchsize=1: the source's one cloud per step
    one = next(iter(KDSegDataLoader(max_point=1024, batchsize=1, path="shapenet", mode="test", opener=_opener(2, 1100, 7))()))
    assert one[0][0].shape == (1, 3, 1024) and one[1].shape == (1, 1024, 1) and np.array_equal(one[1][0], label[0])
