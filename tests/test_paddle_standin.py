"""Known-answer cases for the paddle stand-in (oracle/paddle_standin): one hand-computed case per entry of the table in its package
docstring.  The stand-in is what tests/golden/make_reference_golden.py executes the reference's model code on, so every Paddle behaviour
the fixtures rest on is stated there and held here.  CPU only; the stand-in is on sys.path only while this module's fixture is alive."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle.paddle_standin import on_path
from tests.util import reference_weight


@pytest.fixture(scope="module")
def paddle():
    with on_path():
        import paddle as p
        p.set_float("float32")
        p.TIE_RULE = "all"
        yield p
        p.set_float("float32")
    assert "paddle" not in sys.modules and not any(s.endswith("paddle_standin") for s in sys.path)


def T(paddle, a, dtype=np.float32):
    return paddle.to_tensor(np.asarray(a, dtype))


def test_not_importable_by_default():
    assert not any(s.rstrip(os.sep).endswith("paddle_standin") for s in sys.path)


def test_unknown_names_raise_by_name(paddle):
    for mod, name in ((paddle, "einsum"), (paddle.nn, "GRU"), (paddle.nn.functional, "gelu")):
        with pytest.raises(AttributeError, match=name):
            getattr(mod, name)


def test_to_tensor(paddle):                                                  # T1
    a64 = np.array([1.5, 2.5])
    t = paddle.to_tensor(a64)
    assert t.dtype == torch.float64 and not t.requires_grad and t.is_leaf and t.stop_gradient
    a64[0] = 9.0
    assert t.numpy()[0] == 1.5                                               # a copy
    assert paddle.to_tensor(np.array([1, 2], np.int8)).dtype == torch.int8
    w = T(paddle, [1.0, 2.0])
    w.stop_gradient = False
    d = paddle.to_tensor(w * 2)
    assert not d.requires_grad and d.grad_fn is None and d.numpy().tolist() == [2.0, 4.0]


def test_numpy_detaches(paddle):                                             # T2
    w = T(paddle, [1.0, 2.0])
    w.stop_gradient = False
    y = w * 3
    assert y.requires_grad and y.numpy().tolist() == [3.0, 6.0]


def test_float_switch(paddle):                                               # T3
    try:
        assert paddle.zeros([2, 3]).dtype == torch.float32 and paddle.ones((2,)).dtype == torch.float32 and paddle.eye(3).dtype == torch.float32
        assert paddle.to_tensor(np.eye(2)).astype("float32").dtype == torch.float32
        paddle.set_float("float64")
        assert paddle.zeros([2, 3]).dtype == torch.float64 and paddle.ones([2]).dtype == torch.float64 and paddle.eye(3).dtype == torch.float64
        assert paddle.to_tensor(np.eye(2)).astype("float32").dtype == torch.float64
        assert paddle.to_tensor(np.zeros(2, np.float32)).dtype == torch.float32      # to_tensor keeps the array's type in either mode
        assert paddle.nn.Linear(2, 3).weight.dtype == torch.float64
        assert paddle.ones([2, 2]).sum().item() == 4.0 and paddle.eye(3).numpy()[1].tolist() == [0.0, 1.0, 0.0]
    finally:
        paddle.set_float("float32")


def test_transpose_reshape(paddle):                                          # T4
    x = T(paddle, np.arange(24).reshape(2, 3, 4))
    y = x.transpose([0, 2, 1])
    assert tuple(y.shape) == (2, 4, 3) and y.numpy()[1, 3, 2] == 12 + 2 * 4 + 3
    assert paddle.transpose(x, (2, 0, 1)).numpy()[3, 1, 2] == 12 + 2 * 4 + 3
    assert tuple(x.reshape([4, -1]).shape) == (4, 6) and tuple(paddle.reshape(x, (-1, 2)).shape) == (12, 2)
    with pytest.raises(AssertionError):
        x.transpose([0, 1])                                                  # torch's two-axis swap is NOT paddle's transpose


def test_max_values_and_tie_rule(paddle):                                    # T5
    a = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 0.0, 5.0, 5.0]], np.float32)
    for rule, grad in (("all", [[0, 2, 2, 0], [7, 0, 7, 7]]), ("first", [[0, 2, 0, 0], [7, 0, 0, 0]])):
        paddle.TIE_RULE = rule
        x = T(paddle, a)
        x.stop_gradient = False
        m = paddle.max(x, axis=1)
        assert isinstance(m, paddle.Tensor) and m.numpy().tolist() == [3.0, 5.0]          # values only, no (values, indices) pair
        assert x.max(axis=-1, keepdim=True).numpy().tolist() == [[3.0], [5.0]]
        (m * T(paddle, [2.0, 7.0])).sum().backward()
        assert x.grad.numpy().tolist() == grad, rule
    paddle.TIE_RULE = "all"


def test_sort_argsort(paddle):                                               # T6, T7
    a = np.array([[2.0, 1.0, 2.0, 1.0, 0.5]], np.float32)
    s = paddle.sort(T(paddle, a), axis=-1)
    assert isinstance(s, paddle.Tensor) and s.numpy().tolist() == [[0.5, 1.0, 1.0, 2.0, 2.0]]
    assert T(paddle, a).sort(axis=-1)[:, :2].numpy().tolist() == [[0.5, 1.0]]              # sliced directly: values, not a pair
    assert paddle.argsort(T(paddle, a), axis=-1).numpy().tolist() == [[4, 1, 3, 0, 2]]     # equal keys keep their order
    assert paddle.argsort(s, axis=-1).numpy().tolist() == [[0, 1, 2, 3, 4]]                # argsort of a sorted row: the FP layer's quirk
    i = T(paddle, [[3, 7, 3, 0]], np.int64).sort(axis=-1)
    assert i.dtype == torch.int64 and i.numpy().tolist() == [[0, 3, 3, 7]]


def test_argmax_first(paddle):                                               # T8
    r = paddle.argmax(T(paddle, [[1.0, 4.0, 4.0], [2.0, 2.0, 2.0]]), -1)
    assert r.dtype == torch.int64 and r.numpy().tolist() == [1, 0]


def test_small_ops(paddle):                                                  # T9
    x = T(paddle, [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    assert paddle.sum(x, axis=-1).numpy().tolist() == [6.0, 15.0] and tuple(paddle.sum(x, axis=1, keepdim=True).shape) == (2, 1)
    a = T(paddle, np.arange(12).reshape(2, 2, 3))
    b = T(paddle, np.ones((2, 3, 1)))
    assert paddle.matmul(a, b).numpy().reshape(-1).tolist() == [3.0, 12.0, 21.0, 30.0]
    assert paddle.concat([x, x * 2], axis=1).numpy()[1].tolist() == [4.0, 5.0, 6.0, 8.0, 10.0, 12.0]
    assert paddle.concat([x, x * 2], 0).numpy()[3].tolist() == [8.0, 10.0, 12.0]
    t = paddle.tile(T(paddle, [[1.0, 2.0]]), [2, 2])
    assert t.numpy().tolist() == [[1.0, 2.0, 1.0, 2.0], [1.0, 2.0, 1.0, 2.0]]
    assert tuple(paddle.squeeze(x, axis=-1).shape) == (2, 3)                  # an axis longer than 1: no-op
    assert tuple(paddle.squeeze(x.reshape([2, 3, 1]), axis=-1).shape) == (2, 3)
    assert tuple(paddle.unsqueeze(x, 1).shape) == (2, 1, 3) and tuple(x.unsqueeze(1).shape) == (2, 1, 3)
    sel = paddle.index_select(x, axis=1, index=T(paddle, [2, 0], np.int64))
    assert sel.numpy().tolist() == [[3.0, 1.0], [6.0, 4.0]]
    assert (x > 2.0).numpy().tolist() == [[False, False, True], [True, True, True]]


def test_arange_randint(paddle):                                             # T10, T11
    assert paddle.arange(4).dtype == torch.int64 and paddle.arange(4).numpy().tolist() == [0, 1, 2, 3]
    assert (paddle.arange(0, 3) * 3).numpy().tolist() == [0, 3, 6]
    paddle.RANDINT_QUEUE[:] = [np.array([5, 2]), np.array([1, 1])]
    r = paddle.randint(0, 8, (2,))
    assert r.dtype == torch.int64 and r.numpy().tolist() == [5, 2]
    assert paddle.randint(0, 8, (2,)).numpy().tolist() == [1, 1]
    with pytest.raises(RuntimeError):
        paddle.randint(0, 8, (2,))
    paddle.RANDINT_QUEUE[:] = [np.array([9, 0])]
    with pytest.raises(AssertionError):
        paddle.randint(0, 8, (2,))                                           # a queued draw outside [low, high)
    paddle.RANDINT_QUEUE[:] = []


def test_setitem_casts(paddle):                                              # T12
    c = paddle.zeros([2, 3])
    c[:, 1] = T(paddle, [7, 9], np.int64)
    assert c.dtype == torch.float32 and c.numpy().tolist() == [[0.0, 7.0, 0.0], [0.0, 9.0, 0.0]]
    assert c.numpy().astype("int64")[1, 1] == 9


def _set(p, a):
    with torch.no_grad():
        p.copy_(torch.as_tensor(np.asarray(a, np.float32)))


def test_linear(paddle):                                                     # L1
    lin = paddle.nn.Linear(2, 3)
    assert tuple(lin.weight.shape) == (2, 3) and tuple(lin.bias.shape) == (3,)
    _set(lin.weight, [[1, 2, 3], [4, 5, 6]])
    _set(lin.bias, [0.5, 0.0, -0.5])
    assert lin(T(paddle, [[1.0, 10.0]])).numpy().tolist() == [[41.5, 52.0, 62.5]]          # x W + b with W [in, out]


@pytest.mark.parametrize("cls", ["BatchNorm", "BatchNorm1D"])
def test_batchnorm_train_eval(paddle, cls):                                  # L2
    bn = getattr(paddle.nn, cls)(2)
    assert list(bn.state_dict().keys()) == ["weight", "bias", "_mean", "_variance"]
    assert [n for n, _ in bn.named_parameters()] == ["weight", "bias"] and not bn._mean.requires_grad
    assert bn.weight.numpy().tolist() == [1.0, 1.0] and bn._variance.numpy().tolist() == [1.0, 1.0] and bn._mean.numpy().tolist() == [0.0, 0.0]
    _set(bn.weight, [2.0, 1.0])
    _set(bn.bias, [1.0, 0.0])
    # channel 0 holds 1, 3, 5, 7 over (batch, length): mean 4, BIASED variance 5 (unbiased 20/3); channel 1 holds 0, 0, 4, 4: mean 2, variance 4
    x = T(paddle, [[[1.0, 3.0], [0.0, 0.0]], [[5.0, 7.0], [4.0, 4.0]]])
    y = bn(x).numpy()
    inv0, inv1 = 1.0 / np.sqrt(5.0 + 1e-5), 1.0 / np.sqrt(4.0 + 1e-5)
    np.testing.assert_allclose(y[:, 0].reshape(-1), np.array([-3, -1, 1, 3]) * inv0 * 2.0 + 1.0, rtol=1e-6)
    np.testing.assert_allclose(y[:, 1].reshape(-1), np.array([-2, -2, 2, 2]) * inv1, rtol=1e-6)
    np.testing.assert_allclose(bn._mean.numpy(), [0.1 * 4.0, 0.1 * 2.0], rtol=1e-6)                         # 0.9 * 0 + 0.1 * batch
    np.testing.assert_allclose(bn._variance.numpy(), [0.9 + 0.1 * 5.0, 0.9 + 0.1 * 4.0], rtol=1e-6)         # ... of the BIASED variance
    bn.eval()
    y = bn(T(paddle, [[[0.4], [0.2]]])).numpy().reshape(-1)                                                  # x == running mean -> beta
    np.testing.assert_allclose(y, [1.0, 0.0], atol=1e-6)
    y = bn(T(paddle, [[[1.4], [1.2]]])).numpy().reshape(-1)
    np.testing.assert_allclose(y, [2.0 / np.sqrt(1.4 + 1e-5) + 1.0, 1.0 / np.sqrt(1.3 + 1e-5)], rtol=1e-6)
    np.testing.assert_allclose(bn._mean.numpy(), [0.4, 0.2], rtol=1e-6)                                      # eval updates nothing
    np.testing.assert_allclose(bn._variance.numpy(), [1.4, 1.3], rtol=1e-6)


def test_batchnorm_ranks(paddle):                                            # L2: 2-D rows, 4-D and 5-D maps normalise over everything but axis 1
    rng = np.random.default_rng(0)
    for cls, shape in (("BatchNorm1D", (6, 3)), ("BatchNorm2D", (2, 3, 4, 5)), ("BatchNorm3D", (2, 3, 2, 2, 2)), ("BatchNorm", (2, 3, 2, 2, 2))):
        bn = getattr(paddle.nn, cls)(3)
        a = rng.normal(size=shape).astype(np.float32)
        y = bn(T(paddle, a)).numpy()
        axes = tuple(i for i in range(len(shape)) if i != 1)
        np.testing.assert_allclose(y, (a - a.mean(axes, keepdims=True)) / np.sqrt(a.var(axes, keepdims=True) + 1e-5), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(bn._variance.numpy(), 0.9 + 0.1 * a.var(axes), rtol=1e-5)


def test_conv(paddle):                                                       # L3
    c = paddle.nn.Conv1D(2, 1, 2, 1)
    assert tuple(c.weight.shape) == (1, 2, 2)
    _set(c.weight, [[[1, 10], [100, 1000]]])
    _set(c.bias, [0.5])
    y = c(T(paddle, [[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]])).numpy()
    assert y.tolist() == [[[1 + 20 + 400 + 5000 + 0.5, 2 + 30 + 500 + 6000 + 0.5]]]      # cross-correlation: w[k] meets x[t + k]
    c2 = paddle.nn.Conv2D(3, 4, 1)
    assert tuple(c2.weight.shape) == (4, 3, 1, 1)
    c3 = paddle.nn.Conv3D(1, 2, 5, 2)
    assert tuple(c3.weight.shape) == (2, 1, 5, 5, 5) and tuple(c3(paddle.zeros([1, 1, 32, 32, 32])).shape) == (1, 2, 14, 14, 14)
    d = paddle.nn.Conv1DTranspose(1, 1, 2, 2)
    assert tuple(d.weight.shape) == (1, 1, 2)
    _set(d.weight, [[[1, 10]]])
    assert d(T(paddle, [[[1.0, 2.0]]])).numpy().tolist() == [[[1.0, 10.0, 2.0, 20.0]]]    # out[2 i + t] = x[i] w[t]
    assert paddle.nn.Conv1D(3, 4, 1, 1, padding="same")(paddle.zeros([1, 3, 5])).shape[-1] == 5


def test_activations(paddle):                                                # L4
    x = T(paddle, [-2.0, 0.0, 3.0])
    assert paddle.nn.functional.relu(x).numpy().tolist() == [0.0, 0.0, 3.0] and paddle.nn.ReLU()(x).numpy().tolist() == [0.0, 0.0, 3.0]
    np.testing.assert_allclose(paddle.nn.LeakyReLU()(x).numpy(), [-0.02, 0.0, 3.0], rtol=1e-6)
    np.testing.assert_allclose(paddle.nn.LogSoftmax(axis=-1)(T(paddle, [[0.0, np.log(3.0)]])).numpy(), [[np.log(0.25), np.log(0.75)]], rtol=1e-6)


def test_maxpool(paddle):                                                    # L5
    x = T(paddle, [[[1.0, 5.0, 2.0, 4.0]]])
    assert paddle.nn.MaxPool1D(4)(x).numpy().tolist() == [[[5.0]]] and paddle.nn.MaxPool1D(2)(x).numpy().tolist() == [[[5.0, 4.0]]]
    g = T(paddle, np.arange(64).reshape(1, 1, 4, 4, 4))
    assert paddle.nn.MaxPool3D(2, 2, 0)(g).numpy().reshape(-1).tolist() == [21.0, 23.0, 29.0, 31.0, 53.0, 55.0, 61.0, 63.0]
    assert paddle.nn.MaxPool2D(2)(T(paddle, np.arange(16).reshape(1, 1, 4, 4))).numpy().reshape(-1).tolist() == [5.0, 7.0, 13.0, 15.0]


def test_dropout(paddle):                                                    # L6
    d = paddle.nn.Dropout(0.75)
    x = T(paddle, [[1.0, 2.0, 3.0, 4.0]])
    d.eval()
    assert d(x).numpy().tolist() == [[1.0, 2.0, 3.0, 4.0]]
    d.train()
    paddle.nn.DROPOUT_MASK = None
    with pytest.raises(RuntimeError):
        d(x)
    paddle.nn.DROPOUT_MASK = lambda shape: np.array([[1, 0, 0, 1]])
    try:
        assert d(x).numpy().tolist() == [[4.0, 0.0, 0.0, 16.0]]             # keep / (1 - p)
    finally:
        paddle.nn.DROPOUT_MASK = None


def test_layer_registration(paddle):                                         # L7
    nn = paddle.nn

    class Net(nn.Layer):
        def __init__(self):
            super(Net, self).__init__()
            self.hidden = [nn.Conv2D(3, 4, 1), nn.BatchNorm2D(4)]            # a plain list: registers nothing
            self.seq = nn.Sequential(nn.Conv1D(3, 4, 1), nn.BatchNorm(4), nn.ReLU(), nn.Dropout(0.5))
            self.fc = nn.Linear(4, 2)

        def forward(self, x):
            return self.fc(x)

    net = Net()
    assert list(net.state_dict().keys()) == ["seq.0.weight", "seq.0.bias", "seq.1.weight", "seq.1.bias", "seq.1._mean", "seq.1._variance",
                                             "fc.weight", "fc.bias"]
    assert [n for n, _ in net.named_parameters()] == ["seq.0.weight", "seq.0.bias", "seq.1.weight", "seq.1.bias", "fc.weight", "fc.bias"]
    assert len(net.parameters()) == 6 and all(p.requires_grad for p in net.parameters())
    net.eval()
    assert not net.training and not net.seq[1].training and not net.seq[3].training and net.hidden[1].training     # eval() never reaches the list
    net.train()
    assert net.seq[1].training
    seen = []
    net.fc.register_forward_pre_hook(lambda layer, args: seen.append(tuple(args[0].shape)))
    net(paddle.zeros([5, 4]))
    assert seen == [(5, 4)]

    class Bare(nn.Layer):
        def __init__(self):
            super().__init__()
            self.convs = [nn.Conv2D(3, 4, 1)]

    assert Bare().parameters() == [] and len(Bare().state_dict()) == 0


def test_param_attr_assign(paddle):                                          # L8
    attr = paddle.framework.ParamAttr(initializer=paddle.nn.initializer.Assign(paddle.reshape(paddle.eye(2), [-1])))
    wattr = paddle.framework.ParamAttr(initializer=paddle.nn.initializer.Assign(paddle.ones((3, 4))))
    lin = paddle.nn.Linear(3, 4, weight_attr=wattr, bias_attr=attr)
    assert lin.bias.numpy().tolist() == [1.0, 0.0, 0.0, 1.0] and lin.weight.numpy().tolist() == [[1.0] * 4] * 3
    assert lin.bias.requires_grad and lin.weight.requires_grad


def test_reference_weight_rule():
    """the rule behind the fixtures' weights: a function of (name, shape, seed) alone, Linear fan-in = the [in, out] matrix's first axis"""
    a = reference_weight("fc1.weight", (1024, 512), 7)
    assert a.dtype == np.float32 and a.shape == (1024, 512) and np.array_equal(a, reference_weight("fc1.weight", (1024, 512), 7))
    assert not np.array_equal(a, reference_weight("fc2.weight", (1024, 512), 7)) and not np.array_equal(a, reference_weight("fc1.weight", (1024, 512), 8))
    assert abs(float(a.std()) - np.sqrt(2.0 / 1024)) < 0.02 * np.sqrt(2.0 / 1024)
    c = reference_weight("sa1.mlp_convs.0.weight", (64, 3, 1, 1), 7)
    assert abs(float(c.std()) - np.sqrt(2.0 / 3)) < 0.15 * np.sqrt(2.0 / 3)
    g = reference_weight("bn1.weight", (512,), 7)
    assert (np.abs(g) >= 0.5).all() and (np.abs(g) <= 1.5).all() and 0.1 < (g < 0).mean() < 0.4
    assert float(np.abs(reference_weight("bn1.bias", (512,), 7)).max()) < 0.6


# ---------------------------------------------------------------------------------------------------------------------------------------
# what the tie rule of the pooled max does to the weight gradients of a set-abstraction layer
# ---------------------------------------------------------------------------------------------------------------------------------------
TIE_FRACTION = 0.32          # measured, see the test's docstring
TIE_RATIO = (1.68, 3.89)


def test_tie_rule_changes_sa_weight_gradients(paddle):
    """One set-abstraction layer (npoint 32, radius 0.3, nsample 16, coordinates only, mlp [16, 32]) on a sparse cloud, in float64, in the
    reference's op decomposition (oracle/torch_cpu_reference: dense ball query, padding with the first hit), pooled with the stand-in's
    ``max`` under both tie rules.  Ball-query padding repeats a group's first neighbour (76 % of the slots here), so many pooled maxima are
    EXACT ties between copies of one row.  "first" and "last" (any single winner) give the same weight gradients, which is what DESIGN section 1 relies on; Paddle's
    documented rule for ``max`` ("all": every tied element receives the full gradient) multiplies the tied rows' contribution.
    Measured: 32 % of the pooled entries are ties; max|dW_all - dW_first| / max|dW_first| = 1.68 (layer 0), 3.89 (layer 1).
    The reference never trains these weights (they sit in plain lists, unregistered), so the choice is unobservable there."""
    from oracle import torch_cpu_reference as TR
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_layers.npz"))
    xyz = torch.from_numpy(z["cloud"][:, :256].astype(np.float64) * 3.0)               # 256 points in a cube of side 1.7: ~6 neighbours within 0.3
    start = z["start1"].astype(np.int64) % 256
    with torch.no_grad():
        _, grouped, _, idx = TR.sample_and_group(32, 0.3, 16, xyz, None, start)
    idx = idx.numpy()
    padded = float((idx[:, :, 1:] == idx[:, :, :1]).mean())
    ws = [torch.from_numpy(reference_weight("toy.%d.weight" % i, s, 3).astype(np.float64)) for i, s in enumerate([(16, 3), (32, 16)])]

    def grads(rule, flip=False):
        paddle.TIE_RULE = rule
        w = [t.clone().requires_grad_(True) for t in ws]
        x = grouped.permute(0, 3, 2, 1)                                                  # [B, C, K, S]
        if flip:
            x = x.flip(2)                                                                # "first" on the reversed neighbour axis = "last"
        for wi in w:
            x = sum(wi[:, c].view(1, -1, 1, 1) * x[:, c:c + 1] for c in range(wi.shape[1]))      # (term by term: no BLAS kernel choice in it)
            mean = x.mean(dim=(0, 2, 3), keepdim=True)
            var = ((x - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
            x = torch.relu((x - mean) / torch.sqrt(var + 1e-5))
        pooled = paddle.max(x.as_subclass(paddle.Tensor), 2)
        ties = float(((x == x.amax(2, keepdim=True)).sum(2) > 1).double().mean())
        pooled.sum().backward()
        return [t.grad.clone() for t in w], ties

    try:
        g_first, ties = grads("first")
        g_last, _ = grads("first", flip=True)
        g_all, _ = grads("all")
    finally:
        paddle.TIE_RULE = "all"
    ratios = [float((a - f).abs().max() / f.abs().max()) for a, f in zip(g_all, g_first)]
    single = [float((l - f).abs().max() / f.abs().max()) for l, f in zip(g_last, g_first)]
    print("padded slots %.2f, tied pooled entries %.2f, all-vs-first %s, last-vs-first %s" % (padded, ties, ratios, single))
    assert max(single) < 1e-12                                   # between single winners the parameter gradients do not depend on the rule
    assert abs(ties - TIE_FRACTION) < 0.02
    # (with the 1x1 convolutions written as one einsum, a BLAS call, the layer-0 figure was 1.68 on one host's CPU and 1.35 on another's;
    # term by term, as above, two different hosts give 1.675466857973312 and 3.889434068670008 to the last digit)
    for r, want in zip(ratios, TIE_RATIO):
        assert abs(r - want) < 0.06 * want, (ratios, TIE_RATIO)
