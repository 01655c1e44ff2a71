"""Host tests of papc_amd.rpn.RPN: the module tree and state-dict keys against the list derived from the reference's rpn.py, the output shapes and
[B, H, W, .] order, the second path (torch ops, the one CPU tensors take) against the float64 restatement tests/rpn_ref.py -- forward, parameter
gradients, input gradient, running statistics --, the .pdparams round trip and the configurations that are not built."""
import numpy as np
import pytest
import torch

from papc_amd import _lib, checkpoint
from papc_amd.rpn import RPN
from tests import rpn_ref as R
from tests.util import assert_close

TIGHT = 1e-11        # float64 against float64: two orders of summation of at most 9 * 64 + 96 terms, ~1e-14 each
KITTI = dict(use_norm=True, num_class=1, layer_nums=[3, 5, 5], layer_strides=[2, 2, 2], num_filters=[64, 128, 256], upsample_strides=[1, 2, 4],
             num_upsample_filters=[128, 128, 128], num_input_filters=64, num_anchor_per_loc=2, encode_background_as_zeros=True,
             use_direction_classifier=True, box_code_size=7)
SMALL = dict(num_input_filters=32, num_filters=[32, 32, 64], layer_nums=[1, 2, 1], num_upsample_filters=[32, 64, 32], num_class=1)


def _np(t):
    return t.detach().double().cpu().numpy()


@pytest.mark.parametrize("kw", [{}, KITTI, dict(KITTI, use_norm=False)], ids=["default", "kitti", "kitti-no-norm"])
def test_state_dict_keys_and_shapes(kw):
    m = RPN(**kw)
    want = R.expected_state(**kw)
    got = {k: tuple(v.shape) for k, v in checkpoint.export_state(m).items()}
    assert sorted(got) == sorted(want)
    assert got == want
    # the source's tree: the pad layer sits at index 0 of every block
    own = [k for k in m.state_dict() if not k.endswith("num_batches_tracked")]
    assert "block1.1.weight" in own and "block1.4.weight" in own and "deconv1.0.weight" in own and not any(k.startswith("block1.0") for k in own)
    if kw.get("use_norm", True):
        assert "block1.2.running_mean" in own and "block1.1.bias" not in own
        bn = m.block1[2]
        assert bn.eps == 1e-3 and abs(bn.momentum - 0.99) < 1e-12         # torch weighs the batch value: 1 - paddle's 0.01


def _small(seed=3):
    m = RPN(**SMALL).double().train()
    P = R.seeded_params(m, seed)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(P[k])
    return m, P


def test_second_path_vs_f64_reference():
    B, H, W = 2, 16, 24
    m, P64 = _small()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, 32, H, W, generator=g, dtype=torch.float64)
    xg = x.clone().requires_grad_(True)
    out = m(xg)
    assert list(out) == ["box_preds", "cls_preds", "dir_cls_preds"]
    assert out["box_preds"].shape == (B, H // 2, W // 2, 14) and out["cls_preds"].shape == (B, H // 2, W // 2, 2)
    assert out["dir_cls_preds"].shape == (B, H // 2, W // 2, 4)
    P = {k: v.clone().requires_grad_(True) for k, v in P64.items()}
    xr = x.clone().requires_grad_(True)
    ref, aux = R.forward(P, xr, SMALL["layer_nums"], [2, 2, 2], [1, 2, 4])
    gouts = {k: torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in ref.items()}
    for k in ref:
        assert_close(_np(out[k]), _np(ref[k]), TIGHT, k)                 # (the [B, H, W, .] order: the reference permutes NCHW)
    sum((out[k] * gouts[k]).sum() for k in ref).backward()
    sum((ref[k] * gouts[k]).sum() for k in ref).backward()
    assert_close(_np(xg.grad), _np(xr.grad), TIGHT, "d canvas")
    for k, p in m.named_parameters():
        assert_close(_np(p.grad), _np(P[k].grad), 1e-9, "d " + k)
    for _, nname, _, _, _ in R.layer_names(SMALL["layer_nums"]):
        c = P64[nname + ".weight"].shape[0]
        rm, rv = R.running(aux, nname, torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64))
        sd = m.state_dict()
        assert_close(_np(sd[nname + ".running_mean"]), _np(rm), TIGHT, nname + " running mean")
        assert_close(_np(sd[nname + ".running_var"]), _np(rv), TIGHT, nname + " running var (biased, 0.01 on the running value)")
    # eval mode: the running statistics, nothing updated
    m.eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ev = m(x)
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in before.items())
    stats = {n[1]: (before[n[1] + ".running_mean"], before[n[1] + ".running_var"]) for n in R.layer_names(SMALL["layer_nums"])}
    ref_ev, _ = R.forward(P64, x, SMALL["layer_nums"], [2, 2, 2], [1, 2, 4], stats=stats)
    for k in ref_ev:
        assert_close(_np(ev[k]), _np(ref_ev[k]), TIGHT, "eval " + k)


def test_no_norm_and_no_direction_classifier():
    m = RPN(use_norm=False, use_direction_classifier=False, **SMALL).double()
    out = m(torch.randn(1, 32, 8, 8, dtype=torch.float64))
    assert list(out) == ["box_preds", "cls_preds"] and out["box_preds"].shape == (1, 4, 4, 14)
    # against torch's own modules: the tree is a plain nn.Sequential stack
    x = torch.randn(1, 32, 8, 8, dtype=torch.float64)
    a1 = m.block1(x)
    a2 = m.block2(a1)
    a3 = m.block3(a2)
    cat = torch.cat([m.deconv1(a1), m.deconv2(a2), m.deconv3(a3)], 1)
    assert_close(_np(m(x)["box_preds"]), _np(m.conv_box(cat).permute(0, 2, 3, 1)), TIGHT, "use_norm=False box_preds against the module tree itself")


def test_pdparams_round_trip(tmp_path):
    a, _ = _small(5)
    path = str(tmp_path / "rpn.pdparams")
    checkpoint.save_pdparams(a, path)
    state = checkpoint.load_pdparams(path)
    assert "block1.2._mean" in state and "block1.2._variance" in state and "deconv3.0.weight" in state
    assert state["deconv2.0.weight"].shape == (32, 64, 2, 2)             # [Ci, Co, s, s]: a plain copy
    b = RPN(**SMALL).double()
    missing, unexpected = checkpoint.import_state(b, state, strict=True)
    assert not missing and not unexpected
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(va, vb), k


def test_unbuilt_configurations_raise():
    with pytest.raises(_lib.PapcError, match="not built"):
        RPN(use_bev=True)
    with pytest.raises(_lib.PapcError, match="not built"):
        RPN(use_groupnorm=True)
    with pytest.raises(_lib.PapcError, match="input channels"):
        RPN(**SMALL)(torch.zeros(1, 16, 8, 8))
    with pytest.raises(_lib.PapcError, match="differ in size"):
        RPN(**SMALL)(torch.zeros(1, 32, 9, 8))                           # 9 -> 5 -> 3 -> 2: 5, 6 and 8 rows
