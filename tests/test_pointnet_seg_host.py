"""CPU checks of the PointNet part segmenters (papc_amd.models.PointNet_Seg, segment/pointnet/pointnet.py:4-114, and PointNet_Basic_Seg,
segment/pointnet_base/pointnet_base.py:4-80): checkpoint names and layouts, the identity start of the input T-Net, the .pdparams round trip,
and the concat-conv entry points of the C ABI."""
import ctypes
import os
import pickle

import pytest
import torch

from papc_amd import _lib
from papc_amd import checkpoint as C
from papc_amd.models import PointNet_Basic_Seg, PointNet_Seg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _convs(names, seq, conv_idx):
    for i in conv_idx:
        names.extend(["%s.%d.weight" % (seq, i), "%s.%d.bias" % (seq, i)])
        names.extend(["%s.%d.%s" % (seq, i + 1, s) for s in ("weight", "bias", "_mean", "_variance")])


def _linears(names, seq, idx):
    for i in idx:
        names.extend(["%s.%d.weight" % (seq, i), "%s.%d.bias" % (seq, i)])


def _seg_net_names(names):
    _convs(names, "seg_net", (0, 3, 6, 9))          # pointnet.py:69-80 / pointnet_base.py:9-20
    names.extend(["seg_net.12.weight", "seg_net.12.bias"])   # :81 / :21, Conv1D(128, num_classes, 1)


def _reference_names_pointnet():
    """state_dict keys of the source's PointNet_Seg, read off segment/pointnet/pointnet.py:8-83"""
    names = []
    _convs(names, "input_transform_net", (0, 3, 6))        # :8-20
    _linears(names, "input_fc", (0, 2, 4))                 # :21-30
    _convs(names, "mlp_1", (0, 3))                         # :31-38
    _convs(names, "feature_transform_net", (0, 3, 6))      # :39-51
    _linears(names, "feature_fc", (0, 2, 4))               # :52-58
    _convs(names, "mlp_2", (0, 3, 6))                      # :59-68
    _seg_net_names(names)
    return names


def _reference_names_basic():
    """state_dict keys of the source's PointNet_Basic_Seg, read off segment/pointnet_base/pointnet_base.py:7-22, :44-62"""
    names = []
    _convs(names, "pointnet_bacic.mlp_1", (0, 3))          # :44-51
    _convs(names, "pointnet_bacic.mlp_2", (0, 3, 6))       # :52-62
    _seg_net_names(names)
    return names


def test_export_names_and_layouts_match_the_reference():
    st = C.export_state(PointNet_Seg(50, 2048))
    assert sorted(st) == sorted(_reference_names_pointnet())
    assert st["seg_net.0.weight"].shape == (512, 1088, 1) and st["seg_net.12.weight"].shape == (50, 128, 1)   # Conv1D weights as they are
    assert st["input_fc.4.weight"].shape == (256, 9) and st["feature_fc.4.weight"].shape == (256, 4096)       # Linear as [in, out]
    assert st["seg_net.1._variance"].shape == (512,) and st["seg_net.10._mean"].shape == (128,)
    st = C.export_state(PointNet_Basic_Seg(50, 1024))
    assert sorted(st) == sorted(_reference_names_basic())
    assert st["pointnet_bacic.mlp_2.6.weight"].shape == (1024, 128, 1) and st["seg_net.0.weight"].shape == (512, 1024 + 64, 1)
    assert st["seg_net.12.weight"].shape == (50, 128, 1)
    st = C.export_state(PointNet_Basic_Seg(13, 512))
    assert st["seg_net.0.weight"].shape == (512, 576, 1) and st["seg_net.12.bias"].shape == (13,)


def test_input_tnet_starts_at_the_identity():
    m = PointNet_Seg(50, 2048)
    assert float(m.input_fc[4].weight.detach().abs().max()) == 0.0
    assert torch.equal(m.input_fc[4].bias.detach(), torch.eye(3).reshape(-1))
    assert m.max_point == 2048 and PointNet_Basic_Seg().max_points == 1024
    assert m.seg_net[1].eps == 1e-5


@pytest.mark.parametrize("cls", [PointNet_Seg, PointNet_Basic_Seg])
def test_pdparams_round_trip_is_bit_equal(tmp_path, cls):
    torch.manual_seed(2)
    m = cls(50, 1024)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.uniform_(-1, 1)
                mod.running_var.uniform_(0.5, 2)
    path = str(tmp_path / "seg.pdparams")
    with open(path, "wb") as f:
        pickle.dump(dict(C.export_state(m), **{"StructuredToParameterName@@": {}}), f, protocol=2)
    m2 = cls(50, 1024)
    missing, unexpected = C.import_state(m2, C.load_pdparams(path), strict=True)
    assert not missing and not unexpected
    for (k, a), (k2, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(a, b), k


def test_concat_entry_points_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "papc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("papc_cloud_concat_conv_f32", "papc_cloud_concat_conv_bwd_f32", "papc_cloud_concat_conv_bwd_workspace", "papc_cloud_concat_conv_parts"):
        assert s + "(" in hdr, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    L = _lib.load()
    assert L.papc_abi_version() == 8
    assert L.papc_cloud_concat_conv_parts(32, 1024) == 256 and L.papc_cloud_concat_conv_parts(33, 1000) == (33000 + 127) // 128
    # per chunk of 128 rows of a cloud: a [512, 64] dW_p partial and 512 column sums; plus s [B, 512]
    assert L.papc_cloud_concat_conv_bwd_workspace(32, 1024, 64, 1024, 512) == (32 * 8 * (512 * 64 + 512) + 32 * 512) * 4
    assert L.papc_cloud_concat_conv_bwd_workspace(2, 1000, 64, 64, 512) == (2 * 8 * (512 * 64 + 512) + 2 * 512) * 4
    assert L.papc_cloud_concat_conv_bwd_workspace(32, 1024, 64, 96, 512) == 0
    # validation on the host, before any launch
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    assert L.papc_cloud_concat_conv_f32(None, 64, p, p, None, 1, 8, 64, 64, 512, p, p, None, None) == -1
    for cp, cg, cout, what in ((64, 96, 512, b"Cg=96"), (64, 2048, 512, b"Cg=2048"), (32, 64, 512, b"Cp=32"), (64, 64, 256, b"Cout=256")):
        assert L.papc_cloud_concat_conv_f32(p, 64, p, p, None, 1, 8, cp, cg, cout, p, p, None, None) != 0
        assert what in L.papc_last_error_string()
        assert L.papc_cloud_concat_conv_bwd_f32(p, p, p, p, p, p, p, p, p, 64, p, p, 1, 8, cp, cg, cout, p, 64, 0, p, p, p, None, p, 1 << 30, None) != 0
        assert what in L.papc_last_error_string()
    assert L.papc_cloud_concat_conv_bwd_f32(p, p, p, p, p, p, p, p, p, 64, p, p, 1, 8, 64, 64, 512, p, 64, 0, p, p, p, None, p, 16, None) == -1
    assert b"workspace" in L.papc_last_error_string()


def test_cpu_tensors_raise():
    from papc_amd.segment import cloud_concat_bn_relu
    for m in (PointNet_Seg(50, 64), PointNet_Basic_Seg(50, 64)):
        with pytest.raises(_lib.PapcError):
            m(torch.zeros(2, 3, 64))
        with pytest.raises(_lib.PapcError):
            m([torch.zeros(2, 3, 64).numpy(), None])          # a loader batch for a model whose parameters sit on the CPU
    seg = PointNet_Seg(50, 64).seg_net
    with pytest.raises(_lib.PapcError):
        cloud_concat_bn_relu(torch.zeros(2 * 8, 64), torch.zeros(2, 1024), seg[0], seg[1], 8, True)
