"""CPU checks of the T-Net PointNet classifier (papc_amd.models.PointNet_Clas, pointnet_Conv1D.py:4-104): checkpoint names and layouts,
the identity start of the input T-Net, the .pdparams round trip, and the new entry points of the C ABI."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from papc_amd import _lib
from papc_amd import checkpoint as C
from papc_amd.models import PointNet_Clas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_names():
    """The state_dict keys of the source's PointNet_Clas, read off pointnet_Conv1D.py:7-75: nn.Sequential indices, Conv1D / Linear
    weight + bias, BatchNorm weight + bias + _mean + _variance (ReLU / MaxPool1D / Dropout hold nothing)."""
    names = []

    def convs(seq, conv_idx):
        for i in conv_idx:
            names.extend(["%s.%d.weight" % (seq, i), "%s.%d.bias" % (seq, i)])
            names.extend(["%s.%d.%s" % (seq, i + 1, s) for s in ("weight", "bias", "_mean", "_variance")])

    def linears(seq, idx):
        for i in idx:
            names.extend(["%s.%d.weight" % (seq, i), "%s.%d.bias" % (seq, i)])

    convs("input_transform_net", (0, 3, 6))        # :7-18
    linears("input_fc", (0, 2, 4))                 # :19-28
    convs("mlp_1", (0, 3))                         # :29-36
    convs("feature_transform_net", (0, 3, 6))      # :37-49
    linears("feature_fc", (0, 2, 4))               # :50-56
    convs("mlp_2", (0, 3, 6))                      # :57-66
    linears("fc", (0, 2, 5))                       # :68-75
    return names


def test_export_names_and_layouts_match_the_reference():
    st = C.export_state(PointNet_Clas(16, 1024))
    assert sorted(st) == sorted(_reference_names())
    assert st["input_fc.0.weight"].shape == (1024, 512) and st["input_fc.4.weight"].shape == (256, 9)       # Linear as [in, out]
    assert st["feature_fc.4.weight"].shape == (256, 4096) and st["fc.5.weight"].shape == (256, 16)
    assert st["mlp_1.0.weight"].shape[:2] == (64, 3) and st["feature_transform_net.6.weight"].shape[:2] == (1024, 128)
    assert st["mlp_2.7._variance"].shape == (1024,)


def test_input_tnet_starts_at_the_identity():
    m = PointNet_Clas(16, 1024)
    assert float(m.input_fc[4].weight.detach().abs().max()) == 0.0
    assert torch.equal(m.input_fc[4].bias.detach(), torch.eye(3).reshape(-1))
    assert float(m.feature_fc[4].weight.detach().abs().max()) > 0          # feature_fc: the default initialisation (:56)
    bn = m.mlp_2[7]
    assert bn.eps == 1e-5


def test_pdparams_round_trip_is_bit_equal(tmp_path):
    torch.manual_seed(2)
    m = PointNet_Clas(16, 1024)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.uniform_(-1, 1)
                mod.running_var.uniform_(0.5, 2)
    path = str(tmp_path / "pointnet.pdparams")
    with open(path, "wb") as f:
        pickle.dump(dict(C.export_state(m), **{"StructuredToParameterName@@": {}}), f, protocol=2)
    m2 = PointNet_Clas(16, 1024)
    missing, unexpected = C.import_state(m2, C.load_pdparams(path), strict=True)
    assert not missing and not unexpected
    for (k, a), (k2, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(a, b), k


def test_transform_entry_points_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "papc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("papc_cloud_transform_f32", "papc_cloud_transform_bwd_f32", "papc_cloud_transform_bwd_workspace"):
        assert s + "(" in hdr, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    L = _lib.load()
    assert L.papc_cloud_transform_bwd_workspace(32, 1024, 64) == 32 * 16 * 64 * 64 * 4    # chunks of 64 rows
    assert L.papc_cloud_transform_bwd_workspace(32, 1000, 3) == 32 * 4 * 9 * 4             # chunks of 256 rows
    assert L.papc_cloud_transform_bwd_workspace(32, 1024, 5) == 0
    # validation on the host, before any launch
    assert L.papc_cloud_transform_f32(None, 0, 0, 0, None, 0, 1, 1, 64, None, None) == -1
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert L.papc_cloud_transform_f32(p, 0, 0, 0, p, 25, 1, 1, 5, p, None) != 0
    assert b"C=5" in L.papc_last_error_string()
    assert L.papc_cloud_transform_bwd_f32(p, 0, 0, 0, p, 9, p, 1, 1, 3, None, 0, 0, 0, 0, p, p, 0, None) == -1   # workspace too small
    assert b"workspace" in L.papc_last_error_string()


def test_cpu_tensors_raise():
    from papc_amd.transform import transform_points, transform_rows
    m = PointNet_Clas(16, 64)
    with pytest.raises(_lib.PapcError):
        m(torch.zeros(2, 3, 64))
    with pytest.raises(_lib.PapcError):
        transform_points(torch.zeros(2, 3, 8), torch.zeros(2, 3, 3))
    with pytest.raises(_lib.PapcError):
        transform_rows(torch.zeros(16, 64), torch.zeros(2, 64, 64), 8)
    assert np.isfinite(C.export_state(m)["fc.5.bias"]).all()
