"""CPU checks of the VFE models (papc_amd.models.VFE_Clas, classify/vfe/vfe.py:5-86, and VFE_Seg, segment/vfe/vfe.py:5-97): checkpoint names
and layouts against the recorded reference state (tests/golden/ref_model_vfe_*.npz), the .pdparams round trip, the K-looped concat-conv
entry points of the C ABI (csrc/cloud_concat_k.hip), the error paths and the loader's batches."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from papc_amd import _lib
from papc_amd import checkpoint as C
from papc_amd.models import VFE_Clas, VFE_Seg
from tests.ref_fixtures import gold, shapes_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("papc_cloud_concat_k_ok", "papc_cloud_concat_k_parts", "papc_cloud_concat_k_f32", "papc_cloud_concat_k_bwd_workspace",
       "papc_cloud_concat_k_bwd_f32")


@pytest.mark.parametrize("name,make", [("vfe_clas", VFE_Clas), ("vfe_seg", VFE_Seg)])
def test_export_names_and_layouts_match_the_recorded_reference_state(name, make):
    z = gold("ref_model_" + name)
    m = make()
    st = C.export_state(m)
    keys = [str(s) for s in z["state_keys"]]
    assert sorted(st) == sorted(keys)
    if name == "vfe_clas":
        assert len(keys) == 66
    for k, s in zip(keys, shapes_of(z, "state_shapes")):
        assert tuple(st[k].shape) == s, (k, st[k].shape, s)
    assert sorted(C._to_reference_name(n, m) for n, _ in m.named_parameters()) == sorted(str(s) for s in z["param_names"])
    assert st["vfe.pointnet_2.mlp_1.0._conv.weight"].shape == (64, 512, 1)
    assert st["fc.0.weight" if name == "vfe_clas" else "seg_net.12.weight"].shape == ((1024, 512) if name == "vfe_clas" else (50, 128, 1))


def test_seg_net_width_follows_max_points():
    assert C.export_state(VFE_Seg())["seg_net.0.weight"].shape == (512, 1536, 1)
    st = C.export_state(VFE_Seg(256, 13, 128))
    assert st["seg_net.0.weight"].shape == (512, 640, 1) and st["seg_net.12.bias"].shape == (13,)
    assert st["vfe.pointnet_2.mlp_2.2._conv.weight"].shape == (128, 128, 1)
    st = C.export_state(VFE_Clas(10, 128))
    assert st["fc.0.weight"].shape == (128, 512) and st["fc.5.weight"].shape == (256, 10)       # Linear as [in, out]
    assert VFE_Clas().max_points == 1024 and VFE_Seg().max_points == 1024


@pytest.mark.parametrize("cls", [VFE_Clas, VFE_Seg])
def test_pdparams_round_trip_is_bit_equal(tmp_path, cls):
    torch.manual_seed(2)
    m = cls(max_points=128)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.uniform_(-1, 1)
                mod.running_var.uniform_(0.5, 2)
    path = str(tmp_path / "vfe.pdparams")
    with open(path, "wb") as f:
        pickle.dump(dict(C.export_state(m), **{"StructuredToParameterName@@": {}}), f, protocol=2)
    m2 = cls(max_points=128)
    missing, unexpected = C.import_state(m2, C.load_pdparams(path), strict=True)
    assert not missing and not unexpected
    for (k, a), (k2, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(a, b), k


def test_concat_k_entry_points_in_header_binding_and_library():
    hdr = open(os.path.join(ROOT, "include", "papc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in NEW:
        assert s + "(" in hdr, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    L = _lib.load()
    assert L.papc_abi_version() == 8
    for cp, cg, cout, ok in ((256, 256, 64, 1), (256, 1280, 512, 1), (64, 64, 128, 1), (192, 2304, 64, 1), (320, 256, 64, 0), (32, 256, 64, 0),
                             (256, 256, 576, 0), (256, 96, 64, 0), (256, 2368, 64, 0), (256, 256, 96, 0)):
        assert L.papc_cloud_concat_k_ok(cp, cg, cout) == ok, (cp, cg, cout)
    assert L.papc_cloud_concat_k_parts(32, 1024) == 256 and L.papc_cloud_concat_k_parts(3, 200) == 5 and L.papc_cloud_concat_k_parts(0, 8) == 0


def _ws(B, N, cp, cout):
    """W_p^T, the dW_p range partials (at most 64 ranges of whole multiples of 64 rows, at least 256), the column-sum partials per 128-row
    segment of a cloud, s and the dense dX"""
    M = B * N
    rows = max(256, (-(-M // 64) + 63) // 64 * 64)
    ranges = -(-M // rows)
    return 4 * (cp * cout + ranges * (cout * cp + cout) + B * (-(-N // 128)) * cout + B * cout + M * cp)


def test_concat_k_workspace_formula_and_bound():
    L = _lib.load()
    for B, N, cp, cg, cout in ((64, 1024, 256, 1280, 512), (32, 1024, 256, 256, 64), (3, 200, 64, 64, 128), (1, 64, 192, 2304, 64), (2, 1000, 256, 1280, 512)):
        assert L.papc_cloud_concat_k_bwd_workspace(B, N, cp, cg, cout) == _ws(B, N, cp, cout), (B, N, cp, cg, cout)
    # bounded row ranges: the workspace of the segmenter's layer at B = 64 is no larger than the layer's own y
    assert L.papc_cloud_concat_k_bwd_workspace(64, 1024, 256, 1280, 512) <= 64 * 1024 * 512 * 4
    for cp, cg, cout in ((320, 256, 64), (32, 256, 64), (256, 256, 576), (256, 96, 64), (256, 2368, 64)):
        assert L.papc_cloud_concat_k_bwd_workspace(32, 1024, cp, cg, cout) == 0


def test_concat_k_rejects_on_the_host():
    L = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    fwd = lambda cp, cg, cout, x=p: L.papc_cloud_concat_k_f32(x, 256, p, p, None, 1, 8, cp, cg, cout, p, p, None, None)          # noqa: E731
    bwd = lambda cp, cg, cout, nb=1 << 30, x=p: L.papc_cloud_concat_k_bwd_f32(p, p, p, p, p, p, p, p, x, 256, p, p, 1, 8, cp, cg, cout, p, cp, 0, p,   # noqa: E731
                                                                             p, p, None, p, nb, None)
    for cp, cg, cout, what in ((320, 256, 64, b"Cp=320"), (32, 256, 64, b"Cp=32"), (256, 256, 576, b"Cout=576"), (256, 96, 64, b"Cg=96"),
                               (256, 2368, 64, b"Cg=2368")):
        assert fwd(cp, cg, cout) == -2
        assert what in L.papc_last_error_string()
        assert bwd(cp, cg, cout) == -2
        assert what in L.papc_last_error_string()
    assert fwd(256, 256, 64, x=None) == -1 and b"null" in L.papc_last_error_string()
    assert bwd(256, 256, 64, x=None) == -1 and b"null" in L.papc_last_error_string()
    assert bwd(256, 256, 64, nb=16) == -1
    assert b"workspace" in L.papc_last_error_string()
    # the Cp = 64 entry keeps refusing the wide layer
    assert L.papc_cloud_concat_conv_f32(p, 256, p, p, None, 1, 8, 256, 256, 512, p, p, None, None) != 0
    assert b"Cp=256" in L.papc_last_error_string()


def test_cpu_tensors_raise():
    from papc_amd.vfe import concat_k_bn_relu
    for m in (VFE_Clas(16, 64), VFE_Seg(256, 50, 64)):
        with pytest.raises(_lib.PapcError):
            m(torch.zeros(2, 3, 64))
    with pytest.raises(_lib.PapcError):
        VFE_Seg(256, 50, 64)([torch.zeros(2, 3, 64).numpy(), None])          # a loader batch for a model whose parameters sit on the CPU
    with pytest.raises(_lib.PapcError):
        VFE_Clas(16, 64)(torch.zeros(2, 3, 64).numpy())
    blk = VFE_Clas(16, 64).vfe.pointnet_2.mlp_1[0]
    with pytest.raises(_lib.PapcError):
        concat_k_bn_relu(torch.zeros(2 * 8, 256), torch.zeros(2, 256), blk._conv, blk._batch_norm, 8, True)


@pytest.mark.parametrize("mode1", ["clas", "seg"])
def test_vfe_loader_batches_have_the_models_shapes(mode1):
    from papc_amd.datasets import DataLoader
    N = 64
    rng = np.random.default_rng(21)

    def opener(path):           # a small synthetic file (the loader's h5 keys)
        return {"data": rng.normal(size=(5, 80, 3)).astype(np.float32), "label": rng.integers(0, 16, size=(5, 1)),
                "pid": rng.integers(0, 50, size=(5, 80))}
    gen = DataLoader("vfe", N, 4, path="data", mode1=mode1, mode2="test", opener=opener)
    batch, target = next(iter(gen()))
    data = batch[0] if mode1 == "seg" else batch
    assert data.shape == (4, 3, N) and data.dtype == np.float32             # what VFE_Clas(max_points=N) / VFE_Seg(max_points=N) take
    assert target.shape == ((4, N, 1) if mode1 == "seg" else (4, 1))
