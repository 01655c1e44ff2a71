"""Host check of the caller-allocated workspaces of the kd-tree BatchNorm level, the two cloud-concat convs and the detection loss: every
papc_*_workspace() query returns the byte count recorded here.  An entry point carves its buffer by the same layout function the query sizes
it with (csrc/carve.h: WsCarver), so a size that moves means pieces that move.  The numbers were recorded from a build of the commit before
the layouts were written once; they are literals on purpose -- a formula here would be a third copy of the rule.  papc_nms_workspace and
papc_points_to_voxel_workspace are absent: their last piece is rocPRIM's temporary storage, and the size rocPRIM asks for depends on the
device the process sees (without one the query answers with other numbers than on an MI355X)."""
import ctypes

import pytest

from papc_amd import _lib
from papc_amd.detloss import DetLossDesc

# (B, dim, Cin, F) -> (papc_kdbn_fwd_workspace, papc_kdbn_bwd_workspace): every level shape of tests/test_gpu_kdunet.py at B = 16 and 19, its
# dim = 2 case, the smallest shape with more than one slice of the backward's A (the optional last region), the smallest legal shape, and a
# refused width
KDBN = {
    (16, 1024, 3, 32): (3120, 126016),
    (19, 1024, 3, 32): (3696, 149056),
    (16, 64, 32, 64): (20992, 241536),
    (19, 64, 32, 64): (25216, 293760),
    (16, 16, 64, 256): (33024, 733952),
    (19, 16, 64, 256): (49664, 936704),
    (16, 8, 256, 512): (525312, 6609920),
    (19, 8, 256, 512): (525312, 8195072),
    (16, 4, 512, 1024): (2099200, 22124544),
    (19, 4, 512, 1024): (2099200, 22124544),
    (33, 2, 512, 1024): (2099200, 22124544),
    (1, 64, 32, 96): (8320, 94464),
    (1, 2, 3, 32): (112, 5056),
    (16, 64, 48, 64): (0, 0),
}

# (B, N, Cp, Cg, Cout) -> papc_cloud_concat_conv_bwd_workspace (the cases of tests/test_pointnet_seg_host.py)
CONCAT = {
    (32, 1024, 64, 1024, 512): 34144256,
    (2, 1000, 64, 64, 512): 2134016,
    (32, 1024, 64, 96, 512): 0,
}

# (B, N, Cp, Cg, Cout) -> papc_cloud_concat_k_bwd_workspace (the cases of tests/test_vfe_host.py and one refused width)
CONCAT_K = {
    (64, 1024, 256, 1280, 512): 102498304,
    (32, 1024, 256, 256, 64): 37904384,
    (3, 200, 64, 64, 128): 290816,
    (1, 64, 192, 2304, 64): 148224,
    (2, 1000, 256, 1280, 512): 6819840,
    (32, 1024, 320, 256, 64): 0,
}

# (B, A) -> papc_det_loss_workspace: around the 256 anchors of a main-pass workgroup, and several clouds
DETLOSS = {
    (1, 1): 272,
    (1, 255): 272,
    (1, 256): 272,
    (1, 257): 272,
    (3, 1000): 560,
}


@pytest.mark.parametrize("shape", sorted(KDBN))
def test_kdbn_workspaces(shape):
    L = _lib.load()
    assert (L.papc_kdbn_fwd_workspace(*shape), L.papc_kdbn_bwd_workspace(*shape)) == KDBN[shape]


def test_concat_workspaces():
    L = _lib.load()
    for shape, nb in CONCAT.items():
        assert L.papc_cloud_concat_conv_bwd_workspace(*shape) == nb, shape
    for shape, nb in CONCAT_K.items():
        assert L.papc_cloud_concat_k_bwd_workspace(*shape) == nb, shape


def test_det_loss_workspace():
    L = _lib.load()
    for (B, A), want in DETLOSS.items():
        d = DetLossDesc()
        d.B, d.A, d.C, d.code_size, d.norm_type, d.has_dir = B, A, 1, 7, 1, 1
        d.encode_background_as_zeros, d.codewise, d.sigma, d.gamma = 1, 1, 3.0, 2.0
        n = ctypes.c_int64(0)
        assert L.papc_det_loss_workspace(ctypes.byref(d), ctypes.byref(n)) == 0
        assert n.value == want, (B, A)
