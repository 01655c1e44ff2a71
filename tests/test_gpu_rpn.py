"""GPU tests of papc_amd.rpn.RPN and papc_amd.detector.PointPillars: the model against the float64 restatement (tests/rpn_ref.py) with the kernels'
ReLU signs pinned -- the three maps, every parameter gradient, the canvas gradient, the running statistics -- on a randn canvas and on a
scatter-like sparse one, agreement with the torch-op path (PAPC_RPN=0), bit-reproducible and graph-replayable train steps, no foreign GEMM or
convolution in a step, eval mode, the in-place gradient path, the error paths, and one chain from raw pillars to the loss and to predict()."""
import copy

import numpy as np
import pytest
import torch

from papc_amd import _lib, rpn
from papc_amd.rpn import RPN
from tests import rpn_ref as R
from tests.util import assert_close

pytestmark = pytest.mark.gpu
BAR = 2e-4          # the project's model-level bar (as tests/test_gpu_voxnet.py, tests/test_gpu_kdnet.py)
CFG = dict(num_input_filters=64, num_filters=[64, 128, 256], layer_nums=[1, 2, 1], num_upsample_filters=[128, 128, 128], num_class=1)
STRIDES, UPS = [2, 2, 2], [1, 2, 4]
B, H, W = 2, 32, 48           # block 3 still has 2 * 4 * 6 = 48 samples per channel


def _np(t):
    return t.detach().double().cpu().numpy()


def _seeded(dev, seed):
    m = RPN(**CFG).to(dev).train()
    P64 = R.seeded_params(m, seed)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(P64[k].float())
    return m, P64


def _canvas(kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 64, H, W, generator=g, dtype=torch.float64).float()
    if kind == "sparse":                        # the scatter's real output: zero except the pillars' pixels
        keep = torch.rand(B, 1, H, W, generator=g) < 0.1
        x = x * keep
        assert 0.05 < float(keep.float().mean()) < 0.15
    return x


def _recording(monkeypatch, m):
    rec = {}
    inner = m.backbone_rows

    def wrap(x):
        rec["rows"] = inner(x)
        return rec["rows"]
    monkeypatch.setattr(m, "backbone_rows", wrap)
    return rec


def _kernel_signs(node, m):
    """per norm layer, in the node's order: scale * y + shift > 0 of the kernels' own stored rows and constants, in float64, as NCHW"""
    layers, _ = m._layers()
    n, nconv = len(layers), len(layers) - 3
    saved = node.saved_tensors
    ycat, cstup = saved[1], saved[2]
    ys, csts = saved[3:3 + nconv], saved[3 + nconv:3 + 2 * nconv]
    assert len(saved) == 3 + 2 * nconv + n                                                        # canvas rows, concat y, its constants, y and constants per conv, wt per layer
    signs, hw = [], (H, W)
    for i in range(nconv):
        hw = ((hw[0] - 1) // layers[i].stride + 1, (hw[1] - 1) // layers[i].stride + 1)
        s = (csts[i][2].double() * ys[i].double() + csts[i][3].double()) > 0
        signs.append(s.view(B, hw[0], hw[1], -1).permute(0, 3, 1, 2).cpu())
    s = ((cstup[2].double() * ycat.double() + cstup[3].double()) > 0).view(B, H // 2, W // 2, -1).permute(0, 3, 1, 2).cpu()
    c0 = 0
    for l in layers[nconv:]:
        signs.append(s[:, c0:c0 + l.cout])
        c0 += l.cout
    return signs


@pytest.mark.parametrize("kind", ["randn", "sparse"])
def test_model_vs_f64(dev, monkeypatch, kind):
    monkeypatch.setattr(rpn, "_RPN", True)
    m, P64 = _seeded(dev, 31)
    x = _canvas(kind, 7)
    xg = x.to(dev).requires_grad_(True)
    rec = _recording(monkeypatch, m)
    out = m(xg)
    node = rec["rows"][0].grad_fn
    assert type(node).__name__ == "_RPNBackboneBackward"
    assert out["box_preds"].shape == (B, H // 2, W // 2, 14) and out["cls_preds"].shape == (B, H // 2, W // 2, 2) and out["dir_cls_preds"].shape == (B, H // 2, W // 2, 4)
    P = {k: v.clone().requires_grad_(True) for k, v in P64.items()}
    xr = x.double().requires_grad_(True)
    ref, aux = R.forward(P, xr, CFG["layer_nums"], STRIDES, UPS, signs=_kernel_signs(node, m))
    bad = []

    def close(got, want, what):
        try:
            assert_close(_np(got), _np(want), BAR, "%s [%s]" % (what, kind))
        except AssertionError as e:
            bad.append(str(e))

    for k in ref:
        close(out[k], ref[k], k)
    g = torch.Generator().manual_seed(5)
    gouts = {k: torch.randn(v.shape, generator=g, dtype=torch.float64).float() for k, v in ref.items()}
    sum((out[k] * gouts[k].to(dev)).sum() for k in ref).backward()
    sum((ref[k] * gouts[k].double()).sum() for k in ref).backward()
    close(xg.grad, xr.grad, "d canvas")
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        close(p.grad, P[k].grad, "d " + k)
    sd = m.state_dict()
    for _, nname, _, _, _ in R.layer_names(CFG["layer_nums"]):
        c = P64[nname + ".weight"].shape[0]
        rm, rv = R.running(aux, nname, torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64))
        close(sd[nname + ".running_mean"], rm, nname + " running mean")
        close(sd[nname + ".running_var"], rv, nname + " running var")
    assert not bad, bad


def test_eval_mode_vs_f64(dev, monkeypatch):
    monkeypatch.setattr(rpn, "_RPN", True)
    m, P64 = _seeded(dev, 37)
    x = _canvas("randn", 9)
    with torch.no_grad():
        m(x.to(dev))                                                                              # one train-mode forward: running statistics off their initial values
    m.eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ev = m(x.to(dev))
        ev2 = m(x.to(dev))
    assert all(torch.equal(ev[k], ev2[k]) for k in ev)
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in before.items()), "an eval-mode forward updated the state"
    stats = {n[1]: (before[n[1] + ".running_mean"].double().cpu(), before[n[1] + ".running_var"].double().cpu()) for n in R.layer_names(CFG["layer_nums"])}
    ref, _ = R.forward(P64, x.double(), CFG["layer_nums"], STRIDES, UPS, stats=stats)
    for k in ref:
        assert_close(_np(ev[k]), _np(ref[k]), BAR, "eval " + k)
    # an eval-mode forward that records gradients runs the torch ops (the kernels' backward is the train-mode norm's)
    out = m(x.to(dev))
    assert "_RPNBackbone" not in type(out["box_preds"].grad_fn.next_functions[0][0]).__name__
    for k in ref:
        assert_close(_np(out[k]), _np(ref[k]), BAR, "eval under autograd " + k)


def test_torch_op_path_agrees(dev, monkeypatch):
    """PAPC_RPN=0: the module in torch device ops -- a second, independent implementation.  One forward and backward each."""
    a, _ = _seeded(dev, 41)
    b = copy.deepcopy(a)
    x = _canvas("randn", 12).to(dev)
    g = torch.Generator().manual_seed(6)
    monkeypatch.setattr(rpn, "_RPN", True)
    oa = a(x)
    gouts = {k: torch.randn(v.shape, generator=g).to(dev) for k, v in oa.items()}
    sum((oa[k] * gouts[k]).sum() for k in oa).backward()
    monkeypatch.setattr(rpn, "_RPN", False)
    ob = b(x)
    sum((ob[k] * gouts[k]).sum() for k in ob).backward()
    for k in oa:
        assert_close(_np(oa[k]), _np(ob[k]), BAR, k + " kernel vs torch ops")
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        if "running" in k:
            assert_close(_np(va), _np(vb), BAR, k + " kernel vs torch ops")
    # Gradients: a max-norm bar of 5e-2 only, as tests/test_gpu_voxnet.py::test_torch_op_path_agrees and for its reason: the two implementations'
    # activations differ by fp32 rounding, so a ReLU sign within rounding of zero may fall differently.  Both are float64-checked.
    bad = []
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        try:
            assert_close(_np(pa.grad), _np(pb.grad), 5e-2, "d %s kernel vs torch ops" % k, elem=float("inf"))
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, bad


def _train_setup(dev, seed=5):
    from papc_amd.distributed import FlatAdam, FlatParams
    m, _ = _seeded(dev, seed)
    flat = FlatParams(m)
    opt = FlatAdam(flat, lr=1e-3, weight_decay=1e-4)
    return m, flat, opt, _canvas("sparse", seed).to(dev)


def _step(m, opt, x):
    out = m(x)
    sum(v.sum() for v in out.values()).backward()
    opt.step_dev(1.0, zero_grad=True, self_tick=True)


def _state(m, flat, opt):
    return [flat.data, flat.grad, opt.m, opt.v, opt.t_dev] + [v for k, v in m.state_dict().items() if "running" in k]


def test_train_step_bit_reproducible_and_graph_replay_equal(dev, monkeypatch):
    monkeypatch.setattr(rpn, "_RPN", True)
    m, flat, opt, x = _train_setup(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):                     # warm-up (eager, side stream) before the capture
            _step(m, opt, x)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    snap = [t.clone() for t in _state(m, flat, opt)]

    def restore():
        with torch.no_grad():
            for t, v in zip(_state(m, flat, opt), snap):
                t.copy_(v)
        torch.cuda.synchronize()

    _step(m, opt, x)
    torch.cuda.synchronize()
    eager1 = [t.clone() for t in _state(m, flat, opt)]
    restore()
    _step(m, opt, x)
    torch.cuda.synchronize()
    eager2 = [t.clone() for t in _state(m, flat, opt)]
    for a, b in zip(eager1, eager2):
        assert torch.equal(a, b), "two identical train steps differ"
    assert not torch.equal(eager1[0], snap[0])          # the step did move the parameters
    restore()
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _step(m, opt, x)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    restore()
    g.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(eager1, _state(m, flat, opt))):
        assert torch.equal(a, b), "graph replay differs from the eager step (state tensor %d)" % i


def test_train_step_runs_no_foreign_gemm_or_convolution(dev, monkeypatch):
    from torch.profiler import ProfilerActivity, profile
    monkeypatch.setattr(rpn, "_RPN", True)
    m, flat, opt, x = _train_setup(dev)
    _step(m, opt, x)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        _step(m, opt, x)
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    gemmish = ("cijk", "gemm", "gemv", "bmm", "matmul", "rocblas", "hipblas", "tensile", "mfma", "conv", "miopen", "im2col")
    mine = lambda n: "papc::" in n.split("(")[0] or n.startswith("_ZN4papc")      # (demangled or not)
    ours = [n for n in names if mine(n)]
    for k in ("c2d_prep_kernel", "c2d_fwd_kernel", "c2d_dx_kernel", "c2d_dw_kernel", "c2d_relu_bwd_kernel"):
        assert any(k in n for n in ours), (k, sorted(names))
    foreign = [n for n in names if not mine(n) and any(s in n.lower() for s in gemmish)]
    assert not foreign, foreign


def test_inplace_gradients_equal_autograd(dev, monkeypatch):
    from papc_amd.distributed import FlatParams
    monkeypatch.setattr(rpn, "_RPN", True)
    a, _ = _seeded(dev, 43)
    b = copy.deepcopy(a)
    flat = FlatParams(b)
    x = _canvas("randn", 3).to(dev)
    for m in (a, b):
        out = m(x)
        sum((v * v).sum() for v in out.values()).backward()
    assert float(flat.grad.abs().max()) > 0
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert pb.grad is not None and pb.grad.data_ptr() >= flat.grad.data_ptr(), k
        assert_close(_np(pb.grad), _np(pa.grad), 1e-6, "in-place d " + k)                         # the same sums, added onto zeros


def test_errors(dev, monkeypatch):
    monkeypatch.setattr(rpn, "_RPN", True)
    with pytest.raises(_lib.PapcError, match="not built"):
        RPN(use_bev=True)
    with pytest.raises(_lib.PapcError, match="not built"):
        RPN(use_groupnorm=True)
    m = RPN(**CFG).to(dev)
    with pytest.raises(_lib.PapcError, match="input channels"):
        m(torch.zeros(1, 32, 16, 16, device=dev))
    with pytest.raises(_lib.PapcError, match=r"\[B, C, ny, nx\]"):
        m(torch.zeros(64, 16, 16, device=dev))
    with pytest.raises(_lib.PapcError, match="differ in size"):
        m(torch.zeros(1, 64, 36, 48, device=dev))                                                 # 36 -> 18 -> 9 -> 5: 18, 18 and 20 rows
    # outside papc_conv2d_ok the torch ops take over: 48 filters are no multiple of 32
    odd = RPN(num_input_filters=64, num_filters=[48, 64, 64], layer_nums=[0, 0, 0], num_upsample_filters=[32, 32, 32], num_class=1).to(dev)
    x = torch.randn(1, 64, 8, 8, device=dev)
    assert not odd.kernel_ok(x) and m.kernel_ok(torch.zeros(1, 64, 8, 8, device=dev))
    assert odd(x)["box_preds"].shape == (1, 4, 4, 14)


def test_pillars_to_loss_and_predict(dev, monkeypatch):
    """make_pillars -> PFN -> scatter -> RPN -> pointpillars_loss on targets.assign output -> backward(); then detector.PointPillars in eval mode"""
    from papc_amd import detect, detloss
    from papc_amd import targets as T
    from papc_amd.detector import PointPillars
    from papc_amd.synthetic import make_pillars
    from tests import dettarget_cases as C
    monkeypatch.setattr(rpn, "_RPN", True)
    fh, fw, voxel, y0 = 24, 16, 0.4, -9.6
    geo = C._geometry(fh, fw, voxel, y0)
    nx, ny = 2 * fw, 2 * fh
    pc_range = tuple(float(v) for v in geo["pc_range"])
    voxels, nump, coors = make_pillars(P=200, T=20, seed=3, nx=nx, ny=ny, voxel=(voxel, voxel, 4.0), pc_range=pc_range)
    post = dict(nms_score_threshold=0.05, nms_pre_max_size=100, nms_post_max_size=30, nms_iou_threshold=0.5)
    det = PointPillars([1, 64, ny, nx], num_class=1, pfn=dict(num_input_features=4, num_filters=(64,), voxel_size=(voxel, voxel, 4.0), pc_range=pc_range),
                       rpn=dict(num_filters=[32, 32, 64], layer_nums=[1, 1, 1], num_upsample_filters=[32, 32, 32]), post=post).to(dev).train()
    kind, kw = C._car_gen(voxel, y0)
    assigner = T.TargetAssigner([T.AnchorGeneratorStride(**kw)])
    cache = T.anchor_cache(assigner, geo["fmap"], geo["voxel_size"], geo["pc_range"], geo["grid_size"], device=dev)
    gt = C._gts(np.random.default_rng(8), 3, 10.0, -6.0, 6.0)
    tgt = T.assign(cache, torch.from_numpy(gt[None]).to(dev), torch.ones(1, 3, dtype=torch.int32, device=dev), torch.tensor([3], dtype=torch.int32, device=dev))
    assert int(tgt["num_pos"][0]) > 0
    example = {"voxels": torch.from_numpy(voxels).to(dev), "num_points": torch.from_numpy(nump).to(dev), "coordinates": torch.from_numpy(coors).to(dev),
               "anchors": cache["anchors"].unsqueeze(0), "labels": tgt["labels"], "reg_targets": tgt["reg_targets"], "image_idx": [0]}
    # the chain spelled out, stage by stage
    feats = det.pfn(example["voxels"], example["num_points"], example["coordinates"])
    canvas = det.mfe(feats, example["coordinates"], 1)
    assert canvas.shape == (1, 64, ny, nx)
    preds = det.rpn(canvas)
    assert preds["box_preds"].shape == (1, fh, fw, 14)
    res = detloss.pointpillars_loss(preds["box_preds"], preds["cls_preds"], preds["dir_cls_preds"], tgt["labels"], tgt["reg_targets"], example["anchors"], num_class=1)
    res["loss"].backward()
    gw = det.pfn.pfn_layers[0].linear.weight.grad
    assert gw is not None and bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0, "no gradient reached the PFN's weight"
    assert float(det.rpn.block1[1].weight.grad.abs().max()) > 0
    # the module's train branch is that chain
    det2 = copy.deepcopy(det)
    det2.zero_grad(set_to_none=True)
    assert bool(torch.isfinite(det2(example)["loss"]))
    # eval mode: the list predict() returns on the same maps
    det.eval()
    with torch.no_grad():
        got = det(example)
        maps = det.rpn(det.mfe(det.pfn(example["voxels"], example["num_points"], example["coordinates"]), example["coordinates"], 1))
        want = detect.predict(example, maps, num_class=1, **post)
    assert isinstance(got, list) and len(got) == len(want) == 1 and got[0]["box3d_lidar"] is not None
    for k in ("box3d_lidar", "scores", "label_preds"):
        assert torch.equal(got[0][k], want[0][k]), k
