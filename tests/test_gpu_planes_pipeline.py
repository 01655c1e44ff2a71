"""The pipelined main loop of the plane-set GEMMs (PAPC_PG_PIPE=1, pg_ring_k16 in csrc/smallm.hip: a four-slot k16 LDS ring whose LDS-DMA
stays in flight across the barriers) against the k32 stage loop it replaces (PAPC_PG_PIPE=0): BIT-identical results on the raw entry
points for every epilogue, both tile flavours, split K and the grouped launch, at block counts below, at and beyond the ring's four slots;
against a float64 product on its own terms; and three launches back to back (a drain that left a DMA behind would show in the next
workgroup on the CU)."""
import ctypes

import numpy as np
import pytest
import torch

from papc_amd import _lib, smallm
from tests.test_gpu_planes_grouped import _layer_products, _planes, _rand
from tests.util import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture
def knobs():
    lib = _lib.load()
    old = {}

    def set_(name, v):
        if name not in old:
            o = ctypes.c_int()
            _lib.check(lib.papc_knob_get(name, ctypes.byref(o)), "papc_knob_get")
            old[name] = o.value
        _lib.check(lib.papc_knob_set(name, int(v)), "papc_knob_set")
    yield set_
    for name, v in old.items():
        _lib.check(lib.papc_knob_set(name, v), "papc_knob_set")


class _Product:
    """one A [R1, K] x B [R2, K]^T product on random operands, with every array any epilogue needs"""

    def __init__(self, dev, R1, R2, K, seed):
        self.lib = lib = _lib.load()
        self.dev, self.R1, self.R2, self.K = dev, R1, R2, K
        rng = np.random.default_rng(seed)
        self.a, self.b = _rand(rng, (R1, K), dev), _rand(rng, (R2, K), dev)
        self.pa, self.pb = _planes(lib, self.a, dev), _planes(lib, self.b, dev)
        self.bias = _rand(rng, (R2,), dev)
        self.y_prev = _rand(rng, (R1, R2), dev)
        self.cst = torch.from_numpy(rng.normal(size=(4, R2)).astype(np.float32)).to(dev)     # mean, invstd, scale, shift
        self.cst[1] = self.cst[1].abs() + 0.5
        self.tiles = (R1 + 127) // 128

    def run(self, epi, split=1):
        """launch into NaN-poisoned outputs; returns the list of output tensors"""
        dev, R1, R2, T = self.dev, self.R1, self.R2, self.tiles
        nan = float("nan")
        c = torch.full((split, R1, R2), nan, device=dev)
        outs = [c]
        g = smallm.PgGemm()
        g.epi, g.a, g.b, g.R1, g.R2, g.K = epi, self.pa.data_ptr(), self.pb.data_ptr(), R1, R2, self.K
        g.c, g.ldc, g.split, g.split_stride, g.family = c.data_ptr(), R2, split, R1 * R2, smallm.K_MLP_GEMM
        if epi != smallm.EPI_STORE:
            stats = torch.full((T, 2, R2), nan, device=dev)
            g.stats = stats.data_ptr()
            outs.append(stats)
        if epi in (smallm.EPI_FWD, smallm.EPI_FWD_GMAX):
            g.bias = self.bias.data_ptr()
        if epi == smallm.EPI_FWD_GMAX:
            gm = [torch.full((T, R2), nan, device=dev) for _ in range(2)]
            am = [torch.full((T, R2), -1, device=dev, dtype=torch.int32) for _ in range(2)]
            g.gmax, g.gmin, g.amax, g.amin = gm[0].data_ptr(), gm[1].data_ptr(), am[0].data_ptr(), am[1].data_ptr()
            outs += gm + am
        if epi == smallm.EPI_RED:
            g.y_prev = self.y_prev.data_ptr()
            g.mean, g.invstd, g.scale, g.shift = (self.cst[i].data_ptr() for i in range(4))
        _lib.check(self.lib.papc_pg_gemm_f32(ctypes.byref(g), _lib.stream_ptr()), "papc_pg_gemm_f32")
        return outs


def _variants(R1, K):
    """(epilogue, split) pairs the shape admits"""
    v = [(smallm.EPI_STORE, 1), (smallm.EPI_FWD, 1), (smallm.EPI_RED, 1)]        # (ldc == R2 throughout: RED always applies)
    if R1 % 128 == 0:
        v.append((smallm.EPI_FWD_GMAX, 1))
    nst = (K + 31) // 32
    v += [(smallm.EPI_STORE, s) for s in (2, 3) if nst % s == 0]
    return v


# k16 blocks per workgroup: 2, 2, 4, 4, 6, 8, 10, 18 (fewer than the ring's slots, exactly one ring, one wrap, several wraps; zero-padded
# last blocks at K = 16, 48, 160); split 3 at K = 96 leaves a single k32 stage per workgroup
@pytest.mark.parametrize("R1,R2", [(128, 128), (256, 64), (200, 72), (384, 24)])     # full tiles, ragged rows, ragged columns, one narrow tile
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("K", [16, 32, 48, 64, 96, 128, 160, 288])
def test_pipelined_equals_unpipelined(dev, knobs, K, nb, R1, R2):
    pr = _Product(dev, R1, R2, K, 1000 * K + 10 * R1 + R2 + nb)
    knobs(b"PAPC_PG_NB", nb)
    for epi, split in _variants(R1, K):
        knobs(b"PAPC_PG_PIPE", 0)
        want = pr.run(epi, split)
        knobs(b"PAPC_PG_PIPE", 1)
        got = pr.run(epi, split)
        for i, (a, b) in enumerate(zip(got, want)):
            assert bool(torch.isfinite(b.float()).all()), (epi, split, i)
            assert torch.equal(a, b), "epilogue %d, split %d, output %d" % (epi, split, i)
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,cin,cout,red", [(384, 43, 72, True), (512, 259, 24, False), (384, 43, 24, True)])
def test_pipelined_group_equals_unpipelined(dev, knobs, M, cin, cout, red):
    """the grouped launch on products with different stage counts, in both array orders"""
    lib = _lib.load()
    st = _lib.stream_ptr()
    gs, outs, keep = _layer_products(dev, M, cin, cout, red, 7 * M + cin + cout)
    knobs(b"PAPC_PG_GROUP", 1)
    for order in ((0, 1), (1, 0)):
        arr = (smallm.PgGemm * 2)(gs[order[0]], gs[order[1]])
        res = []
        for pipe in (0, 1):
            knobs(b"PAPC_PG_PIPE", pipe)
            for t in outs:
                t.fill_(float("nan"))
            _lib.check(lib.papc_pg_gemm_group_f32(arr, 2, st), "papc_pg_gemm_group_f32")
            res.append([t.clone() for t in outs])
        for i, (a, b) in enumerate(zip(res[1], res[0])):
            assert bool(torch.isfinite(b).all()), (order, i)
            assert torch.equal(a, b), (order, i)
    torch.cuda.synchronize()
    del keep


@pytest.mark.parametrize("R1,R2,K,nb", [(128, 128, 16, 0), (200, 72, 288, 1)])       # the shortest loop; wraps, ragged, 64-column tiles
def test_pipelined_vs_f64(dev, knobs, R1, R2, K, nb):
    """correct on its own terms: the 3e-6 bar of tests/test_gpu_planes.py::test_planes_gemm_vs_f64 (there relative to sum |a_k b_k|, whose
    figure is printed) under tests.util.assert_close"""
    pr = _Product(dev, R1, R2, K, R1 + R2 + K)
    knobs(b"PAPC_PG_NB", nb)
    knobs(b"PAPC_PG_PIPE", 1)
    got = pr.run(smallm.EPI_STORE)[0][0].double()
    ref = pr.a.double() @ pr.b.double().t()
    mag = pr.a.double().abs() @ pr.b.double().abs().t()
    err = float(((got - ref).abs() / mag).max())
    print("planes pipeline vs f64: R1 %d R2 %d K %d: max error / sum|a b| = %.3g" % (R1, R2, K, err))
    assert_close(got.cpu().numpy(), ref.cpu().numpy(), 3e-6, "pipelined planes GEMM vs f64")


def test_pipelined_back_to_back(dev, knobs):
    """three launches on one stream into three buffers: nothing of one workgroup's ring survives into the next on the CU"""
    pr = _Product(dev, 512, 256, 160, 5)
    knobs(b"PAPC_PG_NB", 2)
    knobs(b"PAPC_PG_PIPE", 1)
    runs = [pr.run(smallm.EPI_FWD) for _ in range(3)]
    torch.cuda.synchronize()
    for r in runs[1:]:
        for i, (a, b) in enumerate(zip(r, runs[0])):
            assert bool(torch.isfinite(b).all()), i
            assert torch.equal(a, b), i
