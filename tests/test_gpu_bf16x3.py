"""The 3-way bf16 split of an fp32 operand (papc_amd/csrc/bf16x3.h), pinned bit for bit.

papc_pg_prep_weights_f32 applies the split to a caller's fp32 matrix with nothing else in between and stores the three planes in the
fragment layout of csrc/smallm.hip.  The planes are decoded here and every stored bf16 is compared, plane by plane and on its BITS,
with a NumPy emulation of what bf16x3.h documents:

    x1 = bf16(x)    x2 = bf16(x - x1)    x3 = bf16(x - x1 - x2)        (round to nearest even; the subtractions in float32)

No tolerance: a float32 NumPy subtraction is the IEEE subtraction the kernel performs, and the rounding is emulated on the integer
bits.  The tolerance tests of the GEMMs would pass a swapped subtraction or a truncating conversion in one copy of the split
(about 1e-5 relative); this test is what says which bits every copy must produce.

Inputs are finite with |x| < 2^127: from 2^127 (1 - 2^-9) on the leading plane can round to infinity and the residual is no longer
a number.  No NaN, no infinity.
"""
import numpy as np
import pytest
import torch

from papc_amd import _lib, smallm

gpu = pytest.mark.gpu          # (test_the_emulation is NumPy only and runs everywhere)

LIMIT = np.float32(2.0 ** 127)
NEG_RESIDUAL = np.float32(1.99)        # bf16(1.99) = 1.9921875 > 1.99: the first residual is negative
HAND = np.array([0.0, -0.0, 1.0, 1.0 + 2.0 ** -23, NEG_RESIDUAL, -NEG_RESIDUAL, 2.0 ** -126, -(2.0 ** -126)], np.float32)


# ---- the split, in NumPy ---------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 -> the bits of the nearest bf16, ties to even (finite inputs)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def split3(x):
    """[R, K] float32 -> bits of the three planes, [3, R, K] uint16"""
    assert x.dtype == np.float32
    planes, r = [], x.copy()
    for _ in range(3):
        p = bf16_rne(r)
        planes.append(p)
        r = r - bf16_to_f32(p)          # float32 - float32 -> float32
        assert r.dtype == np.float32
    return np.stack(planes)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def values(rng, R, K):
    """normal float32 with the exponent uniform over 2^-60 .. 2^60, every significand bit random, either sign; the hand-picked values first"""
    n = R * K
    bits = (rng.integers(0, 2, n, dtype=np.uint32) << 31) | (rng.integers(127 - 60, 127 + 61, n, dtype=np.uint32) << 23) | rng.integers(0, 1 << 23, n, dtype=np.uint32)
    v = bits.view(np.float32).copy()
    v[:HAND.size] = HAND
    assert np.isfinite(v).all() and (np.abs(v) < LIMIT).all()
    return v.reshape(R, K)


def ru(a, b):
    return (a + b - 1) // b * b


def decode(buf, R, K):
    """plane buffer (uint8 tensor) -> [3, ru(R, 32), ru(K, 32)] uint16: the part of the padded planes that the prep kernel writes.
    Fragment (rb, kb, plane) at byte ((rb * KB + kb) * 3 + plane) * 1024, KB = ru(K, 32) / 16; in it element (r, k) is bf16 number
    k & 7 of the 16-byte lane slot (r & 31) + 32 * ((k & 15) >> 3)."""
    Rp, Kp = ru(R, 32), ru(K, 32)
    RB, KB = Rp // 32, Kp // 16
    a = buf.cpu().numpy().view(np.uint16)[:RB * KB * 3 * 512].reshape(RB, KB, 3, 2, 32, 8)     # rb, kb, plane, k half, row, k & 7
    return np.ascontiguousarray(a.transpose(2, 0, 4, 1, 3, 5)).reshape(3, Rp, Kp)


def run(dev, mats):
    """[(x [R, K] float32, transposed source?)] -> decoded planes, all jobs in ONE launch"""
    lib = _lib.load()
    arr, keep = (smallm.PgWJob * len(mats))(), []
    for a, (x, tr) in zip(arr, mats):
        R, K = x.shape
        src = torch.from_numpy(np.ascontiguousarray(x.T if tr else x)).to(dev)
        buf = torch.full((lib.papc_pg_planes_bytes(R, K),), 0xA5, dtype=torch.uint8, device=dev)    # (not zeros: the padding must be WRITTEN)
        a.src, a.R, a.K, a.planes = src.data_ptr(), R, K, buf.data_ptr()
        a.row_stride, a.col_stride = (1, R) if tr else (K, 1)
        keep.append((src, buf))
    _lib.check(lib.papc_pg_prep_weights_f32(arr, len(mats), _lib.stream_ptr()), "papc_pg_prep_weights_f32")
    torch.cuda.synchronize()
    return [decode(buf, *x.shape) for (x, _), (_, buf) in zip(mats, keep)]


def check(x, got):
    R, K = x.shape
    ref = split3(x)
    for p in range(3):
        assert np.array_equal(got[p, :R, :K], ref[p]), "plane %d: %d of %d bf16 differ" % (p, int((got[p, :R, :K] != ref[p]).sum()), R * K)
    assert not got[:, R:, :].any(), "padding rows are not zero"
    assert not got[:, :, K:].any(), "padding k is not zero"
    # the planes add up to the input, exactly, in float32
    p1, p2, p3 = (bf16_to_f32(got[p, :R, :K]) for p in range(3))
    s = (p1 + p2) + p3
    assert s.dtype == np.float32
    normal = np.abs(x) >= np.float32(2.0 ** -126)
    assert np.array_equal(s[normal], x[normal])
    assert np.array_equal(s.view(np.uint32)[normal], x.view(np.uint32)[normal])


def test_the_emulation():
    """The self-check of the reference and of the inputs: round to nearest EVEN, a negative residual, and inputs on which a
    truncating conversion or a dropped plane has other bits."""
    assert bf16_rne(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23], np.float32)).tolist() == [0x3F80, 0x3F82, 0x3F81]
    h = split3(HAND.reshape(1, -1))[:, 0]
    assert bf16_to_f32(h[1])[4] < 0 and bf16_to_f32(h[1])[5] > 0                      # NEG_RESIDUAL
    assert h[:, 3].tolist() == [0x3F80, 0x3400, 0]                                    # 1 + 2^-23 = 1 + 2^-23 + 0
    assert h[:, 0].tolist() == [0, 0, 0] and h[:, 1].tolist() == [0x8000, 0, 0]       # -0 - (-0) = +0
    assert h[:, 6].tolist() == [0x0080, 0, 0]                                         # the smallest normal
    x = values(np.random.default_rng(1), 33, 17)
    ref = split3(x)
    trunc = (x.view(np.uint32) >> 16).astype(np.uint16)
    assert (ref[0] != trunc).mean() > 0.3 and ref[2].any()


@gpu
@pytest.mark.parametrize("R,K", [(33, 17), (128, 32)])
def test_split_row_major(dev, R, K):
    """(33, 17): ragged rows and ragged k, a second row block and a second k block; (128, 32): full fragments"""
    x = values(np.random.default_rng(1000 + R), R, K)
    got, = run(dev, [(x, False)])
    check(x, got)


@gpu
def test_split_transposed_two_jobs(dev):
    """the W^T job form of the backward (row_stride = 1, col_stride = R), and two jobs in one launch (the blockIdx.y job index)"""
    rng = np.random.default_rng(2000)
    xs = [values(rng, 5, 9), values(rng, 5, 9)]
    assert not np.array_equal(xs[0], xs[1])
    for x, got in zip(xs, run(dev, [(x, True) for x in xs])):
        check(x, got)
