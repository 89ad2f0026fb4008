"""-m gpu: the densify family (sassd_densify, _densify_bf16, _densify_from_bf16) and sassd_voxel_mean alone, bit for bit against
the references of tests/rulebook_cases.py: both clearing branches of sassd_densify, both channel orders away from C = 64, n = 0,
n < cap with live-looking rows past n, a count above the capacity, n * C either side of a block, -0.0 / inf / subnormal / NaN
payloads, the bf16 rounding at ties, at overflow and at +-0."""
import numpy as np
import pytest
import torch

from sassd import kernels as K
from oracle import clib, nets as onets
import rulebook_cases as RC

pytestmark = pytest.mark.gpu

I32, I16 = torch.int32, torch.int16


def _f32(bits, dev):
    """fp32 device tensor holding exactly these uint32 bit patterns."""
    return torch.tensor(np.ascontiguousarray(bits).view(np.int32), device=dev).view(torch.float32)


def _bf16(bits, dev):
    return torch.tensor(np.ascontiguousarray(bits).view(np.int16), device=dev).view(torch.bfloat16)


def _bits32(t):
    return t.contiguous().view(I32).cpu().numpy().view(np.uint32)


def _bits16(t):
    return t.contiguous().view(I16).cpu().numpy().view(np.uint16)


def _oracle_map(bits, idx, n, shape, batch, order):
    """oracle.nets.densify plus the permutation of test_densify, as uint32 bits."""
    d, h, w = shape
    c = bits.shape[1]
    f = torch.from_numpy(np.ascontiguousarray(bits[:n]).view(np.int32).copy()).view(torch.float32)
    o = onets.densify(f, idx[:n], shape, batch)
    if order:
        o = o.view(batch, c, d, h, w).permute(0, 2, 1, 3, 4).reshape(batch, c * d, h, w)
    return _bits32(o)


def _calls(cs):
    """(n_ptr value, cap told to the kernel, rows the map must hold): n < cap, and a count above the capacity (clamped)."""
    return [(cs["n"], cs["cap"], cs["n"]), (cs["cap"] + 5, cs["cap"], cs["cap"])]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("cfg", range(len(RC.DENSIFY_F32)))
def test_densify(dev, cfg, order):
    shape, batch, chans, rows = RC.DENSIFY_F32[cfg]
    d, h, w = shape
    for c in chans:
        memset_branch = (batch * c * d * h * w * 4) % 16 != 0
        assert memset_branch == (cfg == 0)
        for n in rows or RC.densify_rows(c):
            cs = RC.densify_case(shape, batch, c, n, RC.SPECIAL_F32)
            feats, idx = _f32(cs["feats"], dev), torch.tensor(cs["idx"], device=dev)
            for nptr, cap, live in _calls(cs):
                out = torch.full((batch, c * d, h, w), 123.0, device=dev)
                assert memset_branch or out.data_ptr() % 16 == 0
                r = K.densify(feats, idx, torch.tensor([nptr], dtype=I32, device=dev), cap, shape, batch, order, out=out)
                assert r is out
                ref = RC.densify_ref_bits(cs["idx"], cs["feats"], live, shape, batch, order)
                assert np.array_equal(ref, _oracle_map(cs["feats"], cs["idx"], live, shape, batch, order))
                got = _bits32(out)
                assert np.array_equal(got, ref), (shape, c, n, nptr, order, int((got != ref).sum()))
                if live == 0:
                    assert not got.any()
            assert n * c < len(RC.SPECIAL_F32) or set(RC.SPECIAL_F32.tolist()) <= set(cs["feats"][:n].reshape(-1).tolist())


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("cfg", range(len(RC.DENSIFY_BF16)))
def test_densify_bf16(dev, cfg, order):
    shape, batch, chans, rows = RC.DENSIFY_BF16[cfg]
    d, h, w = shape
    pat = RC.bf16_patterns()
    assert K.densify_bf16_supported(chans[0], shape)
    for c in chans:
        ns = rows or RC.densify_rows(c)
        assert max(ns) * c >= len(pat), "the largest case holds every pattern"
        for n in ns:
            cs = RC.densify_case(shape, batch, c, n, pat, seed=1)
            feats, idx = _f32(cs["feats"], dev), torch.tensor(cs["idx"], device=dev)
            for nptr, cap, live in _calls(cs):
                out = _bf16(np.full((batch, c * d, h, w), 0x4321, np.uint16), dev)
                K.densify_bf16(feats, idx, torch.tensor([nptr], dtype=I32, device=dev), cap, shape, batch, order, out=out)
                got = _bits16(out)
                ref32 = RC.densify_ref_bits(cs["idx"], cs["feats"], live, shape, batch, order)
                nan = RC.is_nan_bits32(ref32)
                assert np.array_equal(RC.is_nan_bits16(got), nan), "NaN stays NaN and nothing else becomes one"
                ref16 = RC.round_bf16_bits(ref32)
                assert np.array_equal(got[~nan], ref16[~nan]), (shape, c, n, nptr, order)
                tref = torch.from_numpy(ref32.view(np.int32).copy()).view(torch.float32).to(torch.bfloat16)
                assert np.array_equal(got[~nan], _bits16(tref)[~nan])
            if n == max(ns):
                assert set(pat.tolist()) <= set(cs["feats"][:n].reshape(-1).tolist())


def test_densify_bf16_refuses_a_plane_the_fill_kernel_cannot_clear(dev):
    shape, batch, c = (3, 5, 7), 2, 3
    assert not K.densify_bf16_supported(c, shape)
    cs = RC.densify_case(shape, batch, c, 20, RC.SPECIAL_F32)
    out = _bf16(np.full((batch, c * 3, 5, 7), 0x4321, np.uint16), dev)
    nptr = torch.tensor([20], dtype=I32, device=dev)
    with pytest.raises(RuntimeError, match="sassd_densify_bf16 failed"):
        K.densify_bf16(_f32(cs["feats"], dev), torch.tensor(cs["idx"], device=dev), nptr, cs["cap"], shape, batch, 0, out=out)
    feats16 = _bf16((cs["feats"] >> 16).astype(np.uint16), dev)
    with pytest.raises(RuntimeError, match="sassd_densify_from_bf16 failed"):
        K.densify_from_bf16(feats16, torch.tensor(cs["idx"], device=dev), nptr, cs["cap"], shape, batch, 0, out=out)
    torch.cuda.synchronize()
    assert (_bits16(out) == 0x4321).all(), "an error return must not launch"


@pytest.mark.parametrize("out_bf16", [True, False])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("cfg", range(len(RC.DENSIFY_BF16)))
def test_densify_from_bf16(dev, cfg, order, out_bf16):
    """bits copied into a bf16 map, or widened exactly (<< 16) into an fp32 map."""
    shape, batch, chans, rows = RC.DENSIFY_BF16[cfg]
    d, h, w = shape
    special = (RC.SPECIAL_F32 >> 16) << 16
    special = np.concatenate([special, np.array([0x7FC10000, 0x00010000, 0x80010000, 0x7F7F0000], np.uint32)])
    for c in chans:
        for n in rows or RC.densify_rows(c):
            cs = RC.densify_case(shape, batch, c, n, special, seed=2)
            bits16 = (cs["feats"] >> 16).astype(np.uint16)
            assert (bits16[n:] != 0).all()
            feats, idx = _bf16(bits16, dev), torch.tensor(cs["idx"], device=dev)
            for nptr, cap, live in _calls(cs):
                if out_bf16:
                    out = _bf16(np.full((batch, c * d, h, w), 0x4321, np.uint16), dev)
                else:
                    out = torch.full((batch, c * d, h, w), 123.0, device=dev)
                K.densify_from_bf16(feats, idx, torch.tensor([nptr], dtype=I32, device=dev), cap, shape, batch, order, out=out,
                                    out_bf16=out_bf16)
                ref = RC.densify_ref_bits(cs["idx"], bits16, live, shape, batch, order)
                if out_bf16:
                    assert np.array_equal(_bits16(out), ref), (shape, c, n, nptr, order)
                else:
                    assert np.array_equal(_bits32(out), ref.astype(np.uint32) << 16), (shape, c, n, nptr, order)


@pytest.mark.parametrize("t", RC.VOXEL_MEAN_T)
@pytest.mark.parametrize("ndim,nfeat", RC.VOXEL_MEAN_DIMS)
def test_voxel_mean(dev, t, ndim, nfeat):
    for m in RC.VOXEL_MEAN_M:
        v, num = RC.voxel_mean_case(m, t, ndim)
        got = K.voxel_mean(torch.tensor(v, device=dev), torch.tensor(num, device=dev), nfeat)
        assert got.shape == (m, nfeat) and got.dtype == torch.float32
        got = _bits32(got)
        assert np.array_equal(got, clib.voxel_mean(v, num, nfeat).view(np.uint32)), (t, ndim, nfeat, m)
        assert np.array_equal(got, RC.voxel_mean_twin(v, num, nfeat).view(np.uint32)), (t, ndim, nfeat, m)


def test_voxel_mean_without_voxels(dev):
    """m = 0 returns without a launch (a tensor without rows has no address: it is not an invalid argument)."""
    got = K.voxel_mean(torch.empty(0, 5, 4, device=dev), torch.empty(0, dtype=I32, device=dev), 4)
    torch.cuda.synchronize()
    assert got.shape == (0, 4)
