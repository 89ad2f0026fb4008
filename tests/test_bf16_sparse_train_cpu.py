"""bf16 sparse backbone in TRAINING (autograd.set_sparse_precision("bf16"), train_cfg['sparse_precision']) without a GPU: the new
C-ABI entry points (symbols, `_supported` predicates, argument checks), the setter, forward_train's resolution of the config key,
the weight-image kinds, and the float64 restatement of the arithmetic contract the GPU test (test_gpu_bf16_sparse_train.py)
compares the kernels against.

The contract (include/sassd.h "bf16 sparse backbone, training"): every sparse conv but the 4-channel first one multiplies its
bf16-stored operand by the fp32 master weight rounded once to bf16; products are exact, sums fp32, the raw result fp32.  The data
gradient is the same operator on dy (bf16) with the bf16 image of W[k]^T -- on the transposed table, or for a submanifold layer on
the forward table with the offsets reversed; the weight gradient is sum_pairs x^T dy of the two bf16 tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import _C, autograd as AG, kernels as K, weight_images as WI
from oracle import rulebook
from oracle.train_ref import round_bf16
from test_bf16_sparse_infer_cpu import sparse_conv64

EINVAL = -1
FWD_PAIRS = [(16, 16), (16, 32), (32, 32), (32, 64), (64, 64)]
DGRAD_PAIRS = [(32, 16), (64, 32)]
NEW = ("sassd_spconv_train_bf16_supported", "sassd_spconv_train_bf16_packed_bytes", "sassd_spconv_train_bf16_pack_weight",
       "sassd_spconv_fwd_bf16_raw", "sassd_spconv_bwd_weight_bf16_workspace_bytes", "sassd_spconv_bwd_weight_bf16",
       "sassd_bn_relu_fwd_bf16out", "sassd_bn_relu_bwd_bf16out")


# ---- the contract in float64 -------------------------------------------------------------------------------------------------
def R(t):
    """bf16 value (nearest even) of an fp32 tensor, carried in float64"""
    return round_bf16(t.float()).double()


def fwd64(xb, nbr, w):
    """raw forward: xb bf16 values (float64), w fp32 master weight [K, Cin, Cout] -> (sum, sum of magnitudes)"""
    return sparse_conv64(xb, nbr, R(w))


def transpose_table(nbr, n_in):
    """nbrT[i][k] = o  <=>  nbr[o][k] = i"""
    t = np.full((n_in, nbr.shape[1]), -1, np.int64)
    o, k = np.nonzero(nbr >= 0)
    t[nbr[o, k], k] = o
    return t


def dgrad64(dyb, nbr, w, n_in):
    """data gradient on the transposed table with the image of W[k]^T"""
    return sparse_conv64(dyb, transpose_table(np.asarray(nbr), n_in), R(w).transpose(1, 2).contiguous())


def dgrad64_forward_table(dyb, nbr, w):
    """submanifold layers: the forward table with the offset-reversed image of W[k]^T"""
    return sparse_conv64(dyb, nbr, R(w).flip(0).transpose(1, 2).contiguous())


def wgrad64(xb, dyb, nbr):
    """dw[k] = sum over the pairs of offset k of x[in]^T dy[out]; also the sum of magnitudes and the pair count per offset"""
    nbr = torch.as_tensor(np.asarray(nbr), dtype=torch.int64)
    kk = nbr.shape[1]
    dw = torch.zeros(kk, xb.shape[1], dyb.shape[1], dtype=torch.float64)
    mag = torch.zeros_like(dw)
    cnt = np.zeros(kk, np.int64)
    for k in range(kk):
        o = torch.nonzero(nbr[:, k] >= 0).view(-1)
        cnt[k] = o.numel()
        if o.numel():
            xi = xb[nbr[o, k]]
            dw[k] = xi.t() @ dyb[o]
            mag[k] = xi.abs().t() @ dyb[o].abs()
    return dw, mag, cnt


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_resolve():
    L = _C.lib()
    for name in NEW:
        assert name in _C.EXPORTS and callable(getattr(L, name)), name


def test_supported_predicates():
    L = _C.lib()
    sup = L.sassd_spconv_train_bf16_supported
    for cin, cout in FWD_PAIRS + DGRAD_PAIRS:
        for k in (27, 1):
            for cap in (1, 20000, 320000, 1200000):
                assert sup(k, cin, cout, cap), (k, cin, cout, cap)
        assert L.sassd_spconv_train_bf16_packed_bytes(27, cin, cout) == 27 * cin * cout * 2
    for k, cin, cout in ((27, 4, 16), (27, 48, 64), (27, 16, 64), (27, 64, 16), (27, 8, 16), (27, 64, 128), (9, 64, 64), (1, 4, 16)):
        assert not sup(k, cin, cout, 20000), (k, cin, cout)
        assert L.sassd_spconv_train_bf16_packed_bytes(k, cin, cout) == 0
    assert not sup(27, 64, 64, 0) and not sup(27, 64, 64, 1 << 25)
    wsb = L.sassd_spconv_bwd_weight_bf16_workspace_bytes
    for cin, cout in FWD_PAIRS:
        assert wsb(20000, 27, cin, cout) == L.sassd_spconv_bwd_weight_workspace_bytes(20000, 27, cin, cout) > 0
        assert AG.sparse_bf16_layer_supported(27, cin, cout, 20000) and AG.sparse_bf16_layer_supported(1, cin, cout, 20000)
    for cin, cout in DGRAD_PAIRS + [(4, 16), (48, 64)]:                 # data-gradient shapes have no weight gradient of their own
        assert wsb(20000, 27, cin, cout) == 0
        assert not AG.sparse_bf16_layer_supported(27, cin, cout, 20000)
    assert wsb(20000, 1, 64, 64) == 0
    # the inference predicate is what it was
    assert not L.sassd_spconv_bf16_supported(27, 64, 32, 20000) and L.sassd_spconv_bf16_supported(27, 4, 16, 20000)


def _caller(fn, ok, names):
    def call(**kw):
        a = list(ok)
        for n_, v in kw.items():
            a[names.index(n_)] = v
        return fn(*a)
    return call


def test_null_misaligned_and_unsupported_arguments_are_einval():
    L = _C.lib()
    null, p16, odd = None, C.c_void_p(4096), C.c_void_p(4096 + 8)
    pack = _caller(L.sassd_spconv_train_bf16_pack_weight, (p16, 27, 64, 32, p16, null), ("w", "K", "cin", "cout", "out", "s"))
    assert pack(w=null) == EINVAL and pack(out=null) == EINVAL and pack(out=odd) == EINVAL and pack(w=C.c_void_p(4098)) == EINVAL
    assert pack(cin=4, cout=16) == EINVAL and pack(cin=48, cout=64) == EINVAL and pack(K=9) == EINVAL
    fwd = _caller(L.sassd_spconv_fwd_bf16_raw, (p16, p16, p16, 1000, p16, 27, 64, 64, p16, 0, null),
                  ("x", "nbr", "n", "cap", "w", "K", "cin", "cout", "y", "cfg", "s"))
    assert fwd(x=null) == EINVAL and fwd(n=null) == EINVAL and fwd(w=null) == EINVAL and fwd(y=null) == EINVAL
    assert fwd(x=odd) == EINVAL and fwd(w=odd) == EINVAL and fwd(y=odd) == EINVAL and fwd(nbr=C.c_void_p(4098)) == EINVAL
    assert fwd(cap=0) == EINVAL and fwd(cap=1 << 25) == EINVAL and fwd(cfg=1) == EINVAL
    assert fwd(cin=4, cout=16) == EINVAL and fwd(cin=48) == EINVAL and fwd(K=9) == EINVAL
    assert fwd(nbr=null) == EINVAL and fwd(K=1) == EINVAL                       # K = 1 <-> identity rulebook
    wg = _caller(L.sassd_spconv_bwd_weight_bf16, (p16, p16, p16, p16, 1000, 27, 64, 64, p16, 0, 0, p16, 1 << 40, null),
                 ("x", "dy", "nbr", "n", "cap", "K", "cin", "cout", "dw", "acc", "cfg", "ws", "wsb", "s"))
    for name in ("x", "dy", "nbr", "n", "dw", "ws"):
        assert wg(**{name: null}) == EINVAL, name
    assert wg(x=odd) == EINVAL and wg(dy=odd) == EINVAL and wg(ws=odd) == EINVAL and wg(dw=C.c_void_p(4098)) == EINVAL
    assert wg(cap=0) == EINVAL and wg(K=1) == EINVAL and wg(cfg=32) == EINVAL
    assert wg(cin=64, cout=32) == EINVAL and wg(cin=4, cout=16) == EINVAL and wg(cin=48) == EINVAL
    assert wg(wsb=16) == _C.ENOSPC
    ws = L.sassd_bn_relu_workspace_bytes(64)
    bf = _caller(L.sassd_bn_relu_fwd_bf16out, (p16, 100, 64, p16, p16, p16, p16, 0.01, 1e-3, p16, p16, p16, p16, ws, null),
                 ("x", "n", "C", "g", "b", "rm", "rv", "mom", "eps", "y", "mean", "invstd", "ws", "wsb", "s"))
    for name in ("x", "g", "b", "y", "mean", "invstd", "ws"):
        assert bf(**{name: null}) == EINVAL, name
    assert bf(rm=null) == EINVAL                                                # both running statistics or neither
    assert bf(y=C.c_void_p(4098)) == EINVAL and bf(x=odd) == EINVAL and bf(C=6) == EINVAL and bf(n=0) == EINVAL
    assert bf(wsb=16) == _C.ENOSPC
    bb = _caller(L.sassd_bn_relu_bwd_bf16out, (p16, p16, 100, 64, p16, p16, p16, p16, p16, p16, p16, p16, ws, null),
                 ("x", "dy", "n", "C", "g", "b", "mean", "invstd", "dx", "dg", "db", "ws", "wsb", "s"))
    for name in ("x", "dy", "g", "b", "mean", "invstd", "dx", "dg", "db", "ws"):
        assert bb(**{name: null}) == EINVAL, name
    assert bb(dx=C.c_void_p(4098)) == EINVAL and bb(dy=odd) == EINVAL and bb(C=6) == EINVAL and bb(n=0) == EINVAL


# ---- host layer ----------------------------------------------------------------------------------------------------------------
def test_setter_rejects_unknown_values():
    assert AG.sparse_precision() == "fp32"
    for bad in ("fp16", "BF16", None, 16):
        with pytest.raises(ValueError):
            AG.set_sparse_precision(bad)
        with pytest.raises(ValueError):
            AG.sparse_precision_scope(bad)
    AG.set_sparse_precision("bf16")
    try:
        assert AG.sparse_precision() == "bf16"
        with AG.sparse_precision_scope("fp32"):
            assert AG.sparse_precision() == "fp32"
        assert AG.sparse_precision() == "bf16"
    finally:
        AG.set_sparse_precision("fp32")
    assert AG.sparse_precision() == "fp32" and AG.bev_precision() == "fp32"


def test_forward_train_resolves_the_config_key_and_the_key_beats_the_setter(monkeypatch):
    from sassd import detector as D
    from sassd.config import Config
    c = Config.fromfile("configs/car_cfg.py")
    model = D.build_detector(c.model, c.train_cfg, c.test_cfg)
    assert "sparse_precision" not in model.train_cfg
    seen = []
    monkeypatch.setattr(type(model), "_forward_train", lambda self, img, meta, **kw: seen.append(AG.sparse_precision()) or {})
    model.forward_train(None, [{}])
    assert seen == ["fp32"] and model.sparse_training_precision() == "fp32"
    AG.set_sparse_precision("bf16")
    try:
        model.forward_train(None, [{}])                          # no key: the setter
        model.train_cfg["sparse_precision"] = "fp32"
        model.forward_train(None, [{}])                          # the key wins
        assert AG.sparse_precision() == "bf16"                   # ... and the setter's value is back afterwards
    finally:
        AG.set_sparse_precision("fp32")
    model.train_cfg["sparse_precision"] = "bf16"
    model.forward_train(None, [{}])
    assert seen == ["fp32", "bf16", "fp32", "bf16"] and AG.sparse_precision() == "fp32"
    model.train_cfg["sparse_precision"] = "fp16"
    with pytest.raises(ValueError, match="sparse_precision"):
        model.forward_train(None, [{}])
    assert len(seen) == 4


def test_weight_image_kinds_are_distinct_and_follow_the_weight(monkeypatch):
    packed = []

    def fake_pack(w):                                            # the pack kernel's layout on the host
        packed.append(tuple(w.shape))
        return round_bf16(w).transpose(1, 2).contiguous()
    monkeypatch.setattr(K, "spconv_train_bf16_pack_weight", fake_pack)
    WI.store.clear()
    w = torch.nn.Parameter(torch.randn(27, 32, 64))
    kinds = ("spconv16", "spconv16_t", "spconv16_t_rev")
    imgs = {k: AG._spconv16_pack(w, k) for k in kinds}
    assert packed == [(27, 32, 64), (27, 64, 32), (27, 64, 32)]
    wr = round_bf16(w.detach())
    assert torch.equal(imgs["spconv16"], wr.transpose(1, 2))                     # [K][Cout][Cin]
    assert torch.equal(imgs["spconv16_t"], wr)                                   # image of W^T: [K][Cin][Cout]
    assert torch.equal(imgs["spconv16_t_rev"], wr.flip(0))
    assert len({id(v) for v in imgs.values()}) == 3
    for k in kinds:
        assert AG._spconv16_pack(w, k) is imgs[k] and WI.peek(w, k) is imgs[k]   # cached
    assert WI.peek(w, "spconv") is None and WI.peek(w, "spconv_t") is None       # the fp32 kinds are other entries
    with torch.no_grad():
        w.mul_(2.0)                                                              # an in-place write: every image is stale
    for k in kinds:
        assert WI.peek(w, k) is None, k
        assert AG._spconv16_pack(w, k) is not imgs[k]
    imgs = {k: WI.peek(w, k) for k in kinds}
    K.bump_weights_generation()                                                  # a raw-pointer writer (the fused optimizer)
    for k in kinds:
        assert WI.peek(w, k) is None, k
    WI.store.clear()


# ---- the contract --------------------------------------------------------------------------------------------------------------
def _subm_case(seed, cin, cout):
    rng = np.random.default_rng(seed)
    shape = (6, 9, 8)
    idx = np.stack([rng.integers(0, 2, 120), rng.integers(0, shape[0], 120), rng.integers(0, shape[1], 120),
                    rng.integers(0, shape[2], 120)], 1).astype(np.int32)
    idx, nbr = rulebook.subm_rulebook(np.unique(idx, axis=0), shape)
    g = torch.Generator().manual_seed(seed)
    n = idx.shape[0]
    return (nbr, R(torch.relu(torch.randn(n, cin, generator=g))), torch.randn(27, cin, cout, generator=g) / 8,
            R(torch.randn(n, cout, generator=g)))


def test_float64_contract_is_the_gradient_of_its_forward():
    """dgrad64 / wgrad64 are the derivatives of fwd64 with respect to the operand and to the (rounded) weight"""
    nbr, xb, w, dyb = _subm_case(3, 16, 32)
    x = xb.clone().requires_grad_(True)
    wr = R(w).requires_grad_(True)
    y = torch.zeros(nbr.shape[0], 32, dtype=torch.float64)
    nb = torch.as_tensor(nbr, dtype=torch.int64)
    for k in range(27):
        o = torch.nonzero(nb[:, k] >= 0).view(-1)
        y = y.index_add(0, o, x[nb[o, k]] @ wr[k])
    assert torch.equal(y.detach(), fwd64(xb, nbr, w)[0])
    y.backward(dyb)
    dx, _ = dgrad64(dyb, nbr, w, xb.shape[0])
    dw, mag, cnt = wgrad64(xb, dyb, nbr)
    assert torch.allclose(dx, x.grad, rtol=1e-12, atol=1e-12) and torch.allclose(dw, wr.grad, rtol=1e-12, atol=1e-12)
    assert (mag >= dw.abs() - 1e-12).all() and cnt[13] == nbr.shape[0]


@pytest.mark.parametrize("cin,cout", [(16, 16), (16, 32), (64, 64)])
def test_forward_table_data_gradient_equals_the_transposed_table_form(cin, cout):
    """on rounded operands: dx[i] = sum_k dy[nbr[i][k]] . bf16(W[26-k])^T equals the transposed-table sum term by term (the same
    exact products), so the float64 sums agree to their own rounding"""
    nbr, xb, w, dyb = _subm_case(cin + cout, cin, cout)
    a, amag = dgrad64(dyb, nbr, w, xb.shape[0])
    b, bmag = dgrad64_forward_table(dyb, nbr, w)
    assert torch.allclose(amag, bmag, rtol=1e-13, atol=0)
    assert ((a - b).abs() <= 1e-13 * amag + 1e-300).all()
    # ... and the image the pack makes for it is the weight's own [K][Cin][Cout] order, offsets reversed
    assert torch.equal(R(w).flip(0).transpose(1, 2).transpose(1, 2), R(w).flip(0))
