"""-m gpu: the bf16 sparse backbone in TRAINING (autograd.set_sparse_precision("bf16"), train_cfg['sparse_precision'] = 'bf16').

Kernels against the float64 contract of test_bf16_sparse_train_cpu.py on the same rounded operands; the BatchNorm store variants
bit for bit against the fp32 kernels; every sparse launch of an autograd stack against float64 on its live operands; whole
deterministic training steps bit for bit, and the fp32 path untouched by a toggle."""
import math

import numpy as np
import pytest
import torch
from torch import nn

from sassd import autograd as AG, kernels as K, spconv, weight_images as WI
from oracle import rulebook
from oracle.train_ref import round_bf16
import test_bf16_sparse_train_cpu as T16
from test_bf16_sparse_infer_cpu import sparse_conv64
from test_gpu_bf16_sparse import _rand_rulebook, EPS
import det_train

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # unit roundoff of fp32
# Forward / data-gradient bar, per element: d * 2^-24 * sum |x w| with d the longest chain of dependent fp32 additions.
# spconv_raw16_kernel keeps the summation structure of the inference kernel (spconv_bf16_rows is one body): per 4-channel MFMA step
# 4 products, CIN / 16 steps per accumulator chain, the sum of the four quarter chains (2), one slab add per (offset, row) (<= 27),
# the wave-slab sum (3): below 80 additions, i.e. d * 2^-24 < 4.8e-6 -- the EPS = 1.5e-5 derived in test_gpu_bf16_sparse.py covers
# it.  Never more than the order-free bound (m - 1) * 2^-24 with m the number of products of the element.
assert 80 * U < EPS


@pytest.fixture(scope="module", autouse=True)
def _leave_the_process_as_found():
    """This file grows the shared weight-gradient workspace to a 70 000-row capacity and trains four detectors; what it cached
    (kernel workspaces, allocator blocks) is dropped at the end, so the test files after it start from the memory they always had."""
    before = dict(K._ws_cache)
    yield
    for key in [k for k, t in K._ws_cache.items() if before.get(k) is not t]:
        del K._ws_cache[key]
    WI.store.clear()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _bar(asum, m):
    return torch.minimum(torch.full_like(asum, EPS), (m - 1).clamp_min(0) * U) * asum


def _check_conv(y, x64, nbr, w64, tag):
    """y fp32 [n, Cout] against float64 on the same (already rounded) operands"""
    n = y.shape[0]
    if nbr is None:
        acc, asum = x64[:n] @ w64[0], x64[:n].abs() @ w64[0].abs()
        m = torch.full_like(acc, x64.shape[1])
    else:
        acc, asum = sparse_conv64(x64, nbr, w64)
        m = torch.as_tensor((np.asarray(nbr) >= 0).sum(1) * x64.shape[1], dtype=torch.float64).view(-1, 1).expand_as(acc)
    err = (y.double().cpu() - acc).abs()
    bad = err > _bar(asum, m)
    assert not bool(bad.any()), (tag, int(bad.sum()), float((err / asum.clamp_min(1e-300)).max()))
    return float((err / asum.clamp_min(1e-300)).max())


def _wgrad_depth(cap, n):
    """longest chain of dependent fp32 additions of sassd_spconv_bwd_weight_bf16 as built: 16 products inside one
    v_mfma_f32_16x16x16_bf16, one accumulation per 16-pair step of a chunk (rows per chunk / 16), the reduce kernel's per-thread
    chain over every 16th chunk (+ 1 for its two accumulators), its 8 partial sums (+ 1 for `accumulate`)"""
    r = ((cap + 511) // 512 + 63) // 64 * 64
    wg_rows = min(max(r, 128), 2048)
    nwg = (n + wg_rows - 1) // wg_rows
    return 16 + math.ceil(min(wg_rows, max(n, 1)) / 16) + math.ceil(nwg / 16) + 1 + 8 + 1


def _same(a, b, tag):
    assert len(a["loss"]) == len(b["loss"])
    for i, (x, y) in enumerate(zip(a["loss"], b["loss"])):
        assert torch.equal(x, y), (tag, "loss", i, float(x), float(y))
    for k in a["terms"]:
        for i, (x, y) in enumerate(zip(a["terms"][k], b["terms"][k])):
            assert torch.equal(x, y), (tag, k, i)
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(a[k], b[k]), (tag, k)


# ---- 5. whole step (first in the file: its fp32 baseline runs before this file switches the mode on) ---------------------------------
@pytest.mark.parametrize("dense", ["bf16"])
def test_whole_step_is_bit_reproducible_and_a_toggle_leaves_fp32_untouched(dev, dense):
    kw = dict(steps=3, precision=dense, deterministic=True, batch=1, frames=2)
    assert AG.sparse_precision() == "fp32"
    base = det_train.run(dev, **kw)
    AG.set_sparse_precision("bf16")
    try:
        a = det_train.run(dev, **kw)
        b = det_train.run(dev, **kw)
    finally:
        AG.set_sparse_precision("fp32")
    again = det_train.run(dev, **kw)
    assert a["deterministic"] and len(a["loss"]) == 3
    _same(a, b, "bf16 sparse, two runs")
    for k, v in a["terms"].items():
        assert all(bool(torch.isfinite(t).all()) for t in v), k
    assert all(bool(torch.isfinite(t).all()) for t in a["loss"]) and bool(torch.isfinite(a["params"]).all())
    _same(base, again, "fp32 sparse before / after the toggle")
    assert not torch.equal(a["params"], base["params"]), "the mode changed nothing"
    print("3 steps, losses fp32-sparse %s | bf16-sparse %s" % ([round(float(t), 5) for t in base["loss"]],
                                                               [round(float(t), 5) for t in a["loss"]]))


# ---- 1. forward / data-gradient kernel -----------------------------------------------------------------------------------------
PAIRS = T16.FWD_PAIRS + T16.DGRAD_PAIRS
ROWS = (0, 1, 31, 257, 16384, 16385)      # empty, one row, fewer rows than an XCD block has slices, several slices, 1 / 2 blocks per XCD


@pytest.mark.parametrize("k", [27, 1])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_raw_conv_vs_float64(dev, k, cin, cout):
    g = torch.Generator().manual_seed(cin * 7 + cout + k)
    w = torch.randn(k, cin, cout, generator=g) / np.sqrt(cin * min(k, 8))
    wp = K.spconv_train_bf16_pack_weight(w.to(dev))
    assert torch.equal(wp.view(torch.bfloat16).view(k, cout, cin).cpu(), round_bf16(w).transpose(1, 2).to(torch.bfloat16))
    wr = round_bf16(w).double()
    worst = 0.0
    for n in ROWS:
        cap = n + 100
        kind = "subm" if cin == cout else "down"
        n_in = max(n, 1) + (n // 3 if kind == "down" else 0)
        x = torch.randn(n_in, cin, generator=g).to(torch.bfloat16)
        nbr = None if k == 1 else _rand_rulebook(cap, n_in if kind == "down" else max(n, 1), kind, g)
        if nbr is not None and kind == "subm":
            nbr[n:, 13] = 0                                    # (rows past the count: any valid row)
        y = torch.full((cap, cout), float("nan"), dtype=torch.float32, device=dev)
        n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
        K.spconv_fwd_bf16_raw(x.to(dev), None if nbr is None else nbr.to(dev), n_dev, cap, wp, k, cin, cout, y)
        y2 = torch.full_like(y, float("nan"))
        K.spconv_fwd_bf16_raw(x.to(dev), None if nbr is None else nbr.to(dev), n_dev, cap, wp, k, cin, cout, y2)
        torch.cuda.synchronize()
        assert torch.isnan(y[n:]).all(), (k, cin, cout, n, "rows past the count were written")
        assert torch.equal(y[:n], y2[:n]), (k, cin, cout, n, "two calls differ")
        if n:
            worst = max(worst, _check_conv(y[:n], x.double(), None if nbr is None else nbr[:n].numpy(), wr, (k, cin, cout, n)))
    print("raw conv K=%d %d -> %d: worst |err| / sum|x w| = %.2e (bar %.1e)" % (k, cin, cout, worst, EPS))


# ---- 2. weight-gradient kernel ---------------------------------------------------------------------------------------------------
def _wgrad_case(dev, cin, cout, n, cap, g, empty=()):
    n_in = n + n // 3 + 1
    x = torch.relu(torch.randn(n_in, cin, generator=g)).to(torch.bfloat16)
    dy = torch.randn(cap, cout, generator=g).to(torch.bfloat16)
    nbr = _rand_rulebook(cap, n_in, "down", g, density=0.4)
    for k in empty:
        nbr[:, k] = -1
    return x, dy, nbr


def _check_wgrad(dw, base, x, dy, nbr, n, cap, tag):
    ref, mag, cnt = T16.wgrad64(x.double(), dy[:n].double(), nbr[:n].numpy())
    d = _wgrad_depth(cap, n)
    m = torch.as_tensor(cnt, dtype=torch.float64).view(-1, 1, 1)
    bar = torch.minimum(torch.full_like(m, float(d)), (m - 1).clamp_min(0) + (0 if base is None else 1)) * U
    tot = ref if base is None else ref + base.double()
    amag = mag if base is None else mag + base.double().abs()
    err = (dw.double().cpu() - tot).abs()
    bad = err > bar * amag
    assert not bool(bad.any()), (tag, int(bad.sum()), float((err / amag.clamp_min(1e-300)).max()), d)
    if base is None:
        for k in np.nonzero(cnt == 0)[0]:
            assert int((dw[k] != 0).sum()) == 0, (tag, "offset without pairs", k)
    return cnt


@pytest.mark.parametrize("cin,cout", T16.FWD_PAIRS)
def test_weight_gradient_vs_float64(dev, cin, cout):
    g = torch.Generator().manual_seed(cin + 3 * cout)
    cases = [(n, n + 50, ()) for n in (1, 15, 16, 17, 127, 128, 129)]
    cases += [(200, 260, (0, 1, 2, 5, 20, 26)), (1000, 70000, (7,))]        # offsets without a pair; the > 128-row chunk regime
    for n, cap, empty in cases:
        x, dy, nbr = _wgrad_case(dev, cin, cout, n, cap, g, empty)
        xd, dyd, nd = x.to(dev), dy.to(dev), nbr.to(dev)
        n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
        dw = K.spconv_bwd_weight_bf16(xd, dyd, nd, n_dev, cap, cin, cout)
        dw2 = K.spconv_bwd_weight_bf16(xd, dyd, nd, n_dev, cap, cin, cout, dw=torch.full_like(dw, float("nan")))
        torch.cuda.synchronize()
        assert torch.equal(dw, dw2), (cin, cout, n, "two calls differ")
        cnt = _check_wgrad(dw, None, x, dy, nbr, n, cap, (cin, cout, n, cap))
        assert all(cnt[k] == 0 for k in empty)
        base = torch.randn(27, cin, cout, generator=g)
        acc = K.spconv_bwd_weight_bf16(xd, dyd, nd, n_dev, cap, cin, cout, dw=base.to(dev).clone(), accumulate=True)
        torch.cuda.synchronize()
        _check_wgrad(acc, base, x, dy, nbr, n, cap, (cin, cout, n, cap, "accumulate"))
        for k in empty:
            assert torch.equal(acc[k].cpu(), base[k])


# ---- 3. BatchNorm store variants ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [16, 64])
@pytest.mark.parametrize("n", [1, 63, 4097])
def test_bn_relu_bf16_store_is_the_fp32_result_rounded(dev, n, c):
    g = torch.Generator().manual_seed(n + c)
    x = (torch.randn(n, c, generator=g) * 2 + 0.5).to(dev)
    gamma, beta = (torch.rand(c, generator=g) + 0.5).to(dev), (torch.randn(c, generator=g) * 0.2).to(dev)
    dy = torch.randn(n, c, generator=g).to(dev)
    rm, rv = torch.randn(c, generator=g).to(dev), (torch.rand(c, generator=g) + 0.5).to(dev)
    rm1, rv1, rm2, rv2 = rm.clone(), rv.clone(), rm.clone(), rv.clone()
    y, mean, invstd = K.bn_relu_fwd(x, gamma, beta, rm1, rv1, 0.01, 1e-3)
    yb, mean_b, invstd_b = K.bn_relu_fwd(x, gamma, beta, rm2, rv2, 0.01, 1e-3, out_bf16=True)
    torch.cuda.synchronize()
    assert yb.dtype == torch.bfloat16 and torch.equal(yb.view(torch.int16), y.to(torch.bfloat16).view(torch.int16))
    assert torch.equal(mean, mean_b) and torch.equal(invstd, invstd_b) and torch.equal(rm1, rm2) and torch.equal(rv1, rv2)
    assert not torch.equal(rm1, rm)
    dx, dg, db = K.bn_relu_bwd(x, dy, gamma, beta, mean, invstd)
    dxb, dg_b, db_b = K.bn_relu_bwd(x, dy, gamma, beta, mean, invstd, out_bf16=True)
    torch.cuda.synchronize()
    assert dxb.dtype == torch.bfloat16 and torch.equal(dxb.view(torch.int16), dx.to(torch.bfloat16).view(torch.int16))
    assert torch.equal(dg, dg_b) and torch.equal(db, db_b)


# ---- 4. autograd path ----------------------------------------------------------------------------------------------------------------
def _stack(dev, seed=0):
    torch.manual_seed(seed)
    net = spconv.SparseSequential(
        spconv.SubMConv3d(16, 16, 3, bias=False, indice_key="s0"), nn.BatchNorm1d(16, eps=1e-3, momentum=0.01), nn.ReLU(),
        spconv.SparseConv3d(16, 32, 3, (2, 2, 2), padding=1, bias=False, indice_key="d0"), nn.BatchNorm1d(32, eps=1e-3, momentum=0.01),
        nn.ReLU(), spconv.SubMConv3d(32, 32, 3, bias=False, indice_key="s1")).to(dev).train()
    rng = np.random.default_rng(seed)
    shape = (8, 12, 12)
    idx = np.unique(np.stack([rng.integers(0, 2, 500), rng.integers(0, shape[0], 500), rng.integers(0, shape[1], 500),
                              rng.integers(0, shape[2], 500)], 1).astype(np.int32), axis=0)
    feats = torch.relu(torch.randn(idx.shape[0], 16))
    return net, torch.from_numpy(idx).to(dev), shape, feats.to(dev)


def _run_stack(net, idx, shape, feats, gout=None):
    net.zero_grad()
    f = feats.clone().requires_grad_(True)
    out = net(spconv.SparseConvTensor(f, idx, shape, 2))
    y = out.features
    if gout is None:
        gout = torch.randn(y.shape, generator=torch.Generator().manual_seed(9)).to(y.device)
    (y * gout).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), f.grad, [p.grad for p in net.parameters()], gout


def test_autograd_stack_every_sparse_launch_vs_float64(dev, monkeypatch):
    net, idx, shape, feats = _stack(dev)
    assert 200 <= idx.shape[0] <= 500
    raws, wgs, saved = [], [], []
    raw0, wg0 = K.spconv_fwd_bf16_raw, K.spconv_bwd_weight_bf16

    def raw(x, nbr, n_ptr, cap, wp, k, cin, cout, y=None):
        out = raw0(x, nbr, n_ptr, cap, wp, k, cin, cout, y)
        raws.append((x.clone(), None if nbr is None else nbr.clone(), int(n_ptr.item()), wp.clone(), k, cin, cout, out.clone()))
        return out

    def wg(x, dy, nbr, n_ptr, cap, cin, cout, dw=None, accumulate=False):
        out = wg0(x, dy, nbr, n_ptr, cap, cin, cout, dw, accumulate)
        wgs.append((x.clone(), dy.clone(), nbr.clone(), int(n_ptr.item()), cap, cin, cout, out.clone()))
        return out
    monkeypatch.setattr(K, "spconv_fwd_bf16_raw", raw)
    monkeypatch.setattr(K, "spconv_bwd_weight_bf16", wg)
    fwd0 = AG._sparse_bf16_fwd
    monkeypatch.setattr(AG, "_sparse_bf16_fwd", lambda ctx, xb, *a: saved.append(xb) or fwd0(ctx, xb, *a))
    WI.store.clear()
    with AG.sparse_precision_scope("bf16"):
        y, dfeat, grads, _ = _run_stack(net, idx, shape, feats)
    assert AG.sparse_precision() == "fp32"
    assert y.dtype == torch.float32 and dfeat.dtype == torch.float32 and bool(torch.isfinite(y).all())
    assert all(gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().sum()) > 0 for gr in grads), "a parameter without gradient"
    assert float(dfeat.abs().sum()) > 0
    assert len(saved) == 3 and all(s.dtype == torch.bfloat16 for s in saved), "saved conv operands are bf16"
    # 3 forward + 3 data-gradient launches (submanifold ones on the forward table), 3 weight gradients
    assert [(r[5], r[6]) for r in raws] == [(16, 16), (16, 32), (32, 32), (32, 32), (32, 16), (16, 16)]
    assert sorted((w_[5], w_[6]) for w_ in wgs) == [(16, 16), (16, 32), (32, 32)]
    for x, nbr, n, wp, k, cin, cout, out in raws:
        w64 = wp.view(torch.bfloat16).view(k, cout, cin).transpose(1, 2).double().cpu()
        _check_conv(out[:n].cpu(), x.double().cpu(), nbr[:n].cpu().numpy(), w64, ("launch", cin, cout))
    for x, dy, nbr, n, cap, cin, cout, out in wgs:
        assert x.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16
        _check_wgrad(out.cpu(), None, x.cpu(), dy.cpu(), nbr.cpu(), n, cap, ("launch wgrad", cin, cout))
    # the forward images are the master weights rounded once; the data-gradient images their transposes (offsets reversed for
    # the submanifold layers)
    convs = [m for m in net if isinstance(m, spconv.SparseConvolution)]
    for i, m in enumerate(convs):
        wr = round_bf16(m.weight.detach().view(27, m.in_channels, m.out_channels).cpu())
        assert torch.equal(raws[i][3].view(torch.bfloat16).view(27, m.out_channels, m.in_channels).cpu().float(), wr.transpose(1, 2))
        bw = raws[5 - i][3].view(torch.bfloat16).view(27, m.in_channels, m.out_channels).cpu().float()
        assert torch.equal(bw, wr.flip(0) if m.subm else wr), i
    WI.store.clear()


def test_mode_off_stack_equals_the_fp32_kernels_called_directly(dev):
    net, idx, shape, feats = _stack(dev, 1)
    with AG.sparse_precision_scope("bf16"):                    # a toggle first: nothing of it may stay behind
        _run_stack(net, idx, shape, feats)
    WI.store.clear()
    c0, b0, _, c1, b1, _, c2 = list(net)
    rs = [(b.running_mean.clone(), b.running_var.clone()) for b in (b0, b1)]
    y, dfeat, grads, gout = _run_stack(net, idx, shape, feats)
    for b, (m_, v_) in zip((b0, b1), rs):
        b.running_mean.copy_(m_); b.running_var.copy_(v_)
    # the same five layers by hand on today's entry points
    inp = spconv.SparseConvTensor(feats, idx, shape, 2)
    _, nbr0, _, _ = c0.book(inp)
    oi, nbr1, oshape, _ = c1.book(inp)
    mid = spconv.SparseConvTensor(None, oi, oshape, 2)
    _, nbr2, _, _ = c2.book(mid)
    n0, n1 = idx.shape[0], oi.shape[0]
    p = lambda n: AG._n_ptr(n, dev)                                                        # noqa: E731
    w = [c.weight.detach().view(27, c.in_channels, c.out_channels).contiguous() for c in (c0, c1, c2)]
    r0 = K.spconv_fwd(feats, nbr0, p(n0), n0, K.spconv_pack_weight(w[0]), 27, 16, 16)
    a0, m0, i0 = K.bn_relu_fwd(r0, b0.weight.detach(), b0.bias.detach(), b0.running_mean, b0.running_var, 0.01, 1e-3)
    r1 = K.spconv_fwd(a0, nbr1, p(n1), n1, K.spconv_pack_weight(w[1]), 27, 16, 32)
    a1, m1, i1 = K.bn_relu_fwd(r1, b1.weight.detach(), b1.bias.detach(), b1.running_mean, b1.running_var, 0.01, 1e-3)
    r2 = K.spconv_fwd(a1, nbr2, p(n1), n1, K.spconv_pack_weight(w[2]), 27, 32, 32)
    assert torch.equal(y, r2[:n1])
    dw2 = K.spconv_bwd_weight(a1, gout, nbr2, p(n1), nbr2.shape[0], 32, 32)
    da1 = K.spconv_bwd_data(gout, nbr2, p(n1), nbr2.shape[0], K.spconv_pack_weight_t(w[2].flip(0).contiguous()), 27, 32, 32)[:n1]
    dr1, dg1, db1 = K.bn_relu_bwd(r1, da1.contiguous(), b1.weight.detach(), b1.bias.detach(), m1, i1)
    dw1 = K.spconv_bwd_weight(a0, dr1, nbr1, p(n1), nbr1.shape[0], 16, 32)
    nbr1_t = K.rulebook_transpose(nbr1, p(n1), nbr1.shape[0], n0)
    da0 = K.spconv_bwd_data(dr1, nbr1_t, p(n0), n0, K.spconv_pack_weight_t(w[1]), 27, 16, 32)[:n0]
    dr0, dg0, db0 = K.bn_relu_bwd(r0, da0.contiguous(), b0.weight.detach(), b0.bias.detach(), m0, i0)
    dw0 = K.spconv_bwd_weight(feats, dr0, nbr0, p(n0), nbr0.shape[0], 16, 16)
    dx = K.spconv_bwd_data(dr0, nbr0, p(n0), nbr0.shape[0], K.spconv_pack_weight_t(w[0].flip(0).contiguous()), 27, 16, 16)[:n0]
    torch.cuda.synchronize()
    want = [dw0.view_as(c0.weight), dg0, db0, dw1.view_as(c1.weight), dg1, db1, dw2.view_as(c2.weight)]
    assert torch.equal(dfeat, dx)
    for i, (got, ref) in enumerate(zip(grads, want)):
        assert torch.equal(got, ref), i


def test_unsupported_layer_shape_is_an_error_that_names_the_layer(dev):
    conv = spconv.SubMConv3d(48, 64, 3, bias=False, indice_key="odd48").to(dev)
    idx = torch.tensor([[0, 1, 1, 1], [0, 1, 2, 1]], dtype=torch.int32, device=dev)
    x = spconv.SparseConvTensor(torch.randn(2, 48, device=dev, requires_grad=True), idx, (4, 4, 4), 1)
    with AG.sparse_precision_scope("bf16"):
        with pytest.raises(ValueError, match="odd48"):
            conv(x)
