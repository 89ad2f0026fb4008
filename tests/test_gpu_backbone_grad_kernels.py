"""-m gpu: the fp32 backbone gradient kernels alone, against the float64 references of backbone_grad_cases.py -- the sparse weight
gradient in both formulations, the rulebook transpose and the data gradient; the two BatchNorm + ReLU pairs and bn2d_stats; the
dense weight gradient in fp32, bf16 and bf16 with BatchNorm + ReLU in its loader.  Bars, margins and measured figures: the
docstring of backbone_grad_cases.py.  (These cases found one bug: with 2 .. 4 rows bn_relu_fwd lost up to 1.9e-5 of its variance and
6.2e-6 of y -- n = 2 at every C -- to the fp32 rounding of x^2; bn_finalize_kernel now takes the exact re-based sums there.)  No case holds an index outside its tensor or a NaN in anything that selects an address."""
import numpy as np
import pytest
import torch

from sassd import kernels as K
import backbone_grad_cases as BG
from backbone_grad_cases import figure, bar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _leave_the_process_as_found():
    """This file grows the shared sparse weight-gradient workspace to capacities of 70 000, 317 000 and 557 056 rows; what it cached
    (kernel workspaces, allocator blocks) is dropped at the end, so the test files after it start from the memory they always had."""
    before = dict(K._ws_cache)
    yield
    for key in [k for k, t in K._ws_cache.items() if before.get(k) is not t]:
        del K._ws_cache[key]
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _n(n, dev):
    return torch.tensor([n], dtype=torch.int32, device=dev)


class Worst(dict):
    """family -> (largest figure, its bar)"""

    def add(self, fam, fig, lim):
        def ratio(f, b):
            return f / b if b > 0 else (0.0 if f == 0 else float("inf"))
        if fam not in self or ratio(fig, lim) >= ratio(*self[fam]):
            self[fam] = (fig, lim)

    def show(self, title):
        for fam, (fig, lim) in self.items():
            print("%s | %-28s | largest figure %.2e | bar %.2e" % (title, fam, fig, lim))


# ---- A. sparse fp32 gradients ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", BG.WGRAD_PAIRS)
def test_sparse_weight_gradient_vs_float64(dev, cin, cout):
    worst = Worst()
    g = torch.Generator().manual_seed(cin + 5 * cout)
    for fam, n, cap, kind, empty, counts in BG.wgrad_cases(cin, cout):
        x, dy, nbr, n_in = BG.wgrad_case(cin, cout, n, cap, kind, empty, counts)
        xd, dyd, nd, n_dev = x.to(dev), dy.to(dev), nbr.to(dev), _n(n, dev)
        base = torch.randn(27, cin, cout, generator=g)
        for tile in (False, True):
            tag = (fam, n, cap, kind, "tile per wave" if tile else "offset per wave")
            with K.default_cfg(spconv=32 if tile else 0):
                dw = K.spconv_bwd_weight(xd, dyd, nd, n_dev, cap, cin, cout)
                dw2 = K.spconv_bwd_weight(xd, dyd, nd, n_dev, cap, cin, cout, dw=torch.full_like(dw, float("nan")))
                acc = K.spconv_bwd_weight(xd, dyd, nd, n_dev, cap, cin, cout, dw=base.to(dev).clone(), accumulate=True)
            torch.cuda.synchronize()
            assert torch.equal(dw, dw2), (tag, "a second call into a NaN-filled dw differs")
            d = BG.wgrad_depth(n, cap, tile)
            fig, lim, bad, cnt = BG.wgrad_check(dw.cpu(), None, x, dy, nbr, n, d)
            assert bad == 0, (tag, bad, fig, lim)
            worst.add(fam + (", tile" if tile else ""), fig, lim)
            assert all(cnt[k] == 0 for k in empty)
            for k in np.flatnonzero(cnt == 0):
                assert int((dw[k] != 0).sum()) == 0, (tag, "an offset without pairs is not exactly 0", int(k))
                assert torch.equal(acc[k].cpu(), base[k]), (tag, "accumulate moved an offset without pairs", int(k))
            fig, lim, bad, _ = BG.wgrad_check(acc.cpu(), base, x, dy, nbr, n, d)
            assert bad == 0, (tag, "accumulate", bad, fig, lim)
            worst.add("accumulate" + (", tile" if tile else ""), fig, lim)
    worst.show("sparse wgrad %d -> %d" % (cin, cout))


@pytest.mark.parametrize("cin,cout", BG.DGRAD_LAYERS)
def test_rulebook_transpose_and_sparse_data_gradient_vs_float64(dev, cin, cout):
    worst = Worst()
    for n_in in BG.DGRAD_ROWS:
        for kind in ("down",) + (("subm",) if cin == cout else ()):
            dy, w, nbr, n_out, cap_in = BG.dgrad_case(cin, cout, n_in, kind)
            cap_out = nbr.shape[0]
            ref, mag, pairs, t = BG.dgrad_ref(dy, nbr, w, n_out, n_in)
            dyd, nd, wd = dy.to(dev), nbr.to(dev), w.to(dev)
            nbr_t = K.rulebook_transpose(nd, _n(n_out, dev), cap_out, cap_in)
            assert torch.equal(nbr_t[:n_in].cpu().long(), torch.from_numpy(t)), (kind, n_in, "transposed table")
            assert bool((nbr_t[n_in:] == -1).all())
            wt = K.spconv_pack_weight_t(wd)
            dx = K.spconv_bwd_data(dyd, nbr_t, _n(n_in, dev), cap_in, wt, 27, cin, cout)
            dx2 = K.spconv_bwd_data(dyd, nbr_t, _n(n_in, dev), cap_in, wt, 27, cin, cout)
            torch.cuda.synchronize()
            assert torch.equal(dx[:n_in], dx2[:n_in]), (kind, n_in, "two calls differ")
            fig, lim, bad = BG.dgrad_check(dx[:n_in].cpu(), ref, mag, pairs, cout)
            assert bad == 0, (kind, n_in, bad, fig, lim)
            worst.add("transposed table, " + kind, fig, lim)
            if kind == "subm":                           # the forward table with the offset-reversed image: the same sum
                wr = K.spconv_pack_weight_t(wd.flip(0).contiguous())
                dxf = K.spconv_bwd_data(dyd, nd, _n(n_in, dev), cap_out, wr, 27, cin, cout)
                torch.cuda.synchronize()
                fig, lim, bad = BG.dgrad_check(dxf[:n_in].cpu(), ref, mag, pairs, cout)
                assert bad == 0, ("forward table", n_in, bad, fig, lim)
                worst.add("forward table, subm", fig, lim)
    worst.show("sparse dgrad layer %d -> %d" % (cin, cout))


# ---- B. BatchNorm + ReLU pairs --------------------------------------------------------------------------------------------------
def _odd_views(dev, gamma, beta):
    """gamma / beta as views at odd 4-byte offsets into one buffer (the flat parameter buffer of training hands out such views)"""
    c = len(gamma)
    buf = torch.zeros(2 * c + 4, dtype=torch.float32)
    buf[1:1 + c] = torch.from_numpy(gamma)
    buf[c + 3:2 * c + 3] = torch.from_numpy(beta)
    buf = buf.to(dev)
    gv, bv = buf[1:1 + c], buf[c + 3:2 * c + 3]
    assert gv.data_ptr() % 8 == 4 and bv.data_ptr() % 8 == 4 and gv.is_contiguous()
    return gv, bv


def _bn_compare(worst, fam, got, k, tag):
    ref = BG.bn_ref(k["x"], k["gamma"], k["beta"], k["dy"], k["rm"], k["rv"])
    twin = BG.bn_ref(k["x"], k["gamma"], k["beta"], k["dy"], k["rm"], k["rv"], dt=np.float32)
    figs, tfigs = BG.bn_figures(got, ref), BG.bn_figures(BG.bn_twin_as_got(twin), ref)
    for name, fig in figs.items():
        lim = bar(tfigs[name])
        worst.add(fam + " " + name, fig, lim)
        assert fig <= lim, (tag, name, fig, lim, "fp32 twin", tfigs[name])
    return ref


def _np(t):
    return t.detach().double().cpu().numpy()


def _bn1d_check(dev, worst, fam, n, c, cancel=False):
    k = BG.bn1d_case(n, c, cancel)
    x = torch.from_numpy(np.ascontiguousarray(k["x"].T)).to(dev)
    dy = torch.from_numpy(np.ascontiguousarray(k["dy"].T)).to(dev)
    gamma, beta = _odd_views(dev, k["gamma"], k["beta"])
    rm, rv = torch.from_numpy(k["rm"]).clone().to(dev), torch.from_numpy(k["rv"]).clone().to(dev)
    rm2, rv2 = rm.clone(), rv.clone()
    y, mean, invstd = K.bn_relu_fwd(x, gamma, beta, rm, rv, BG.MOMENTUM, BG.EPS_BN)
    y2, mean2, invstd2 = K.bn_relu_fwd(x, gamma, beta, rm2, rv2, BG.MOMENTUM, BG.EPS_BN)
    y3, mean3, invstd3 = K.bn_relu_fwd(x, gamma, beta, None, None, BG.MOMENTUM, BG.EPS_BN)
    dx, dg, db = K.bn_relu_bwd(x, dy, gamma, beta, mean, invstd)
    dx2, dg2, db2 = K.bn_relu_bwd(x, dy, gamma, beta, mean, invstd)
    torch.cuda.synchronize()
    tag = ("bn1d", n, c, cancel)
    for a, b in ((y, y2), (mean, mean2), (invstd, invstd2), (rm, rm2), (rv, rv2), (y, y3), (mean, mean3), (invstd, invstd3), (dx, dx2),
                 (dg, dg2), (db, db2)):
        assert torch.equal(a, b), (tag, "a repeated call, or one without running statistics, differs")
    got = dict(y=y.t().contiguous().cpu().numpy(), mean=_np(mean), var=1.0 / _np(invstd) ** 2, rmean=_np(rm), rvar=_np(rv),
               dbeta=_np(db), dgamma=_np(dg), dx=dx.t().contiguous().cpu().numpy())
    ref = _bn_compare(worst, fam, got, k, tag)
    if n == 1:                                           # what torch refuses
        assert torch.equal(invstd.cpu(), torch.full((c,), np.float32(1.0 / np.sqrt(BG.EPS_BN))))
        assert torch.equal(y.cpu()[0], torch.relu(torch.from_numpy(k["beta"]))) and int((dx != 0).sum()) == 0
        assert torch.equal(mean.cpu(), torch.from_numpy(k["x"][:, 0]))
        assert np.all(ref["var"] == 0)                   # ... so the running variance compared above is the biased form's


@pytest.mark.parametrize("c", sorted(BG.BN1D_ROWS))
def test_bn_relu_1d_vs_float64(dev, c):
    worst = Worst()
    for n in BG.BN1D_ROWS[c]:
        _bn1d_check(dev, worst, "rows", n, c)
    worst.show("bn_relu C = %d" % c)


@pytest.mark.parametrize("n,c", BG.BN1D_CANCEL)
def test_bn_relu_1d_cancelling_channels_and_the_block_cap_vs_float64(dev, n, c):
    worst = Worst()
    nb, rpb, rpt = BG.bn_blocks(n, c)
    _bn1d_check(dev, worst, "cancelling, %d rows per thread" % rpt, n, c, True)
    worst.show("bn_relu (%d, %d)" % (n, c))


@pytest.mark.parametrize("shape", BG.BN2D_SHAPES)
def test_bn2d_relu_and_stats_vs_float64(dev, shape):
    worst = Worst()
    k = BG.bn2d_case(shape)
    x, dy = torch.from_numpy(BG.to_nchw(k["x"], shape)).to(dev), torch.from_numpy(BG.to_nchw(k["dy"], shape)).to(dev)
    gamma, beta = torch.from_numpy(k["gamma"]).to(dev), torch.from_numpy(k["beta"]).to(dev)
    rm, rv = torch.from_numpy(k["rm"]).clone().to(dev), torch.from_numpy(k["rv"]).clone().to(dev)
    rm2, rv2, rm3, rv3 = rm.clone(), rv.clone(), rm.clone(), rv.clone()
    y, mean, invstd = K.bn2d_relu_fwd(x, gamma, beta, rm, rv, BG.MOMENTUM, BG.EPS_BN)
    y2, mean2, invstd2 = K.bn2d_relu_fwd(x, gamma, beta, rm2, rv2, BG.MOMENTUM, BG.EPS_BN)
    y3, mean3, invstd3 = K.bn2d_relu_fwd(x, gamma, beta, None, None, BG.MOMENTUM, BG.EPS_BN)
    smean, sinvstd, aff = K.bn2d_stats(x, gamma, beta, rm3, rv3, BG.MOMENTUM, BG.EPS_BN)
    dx, dg, db = K.bn2d_relu_bwd(x, dy, gamma, beta, mean, invstd)
    dx2, dg2, db2 = K.bn2d_relu_bwd(x, dy, gamma, beta, mean, invstd)
    torch.cuda.synchronize()
    for a, b in ((y, y2), (mean, mean2), (invstd, invstd2), (rm, rm2), (rv, rv2), (y, y3), (mean, mean3), (invstd, invstd3), (dx, dx2),
                 (dg, dg2), (db, db2)):
        assert torch.equal(a, b), (shape, "a repeated call, or one without running statistics, differs")
    # bn2d_stats: the pair's statistics bit for bit, and the affine triple formed from them
    assert torch.equal(smean, mean) and torch.equal(sinvstd, invstd) and torch.equal(rm3, rm) and torch.equal(rv3, rv), shape
    assert torch.equal(aff, torch.stack([mean, invstd * gamma, beta])), shape
    cm = lambda t: t.transpose(0, 1).reshape(shape[1], -1).cpu().numpy()             # noqa: E731  (channel-major, as the cases are)
    got = dict(y=cm(y), mean=_np(mean), var=1.0 / _np(invstd) ** 2, rmean=_np(rm), rvar=_np(rv), dbeta=_np(db), dgamma=_np(dg),
               dx=cm(dx))
    S, chunk, per = BG.BN2D_REGIME[shape]
    _bn_compare(worst, "S = %d, chunk %d" % (S, chunk), got, k, shape)
    worst.show("bn2d_relu %s" % (shape,))


# ---- C. dense weight gradient, per element --------------------------------------------------------------------------------------
def _dense_check(worst, fam, got, ref, scale, twin, tag):
    fig = figure(got.double().cpu().numpy(), ref.numpy(), scale.numpy())
    lim = bar(figure(twin.double().numpy(), ref.numpy(), scale.numpy()))
    worst.add(fam, fig, lim)
    assert fig <= lim, (tag, fig, lim)


def _dense_family(dev, worst, fam, shapes, accumulate, call, operands, kss=(3, 1)):
    """call(x, dy, ks, dw, accumulate) -> dw on the device; operands(x, dy) -> what the reference multiplies"""
    g = torch.Generator().manual_seed(3)
    for shape in shapes:
        b, cin, cout, h, w = shape
        for ks in kss:
            x, dy = BG.dense_case(shape)
            xr, dyr = operands(x, dy)
            xd, dyd = x.to(dev), dy.to(dev)
            got = call(xd, dyd, ks, None, False)
            again = call(xd, dyd, ks, torch.full_like(got, float("nan")), False)
            torch.cuda.synchronize()
            assert torch.equal(got, again), (fam, shape, ks, "a second call into a NaN-filled dw differs")
            _dense_check(worst, fam + " k=%d" % ks, got, *BG.dense_refs(xr, dyr, ks), (fam, shape, ks))
            for ky, kx in BG.dead_taps(h, w, ks):
                assert int((got[:, :, ky, kx] != 0).sum()) == 0, (fam, shape, "a tap that reaches no pixel", ky, kx)
            if shape in accumulate:
                base = torch.randn(cout, cin, ks, ks, generator=g)
                acc = call(xd, dyd, ks, base.to(dev).clone(), True)
                torch.cuda.synchronize()
                _dense_check(worst, fam + " k=%d accumulate" % ks, acc, *BG.dense_refs(xr, dyr, ks, base), (fam, shape, ks, "accumulate"))
                for ky, kx in BG.dead_taps(h, w, ks):
                    assert torch.equal(acc[:, :, ky, kx].cpu(), base[:, :, ky, kx])


def test_dense_weight_gradient_fp32_per_element(dev):
    worst = Worst()
    _dense_family(dev, worst, "fp32", BG.DENSE_SHAPES, BG.DENSE_ACCUMULATE,
                  lambda x, dy, ks, dw, acc: K.conv2d_bwd_weight(x, dy, ks, dw=dw, accumulate=acc), lambda x, dy: (x, dy))
    worst.show("conv2d_bwd_weight")


def test_dense_weight_gradient_bf16_per_element(dev):
    worst = Worst()
    _dense_family(dev, worst, "bf16", BG.DENSE_SHAPES_BF16, BG.DENSE_ACCUMULATE_BF16,
                  lambda x, dy, ks, dw, acc: K.conv2d_bwd_weight(x, dy, ks, dw=dw, accumulate=acc, bf16=True),
                  lambda x, dy: (BG.bf16r(x), BG.bf16r(dy)))
    worst.show("conv2d_bwd_weight bf16")


def test_dense_weight_gradient_bf16_bnrelu_per_element(dev):
    """X = relu(batchnorm(x)) formed in the loader from the affine triple of bn2d_stats (a host-made triple where H * W is no
    multiple of 4, which bn2d_stats does not take)"""
    worst = Worst()
    r = np.random.default_rng(11)
    affs = {}

    def affine(x):
        cin = x.shape[1]
        if cin not in affs:
            affs[cin] = (torch.from_numpy(r.uniform(0.5, 1.5, cin).astype(np.float32)), torch.from_numpy(r.uniform(-0.3, 0.3, cin).astype(np.float32)))
        gamma, beta = affs[cin]
        if (x.shape[2] * x.shape[3]) % 4 == 0:
            return K.bn2d_stats(x.to(dev), gamma.to(dev), beta.to(dev), None, None, BG.MOMENTUM, BG.EPS_BN)[2]
        return BG.host_affine(x.cpu(), gamma, beta).to(dev)

    _dense_family(dev, worst, "bf16 bnrelu", BG.DENSE_SHAPES_BF16, BG.DENSE_ACCUMULATE_BF16,
                  lambda x, dy, ks, dw, acc: K.conv2d_bwd_weight(x, dy, ks, dw=dw, accumulate=acc, bf16=True, x_affine=affine(x)),
                  lambda x, dy: (BG.bf16r(BG.bn_affine_operand(x, affine(x).cpu())), BG.bf16r(dy)), kss=(3,))
    worst.show("conv2d_bwd_weight bf16 bnrelu")
