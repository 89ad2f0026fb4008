"""backbone_grad_cases.py without a GPU: its float64 references against torch float64 autograd, the margins and index ranges its
builders promise, the regime every case is named for, and its restatement of the host geometry against what the library tells."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sassd  # noqa: F401
from sassd import _C
from oracle import nets as onets
import backbone_grad_cases as BG
from test_bf16_sparse_train_cpu import dgrad64, wgrad64, R


# ---- references -------------------------------------------------------------------------------------------------------------
def _close(a, b, scale):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.all(np.abs(a - b) <= 1e-12 * np.maximum(np.asarray(scale, np.float64), 1e-300)), float(np.abs(a - b).max())


@pytest.mark.parametrize("n,c", [(2, 4), (3, 16), (65, 16), (513, 64)])
def test_bn_reference_is_torch_float64_autograd(n, c):
    k = BG.bn1d_case(n, c)
    ref = BG.bn_ref(k["x"], k["gamma"], k["beta"], k["dy"], k["rm"], k["rv"])
    x = torch.from_numpy(k["x"].T.copy()).double().requires_grad_(True)
    g, b = (torch.from_numpy(k[s]).double().requires_grad_(True) for s in ("gamma", "beta"))
    rm, rv = torch.from_numpy(k["rm"]).double(), torch.from_numpy(k["rv"]).double()
    y = torch.relu(F.batch_norm(x, rm, rv, g, b, True, BG.MOMENTUM, BG.EPS_BN))
    y.backward(torch.from_numpy(k["dy"].T.copy()).double())
    _close(ref["y"].T, y.detach(), np.abs(ref["y"]).max())
    _close(ref["dx"].T, x.grad, np.abs(ref["dx"]).max())
    _close(ref["dbeta"], b.grad, ref["s_dbeta"])
    _close(ref["dgamma"], g.grad, ref["s_dgamma"])
    _close(ref["rmean"], rm, ref["s_rmean"])
    _close(ref["rvar"], rv, ref["s_rvar"])
    x64 = k["x"].astype(np.float64)
    _close(ref["mean"], x64.mean(1), ref["s_mean"])
    _close(ref["var"], x64.var(1), ref["s_var"])


def test_bn_reference_2d_layout_and_one_row():
    shape = (2, 3, 2, 6)
    k = BG.bn2d_case(shape)
    ref = BG.bn_ref(k["x"], k["gamma"], k["beta"], k["dy"], k["rm"], k["rv"])
    x = torch.from_numpy(BG.to_nchw(k["x"], shape)).double().requires_grad_(True)
    assert np.array_equal(BG.from_nchw(x.detach().numpy()), k["x"].astype(np.float64))
    rm, rv = torch.from_numpy(k["rm"]).double(), torch.from_numpy(k["rv"]).double()
    y = torch.relu(F.batch_norm(x, rm, rv, torch.from_numpy(k["gamma"]).double(), torch.from_numpy(k["beta"]).double(), True,
                                BG.MOMENTUM, BG.EPS_BN))
    y.backward(torch.from_numpy(BG.to_nchw(k["dy"], shape)).double())
    _close(BG.to_nchw(ref["y"], shape), y.detach(), np.abs(ref["y"]).max())
    _close(BG.to_nchw(ref["dx"], shape), x.grad, np.abs(ref["dx"]).max())
    _close(ref["rvar"], rv, ref["s_rvar"])
    # N = 1 (torch refuses it): invstd = 1 / sqrt(eps), y = relu(beta), dx = 0, the running variance takes the biased form
    k = BG.bn1d_case(1, 16)
    ref = BG.bn_ref(k["x"], k["gamma"], k["beta"], k["dy"], k["rm"], k["rv"])
    assert np.all(ref["invstd"] == 1.0 / np.sqrt(BG.EPS_BN)) and np.all(ref["dx"] == 0) and np.all(ref["var"] == 0)
    assert np.array_equal(ref["y"][:, 0], np.maximum(k["beta"].astype(np.float64), 0))
    _close(ref["rvar"], (1 - BG.MOMENTUM) * k["rv"].astype(np.float64), 1.0)
    assert np.abs(k["beta"]).min() >= 0.05


def test_sparse_references_are_float64_autograd_and_the_oracle():
    for kind in ("down", "subm"):
        dy, w, nbr, n_out, cap_in = BG.dgrad_case(32, 16, 257, kind)
        n_in = cap_in - 50
        g = torch.Generator().manual_seed(5)
        x = BG.q12(torch.randn(n_in, 32, generator=g))
        nb = nbr[:n_out].long()
        xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
        y = torch.zeros(n_out, 16, dtype=torch.float64)
        for k in range(27):
            o = torch.nonzero(nb[:, k] >= 0).view(-1)
            y = y.index_add(0, o, xr[nb[o, k]] @ wr[k])
        y.backward(dy[:n_out].double())
        dx, mag, pairs, t = BG.dgrad_ref(dy, nbr, w, n_out, n_in)
        dw, wmag, cnt = wgrad64(x.double(), dy[:n_out].double(), nbr[:n_out].numpy())
        _close(dx, xr.grad, mag.numpy() + 1e-300)
        _close(dw, wr.grad, wmag.numpy() + 1e-300)
        assert np.array_equal(dx.numpy(), dgrad64(dy[:n_out].double(), nbr[:n_out].numpy(), R(w).float(), n_in)[0].numpy()) or \
            not torch.equal(R(w).float(), w)                     # (dgrad64 rounds the weight to bf16: equal where that is a no-op)
        # through oracle.nets.sparse_conv (fp32): on small integers every fp32 sum is exact
        xi = torch.randint(-4, 5, (n_in, 32), generator=g).float()
        wi = torch.randint(-3, 4, (27, 32, 16), generator=g).float()
        di = torch.randint(-4, 5, (nbr.shape[0], 16), generator=g).float()
        xq, wq = xi.clone().requires_grad_(True), wi.clone().requires_grad_(True)
        onets.sparse_conv(xq, nbr[:n_out].numpy(), wq).backward(di[:n_out])
        assert torch.equal(BG.dgrad_ref(di, nbr, wi, n_out, n_in)[0], xq.grad.double())
        assert torch.equal(wgrad64(xi.double(), di[:n_out].double(), nbr[:n_out].numpy())[0], wq.grad.double())
        if kind == "subm":                                       # the forward-table form is the same sum on a symmetric table
            fw = BG.sparse_conv64(dy[:n_out].double(), nbr[:n_out].numpy(), w.double().flip(0).transpose(1, 2).contiguous())[0]
            _close(fw, dx, mag.numpy() + 1e-300)


def test_dense_reference_is_the_sum_it_names():
    for shape, ks in (((2, 5, 6, 2, 1), 3), ((1, 3, 2, 3, 45), 3), ((1, 3, 2, 1, 7), 1)):
        x, dy = BG.dense_case(shape)
        ref, scale, twin = BG.dense_refs(x, dy, ks)
        xp = F.pad(x.double(), (ks // 2,) * 4)
        h, w = shape[3], shape[4]
        want = torch.stack([torch.stack([torch.einsum("bohw,bihw->oi", dy.double(), xp[:, :, ky:ky + h, kx:kx + w])
                                         for kx in range(ks)], -1) for ky in range(ks)], -2)
        _close(ref, want, scale.numpy() + 1e-300)
        assert bool((scale >= ref.abs() - 1e-12).all())
        assert BG.figure(twin.numpy(), ref.numpy(), scale.numpy()) < 64 * BG.U
        for ky, kx in BG.dead_taps(h, w, ks):
            assert float(scale[:, :, ky, kx].abs().max()) == 0
    assert len(BG.dead_taps(1, 7, 3)) == 6 and len(BG.dead_taps(2, 1, 3)) == 6 and len(BG.dead_taps(1, 1, 3)) == 8
    assert BG.dead_taps(2, 2, 3) == [] and BG.dead_taps(1, 1, 1) == []


# ---- builders ---------------------------------------------------------------------------------------------------------------
def _all_bn_cases():
    for c, rows in BG.BN1D_ROWS.items():
        for n in rows:
            yield ("1d", n, c, False), BG.bn1d_case(n, c)
    for n, c in BG.BN1D_CANCEL:
        yield ("1d", n, c, True), BG.bn1d_case(n, c, True)
    for shape in BG.BN2D_SHAPES:
        yield ("2d",) + shape, BG.bn2d_case(shape)


def test_z_margin_holds_in_every_bn_case_and_the_loop_converged():
    most = 0
    for tag, k in _all_bn_cases():
        z, mar = BG.z_margin(k["x"], k["gamma"], k["beta"])
        assert np.all(np.abs(z) >= mar[:, None]), tag
        assert np.all(mar > 0) and np.all(mar >= BG.Z_ULPS * BG.U * np.abs(k["beta"]).astype(np.float64)), tag
        assert np.abs(k["beta"]).min() >= 0.05 and np.abs(k["gamma"]).min() >= 0.5, tag
        assert k["rounds"] <= 20, tag
        most = max(most, k["rounds"])
        assert 0 < (z > 0).mean() < 1 or z.shape[1] == 1 or z.size < 8, tag           # both sides of the ReLU are there
    print("margin rounds at most", most)
    k = BG.bn1d_case(70001, 256, True)                           # the cancelling channels are still what they are named for
    x = k["x"].astype(np.float64)
    for c in BG.CANCEL_1D[:2]:
        assert x[c].mean() ** 2 > 1024 * x[c].var(), c
    assert x[BG.CANCEL_1D[2], 0] == 3.0 and x[BG.CANCEL_1D[2], 1:].std() < 2e-3        # near-constant behind an outlier first row
    k = BG.bn2d_case(BG.BN2D_SHAPES[-1])
    x = k["x"].astype(np.float64)
    for c in BG.CANCEL_2D:
        assert x[c].mean() ** 2 > 1024 * x[c].var(), c
    assert x[0].mean() ** 2 < 1024 * x[0].var()


def test_sparse_tables_hold_what_their_cases_promise():
    for cin, cout in BG.WGRAD_PAIRS:
        for fam, n, cap, kind, empty, counts in BG.wgrad_cases(cin, cout):
            x, dy, nbr, n_in = BG.wgrad_case(cin, cout, n, cap, kind, empty, counts)
            assert nbr.shape == (cap, 27) and nbr.dtype == torch.int32 and x.shape == (n_in, cin) and dy.shape == (cap, cout)
            assert int(nbr.min()) >= -1 and int(nbr.max()) < n_in, (fam, n)            # rows past the count included
            live = nbr[:n][nbr[:n] >= 0].long()
            assert bool(torch.isfinite(x[live]).all()) and bool(torch.isfinite(dy[:n]).all()) and bool(torch.isnan(dy[n:]).all())
            cnt = (nbr[:n] >= 0).sum(0).numpy()
            assert all(cnt[k] == 0 for k in empty), fam
            assert bool((nbr[:, list(empty)] == -1).all())
            for k, c in (counts or ()):
                assert cnt[k] == c and int((nbr[:128, k] >= 0).sum()) == c, (fam, k)
            if kind == "subm":
                assert torch.equal(nbr[:n, 13], torch.arange(n, dtype=torch.int32)) and bool((nbr[n:, 13] == 0).all())
            assert torch.equal(BG.q12(x[live]), x[live]) and torch.equal(BG.q12(dy[:n]), dy[:n])
    assert sorted(c % 4 for c in BG.MOD4_COUNTS.values()) == [0, 1, 1, 2, 2, 3, 3]
    a, b = BG.q12(torch.tensor([1.0 + 2.0 ** -11, 3.1415926])), BG.q12(torch.tensor([1.0 - 2.0 ** -12, -2.7182818]))
    assert torch.equal((a * b).double(), a.double() * b.double())                     # 12 x 12 bits: exact in fp32
    for cin, cout in BG.DGRAD_LAYERS:
        for n_in in BG.DGRAD_ROWS:
            for kind in ("down",) + (("subm",) if cin == cout else ()):
                dy, w, nbr, n_out, cap_in = BG.dgrad_case(cin, cout, n_in, kind)
                assert int(nbr.min()) >= -1 and int(nbr.max()) < n_in and cap_in > n_in and nbr.shape[0] > n_out
                t = nbr[:n_out].numpy()
                for k in range(27):
                    col = t[:, k][t[:, k] >= 0]
                    assert len(np.unique(col)) == len(col), (kind, k)                  # one output row per (input row, offset)
                assert bool(torch.isnan(dy[n_out:]).all()) and bool(torch.isfinite(dy[:n_out]).all())
                if kind == "subm":
                    tt = BG.transpose_table(t.astype(np.int64), n_in)
                    assert np.array_equal(tt[:, ::-1], t), "the table is not symmetric"
                    assert np.array_equal(t[:, 13], np.arange(n_out))
                else:
                    dead = (BG.transpose_table(t.astype(np.int64), n_in) >= 0).sum(1) == 0
                    assert np.all(dead[3::7]) and (n_in < 5 or dead.sum() > 0) and n_out <= n_in


def test_twins_pass_the_derived_bars():
    """the fp32 twins (pairs left to right: the longest chain there is) stay inside min(d, m - 1) * 2^-24 * sum |terms| only where
    the order-free part binds; what is checked here is that the bars are formed per element and that exact cases are exact"""
    x, dy, nbr, n_in = BG.wgrad_case(16, 16, 200, 250, "down", (), tuple(sorted(BG.MOD4_COUNTS.items())))
    tw = BG.wgrad_twin(x, dy, nbr, 200)
    fig, lim, bad, cnt = BG.wgrad_check(tw, None, x, dy, nbr, 200, 10 ** 6)          # d unbounded: the (m - 1) rule alone
    assert bad == 0 and fig < lim and cnt[3] == 1
    ref = wgrad64(x.double(), dy[:200].double(), nbr[:200].numpy())[0]
    assert torch.equal(tw[3].double(), ref[3])                                         # one pair: no addition, exact
    broken = tw.clone()
    broken[7, 2, 3] += float(x[nbr[:200, 7][nbr[:200, 7] >= 0][0].long(), 2] * dy[int(torch.nonzero(nbr[:200, 7] >= 0)[0]), 3])
    assert BG.wgrad_check(broken, None, x, dy, nbr, 200, BG.wgrad_depth(200, 250))[2] >= 1   # a doubled pair is seen
    dyd, w, nb, n_out, cap_in = BG.dgrad_case(32, 16, 257)
    dx, mag, pairs, t = BG.dgrad_ref(dyd, nb, w, n_out, 257)
    fig, lim, bad = BG.dgrad_check(BG.dgrad_twin(dyd, t, w), dx, mag, pairs, 16)
    assert bad == 0 and 0 < fig < lim
    assert BG.wgrad_depth(1500, 317000) == 4 + 160 + 1 + 1 + 8 + 1 and BG.wgrad_depth(3, 53, True) == 4 + 1 + 1 + 1 + 8 + 1


# ---- regimes and the library's own word -------------------------------------------------------------------------------------
def test_cases_land_in_the_regime_they_are_named_for():
    L = _C.lib()
    # sparse weight gradient
    assert BG.sparse_wgrad_geometry(1000, 70000) == dict(wg_rows=192, nchunk=6, lds_bytes=12288, ws_chunks=547)
    g = BG.sparse_wgrad_geometry(1500, 317000)
    assert g["wg_rows"] == 640 and g["nchunk"] == 3 and g["lds_bytes"] == 40 * 1024
    g = BG.sparse_wgrad_geometry(2500, BG.DYN_LDS_CAP)
    assert g["wg_rows"] == 1088 and g["nchunk"] == 3 and g["lds_bytes"] == 68 * 1024 > 64 * 1024      # needs the dynamic-LDS opt-in
    assert BG.wgrad_rows_per_wg(65536) == 128 and BG.wgrad_rows_per_wg(65537) == 192 and BG.wgrad_rows_per_wg(1 << 24) == 2048
    chunks = [BG.sparse_wgrad_geometry(n, cap)["nchunk"] for fam, n, cap, *_ in BG.wgrad_cases(16, 16) if fam == "reduce edges"]
    assert chunks == [1, 8, 9, 16, 17, 25]
    for cin, cout in BG.WGRAD_PAIRS:
        fams = {c[0] for c in BG.wgrad_cases(cin, cout)}
        assert {"rows", "empty offsets", "ragged last step", "grown chunks"} <= fams
        assert ("waymo regime" in fams) == ((cin, cout) in ((16, 16), (16, 32))) and ("reduce edges" in fams) == ("dynamic LDS" in fams) == (cin == cout == 16)
        for fam, n, cap, *_ in BG.wgrad_cases(cin, cout):
            assert L.sassd_spconv_bwd_weight_workspace_bytes(cap, 27, cin, cout) == \
                BG.sparse_wgrad_geometry(n, cap)["ws_chunks"] * 27 * cin * cout * 4 < (1 << 30)
            # ... which holds the partials of either formulation (chunks of >= 128 rows)
            assert BG.sparse_wgrad_geometry(cap, cap)["nchunk"] <= BG.sparse_wgrad_geometry(n, cap)["ws_chunks"]
    # BatchNorm1d
    assert BG.bn_blocks(*BG.BN1D_CAP) == (1015, 69, 18) and BG.bn_blocks(4099, 16) == (33, 125, 2)
    assert 70001 // (16 * 4) > BG.BN_MAX_BLOCKS                                          # what the cap cuts
    for c, rows in BG.BN1D_ROWS.items():
        assert {1, 2} <= set(rows) and max(BG.bn_blocks(n, c)[0] for n in rows) > 1, c
        assert L.sassd_bn_relu_workspace_bytes(c) == BG.BN_MAX_BLOCKS * 4 * c * 8
        for n in rows:
            nb, rpb, rpt = BG.bn_blocks(n, c)
            assert (nb - 1) * rpb < n <= nb * rpb and rpt <= 16
    # BatchNorm2d
    for shape in BG.BN2D_SHAPES:
        assert BG.bn2d_geometry(shape[1], shape[2] * shape[3]) == BG.BN2D_REGIME[shape], shape
        assert L.sassd_bn2d_relu_workspace_bytes(shape[1]) == -(-shape[1] * BG.BN2D_MAX_SPLIT * 4 * 8 // 256) * 256
    assert 68 - 8 * 8 == 4                                                              # (1,5,4,17): a 4-element last split
    assert -(-1025 // 256) == 5                                                         # bn2d_finalize_kernel: several blocks
    # dense weight gradient
    for shape in set(BG.DENSE_SHAPES + BG.DENSE_SHAPES_BF16):
        b, cin, cout, h, w = shape
        q = BG.wgrad_plan(b, cin, cout, h, w)
        assert (q["nseg"], q["last_cols"], q["nrange"], q["rows_per"], q["last_rows"], q["n_ci_t"], q["n_co_t"]) == \
            BG.DENSE_REGIME[shape], shape
        for ks in (1, 3):
            assert L.sassd_conv2d_wgrad_workspace_bytes(b, cin, cout, h, w, ks) == q["nsplit"] * ks * ks * cout * cin * 4, shape
    for b, cin, cout, h, w in ((2, 256, 256, 200, 176), (1, 128, 256, 24, 176), (3, 256, 28, 16, 24)):     # production-sized maps too
        assert L.sassd_conv2d_wgrad_workspace_bytes(b, cin, cout, h, w, 3) == BG.wgrad_plan(b, cin, cout, h, w)["nsplit"] * 9 * cout * cin * 4
    assert all(s[4] % 2 == 0 for s in BG.DENSE_SHAPES_BF16)
    assert set(BG.DENSE_ACCUMULATE) <= set(BG.DENSE_SHAPES) and set(BG.DENSE_ACCUMULATE_BF16) <= set(BG.DENSE_SHAPES_BF16)
