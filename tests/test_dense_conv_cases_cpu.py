"""CPU proof of tests/dense_conv_cases.py before any GPU is involved: every lattice case stays below 2^24 units of its grid
(recomputed here from the case's operands), the float64 references are torch's, torch's fp32 conv and an fp32 F(2x2) with a
shuffled channel order reproduce them bit for bit, bf16 is the identity on lattice operands, the F(4x4) twin's matrices are
right, the per-element bar catches a twin that loses the third bf16 piece of V, and every shape that claims to sit on a limit of
the host code sits on it (the limit recomputed with the arithmetic of the .hip file, the line quoted)."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_conv_cases as DC


def _lattice_cases():
    out = []
    for c in DC.CONV2D:
        out.append(("conv2d " + c["name"], ("3x3" if c["ks"] == 3 else "1x1", c["b"], c["cin"], c["cout"], c["h"], c["w"])))
    for c in DC.NARROW:
        out.append(("narrow " + c["name"], ("1x1", c["b"], c["cin"], c["cout"], c["h"], c["w"])))
    for c in DC.WINO2:
        out.append(("wino2 " + c["name"], ("3x3", c["b"], c["cin"], c["cout"], c["h"], c["w"])))
    for c in DC.GEMM1X1:
        out.append(("gemm1x1 " + c["name"], ("1x1", c["b"], c["cin"], c["cout"], c["h"], c["w"])))
    for c in DC.BF16_3X3:
        out.append(("bf16 3x3 " + c["name"], (c["kind"], c["b"], c["cin"], c["cout"], c["h"], c["w"])))
    for c in DC.BF16_1X1:
        out.append(("bf16 1x1 " + c["name"], ("1x1", c["b"], c["k"], c["n"], c["h"], c["w"])))
        out.append(("bf16 1x1 t " + c["name"], ("1x1_dgrad", c["b"], c["n"], c["k"], c["h"], c["w"])))
    for c in DC.INFER_3X3:
        out.append(("infer 3x3 " + c["name"], ("3x3", c["b"], c["cin"], c["cout"], c["h"], c["w"])))
    for c in DC.INFER_1X1:
        out.append(("infer 1x1 " + c["name"], ("1x1", c["b"], c["cin"], c["cout"], c["h"], c["w"])))
    return out


LATTICE = _lattice_cases()


@pytest.mark.parametrize("name,args", LATTICE, ids=[n for n, _ in LATTICE])
def test_lattice_case_is_exact_in_fp32(name, args):
    """operands on the lattice, the reference torch's float64 one, and every value an algorithm can form below 2^24 grid units"""
    c = DC.lattice_case(*args, seed=7)
    x, w = c["x"], c["w"]
    assert torch.equal(x, x.round()) and torch.equal(w, w.round()) and x.abs().max() <= 4 and w.abs().max() <= 4
    assert (x == 0).float().mean() <= 1.0 / 9 + 0.05 or x.numel() < 200
    assert set(c["scale"].tolist()) <= set(DC.SCALES) and torch.equal(c["shift"] * 4, (c["shift"] * 4).round())
    assert c["shift"].abs().max() <= 8 and c["scale"].numel() == c["shift"].numel() == c["nout"]
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(w.bfloat16().float(), w), "bf16 is the identity on the lattice"
    ks = c["ks"]
    ref = F.conv_transpose2d(x.double(), w.double(), None, 1, ks // 2) if c["dgrad"] else F.conv2d(x.double(), w.double(), None, 1, ks // 2)
    assert torch.equal(ref, c["acc"]) and c["acc"].shape[1] == c["nout"]
    # the bound, recomputed: 81 (F(2x2): 4 on V x 9/4 on U x 9 terms; the direct form's 9 taps fit under it) x the largest sum
    # over the contracted channels of max|x_c| max|w_c|, through the epilogue, in units of 2^-3
    xm = x.abs().amax(dim=(0, 2, 3))
    wm = w.abs().amax(dim=(2, 3))
    a = (wm * xm.view(-1, 1)).sum(0).max() if c["dgrad"] else (wm * xm.view(1, -1)).sum(1).max()
    bound = ((81.0 if ks == 3 else 1.0) * float(a) * float(c["scale"].abs().max()) + float(c["shift"].abs().max())) * 8.0
    assert bound == c["bound"] and bound < 2.0 ** 24, (name, bound)
    s = F.conv_transpose2d(x.double().abs(), w.double().abs(), None, 1, ks // 2) if c["dgrad"] else \
        F.conv2d(x.double().abs(), w.double().abs(), None, 1, ks // 2)
    assert float(s.max()) <= float(a) * ks * ks
    for form in DC.FORMS:
        for relu in (False, True):
            r64 = DC.lattice_ref(c, form, relu, torch.float64)
            assert torch.equal(r64 * 8, (r64 * 8).round()), "references sit on the 2^-3 grid"
            assert torch.equal(DC.lattice_ref(c, form, relu).double(), r64), "and are fp32 numbers"


def _f2x2(x, w, perm):
    """fp32 Winograd F(2x2, 3x3), pad 1, channels accumulated in the order `perm` (G with 1 and 1/2, B and A with +-1)"""
    G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float32)
    Bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float32)
    At = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float32)
    b, c, h, wd = x.shape
    U = torch.einsum("ij,ocjk,lk->ocil", G, w, G)                      # every sum has <= 3 exact terms
    xp = F.pad(x, (1, 1, 1, 1))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                             # [b, c, th, tw, 4, 4]
    V = torch.einsum("ij,bcyxjk,lk->bcyxil", Bt, d, Bt)
    M = torch.zeros(b, w.shape[0], h // 2, wd // 2, 4, 4)
    peak = 0.0
    for ci in perm:
        M = M + U[None, :, ci, None, None] * V[:, None, ci]
        peak = max(peak, float(M.abs().max()))
    Y = torch.einsum("ij,boyxjk,lk->boyxil", At, M, At)
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(b, w.shape[0], h, wd), peak


@pytest.mark.parametrize("args", [("3x3", 2, 64, 96, 6, 72), ("3x3", 1, 320, 32, 4, 8), ("3x3", 3, 32, 64, 2, 68)])
def test_fp32_conv_and_fp32_f2x2_reproduce_the_reference_bit_for_bit(args):
    """the exactness claim without a GPU: torch's fp32 CPU conv and an fp32 F(2x2) with the channels shuffled equal float64"""
    c = DC.lattice_case(*args, seed=7)
    assert c["bound"] < 2.0 ** 24
    assert torch.equal(F.conv2d(c["x"], c["w"], None, 1, 1).double(), c["acc"])
    perm = torch.randperm(c["x"].shape[1], generator=torch.Generator().manual_seed(3)).tolist()
    y, peak = _f2x2(c["x"], c["w"], perm)
    assert y.dtype == torch.float32 and torch.equal(y.double(), c["acc"])
    y2, _ = _f2x2(c["x"], c["w"], perm[::-1])
    assert torch.equal(y, y2)
    assert peak * 8 <= c["bound"], "the largest intermediate is inside the case's bound"
    print("F(2x2) on %s: largest |intermediate| %.0f, bound %.0f grid units" % (args, peak, c["bound"]))


def test_bt_constants_are_the_kernels():
    """the twin's constants: each literal of bt_vec stands in conv2d_wino4.hip and is the fp32 value of its rational"""
    src = DC.hip_source("conv2d_wino4.hip")
    body = src[src.index("void bt_vec("):src.index("struct W4Geom")]
    lits = set(re.findall(r"[0-9]+\.[0-9]+f", body))
    assert lits == set(DC.BT_CONST), lits ^ set(DC.BT_CONST)
    for lit, (n, d) in DC.BT_CONST.items():
        assert np.float32(float(lit[:-1])) == np.float32(n / d), lit
    assert "o[1] = s + t;" in body and "o[2] = s - t;" in body and "o[3] = u + v;" in body and "o[4] = u - v;" in body
    g = src[src.index("void g_row("):src.index("__global__ void wino4_pack_kernel")]
    assert "g0 + 0.390625f * g2, f = 0.625f * g1" in g and "g0 + 2.25f * g2, f2 = 1.5f * g1" in g
    a = src[src.index("void at_vec("):src.index("// (CoutP")]
    assert "o[3] = 0.244140625f * d1 + 3.375f * d2 + m[5];" in a and "o[2] = 0.390625f * s1 + 2.25f * s2;" in a


@pytest.mark.parametrize("kind,b,cin,cout,h,w", [("randn", 2, 8, 5, 8, 12), ("lattice", 1, 3, 4, 4, 4), ("one_live", 3, 6, 2, 12, 8)])
def test_wino4_twin_in_float64_is_conv2d(kind, b, cin, cout, h, w):
    x, wt, sc, sh = DC.wino4_inputs(kind, b, cin, cout, h, w, 5)
    raw = F.conv2d(x.double(), wt.double(), None, 1, 1)
    got = DC.wino4_twin(x.numpy(), wt.numpy(), np.float64)
    assert np.abs(got - raw.numpy()).max() <= 1e-12 * max(1.0, float(raw.abs().max()))
    ref = DC.epilogue(raw, sc, sh, True).numpy()
    got = DC.wino4_twin(x.numpy(), wt.numpy(), np.float64, sc.numpy(), sh.numpy(), True)
    assert np.abs(got - ref).max() <= 1e-12 * max(1.0, float(np.abs(ref).max()))
    t32 = DC.wino4_twin(x.numpy(), wt.numpy(), np.float32, sc.numpy(), sh.numpy(), True)
    assert t32.dtype == np.float32


@pytest.mark.parametrize("kind,cin", [("randn", 32), ("one_live", 32)])
def test_the_bar_catches_a_lost_third_piece(kind, cin):
    """sharpness: V reduced to two bf16 pieces (a 2^-16 error) passes the whole-tensor bar of test_gpu_wino4.py and misses the
    per-element one by at least 2x"""
    c = DC.wino4_case(kind, 1, cin, 256, 16, 16, 11)
    lossy = DC.wino4_twin_two_pieces(c["x"].numpy(), c["w"].numpy(), c["scale"].numpy(), c["shift"].numpy(), True)
    fig = DC.figure(lossy, c["ref"], c["scale_of"])
    old = np.abs(lossy - c["ref"]).max() / max(1.0, np.abs(c["ref"]).max())
    print("%s Cin %d: fp32 twin %.2e, two-piece twin %.2e = %.1f x the bar %.2e; old whole-tensor figure %.2e (bar 1e-4)"
          % (kind, cin, c["twin_figure"], fig, fig / c["bar"], c["bar"], old))
    assert c["bar"] == max(4 * c["twin_figure"], 4 * 2.0 ** -24)
    assert fig > 2.0 * c["bar"]
    assert old < 1e-4


def test_scale_of_takes_the_tile_maximum():
    x = torch.zeros(1, 1, 8, 8)
    x[0, 0, 4, 5] = 2.0
    w = torch.ones(1, 1, 3, 3)
    s = DC.scale_of(x, w)
    assert torch.equal(s[0, 0, :4, 4:], torch.full((4, 4), 2.0, dtype=torch.float64))       # pixel (3, 4) sees x[4, 5]
    assert torch.equal(s[0, 0, 4:, 4:], torch.full((4, 4), 2.0, dtype=torch.float64))
    assert float(s[0, 0, :, :4].max()) == 0.0                                               # no pixel left of column 4 does
    assert float(DC.scale_of(x, w, tile=0)[0, 0, 0, 4]) == 0.0
    assert float(DC.scale_of(x, w, torch.tensor([-3.0]), torch.tensor([0.5]))[0, 0, 7, 7]) == 6.5


def test_embed_and_check_surround():
    t = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    for mis in (0, 1):
        buf, v = DC.embed(t, poison=float("nan"), misalign=mis)
        assert torch.equal(v, t) and v.data_ptr() % 16 == 4 * mis and torch.isnan(buf).sum() == buf.numel() - 24
        DC.check_surround(buf, v, float("nan"))
    buf, v = DC.embed(torch.zeros(5, dtype=torch.bfloat16), poison=7.0)
    DC.check_surround(buf, v, 7.0)
    off = (v.data_ptr() - buf.data_ptr()) // 2
    for where in (off - 1, off + 5, 0, buf.numel() - 1):
        b2 = buf.clone()
        v2 = b2[off:off + 5]
        b2[where] = 1.0
        with pytest.raises(AssertionError):
            DC.check_surround(b2, v2, 7.0)


# ---- shapes that claim a limit of the host code sit on it ---------------------------------------------------------------
def test_conv2d_cases_reach_every_instantiation_and_their_edges():
    src = DC.hip_source("conv2d.hip")
    for line in ("P.PW = (P.W + 8 + 3) / 4 * 4;", "P.NPR = (C::PIX - 1 + P.W - 1) / P.W + 1 + 2 * C::HALO;",
                 "const size_t ps = ((size_t)C::KC * P.NPR * P.PW + 255) / 256 * 256;",
                 "if (lds > 160 * 1024) return SASSD_EINVAL;",
                 "if (VEC == 4 ? (ps > (size_t)C::MAXPJ * 4 * 256) : ((size_t)C::KC * P.NPR * P.W > (size_t)256 * C::MAXLP))",
                 "static constexpr int MAXPJ = 10;", "static constexpr int MAXLP = (VEC == 4) ? 1 : 40;",
                 "const bool vec = (W % 4 == 0) && (((uintptr_t)x & 15) == 0);",
                 "inline int cout_pad(int Cout) { return (Cout > 64) ? cdiv(Cout, 128) * 128 : cdiv(Cout, 32) * 32; }"):
        assert line in src, line
    seen = set()
    for c in DC.CONV2D:
        p = DC.conv2d_plan(c["cout"], c["ks"], c["h"], c["w"], aligned=not c.get("misalign"))
        assert p["ok"], c["name"]
        assert c["name"].startswith("<%d,%d,%d>" % p["inst"]), (c["name"], p["inst"])
        seen.add(p["inst"])
        hw = c["h"] * c["w"]
        if "widest" in c["name"]:
            assert not DC.conv2d_plan(c["cout"], c["ks"], c["h"], c["w"] + 4)["ok"], c["name"]
            if c["w"] == 312:                                         # nothing wider is accepted, and ps sits on the limit
                assert p["ps"] == 10 * 4 * 256 and p["kc"] * p["NPR"] * p["PW"] == p["ps"]
                assert not any(DC.conv2d_plan(c["cout"], c["ks"], c["h"], w)["ok"] for w in range(316, 4096, 4))
            if c["w"] == 248:
                assert p["ps"] == 10 * 4 * 256 and p["NPR"] == 5 and p["kc"] * p["NPR"] * p["PW"] == p["ps"]
            if c["w"] == 204:
                assert p["NPR"] == 3 and p["ps"] == 10 * 4 * 256
        if "above-a-tile" in c["name"]:
            assert 0 < hw - p["pix"] <= (c["w"] if p["inst"][2] == 4 else 1) and c["w"] <= 8 or c["w"] in (17, 23)
        if "below-a-tile" in c["name"]:
            assert hw < p["pix"]
    assert seen == {(ct, taps, vec) for ct in (4, 1) for taps in (9, 1) for vec in (4, 1)}
    assert {c["cin"] for c in DC.CONV2D} >= {1, 5, 8, 9, 17, 40} and {c["cout"] for c in DC.CONV2D} >= {1, 31, 32, 33, 64, 65, 128, 129}
    for c in DC.CONV2D_REFUSED:
        p = DC.conv2d_plan(c["cout"], c["ks"], c["h"], c["w"])
        assert not p["ok"] and c["name"].startswith("<%d,%d,%d>" % p["inst"]), c["name"]
    # the wide forms refuse W = 2 because of the LDS, and W = 3 is the narrowest map they take
    assert DC.conv2d_plan(128, 3, 150, 2)["lds"] > 160 * 1024 and DC.conv2d_plan(128, 3, 100, 3)["ok"]


def test_narrow_and_bf16_tables_cover_what_they_claim():
    assert [c["cout"] for c in DC.NARROW] == [1, 8, 9, 16, 17, 20, 21, 24, 25, 28, 29, 32]
    assert {c["cin"] for c in DC.NARROW} == {1, 3, 4, 5, 7, 256} and {c["h"] * c["w"] for c in DC.NARROW} == {1, 63, 64, 65}
    src = DC.hip_source("conv1x1_bf16.hip")
    assert "return Cin >= 1 && Cin <= 256 && Cin > 16 * (c1_ksteps(Cin) - 1) && Cout >= 1 && HW >= 4 && HW % 4 == 0;" in src
    assert "int c1_ksteps(int Cin) { return Cin <= 16 ? 1 : Cin <= 32 ? 2 : Cin <= 64 ? 4 : Cin <= 128 ? 8 : 16; }" in src
    ks = lambda c: 1 if c <= 16 else 2 if c <= 32 else 4 if c <= 64 else 8 if c <= 128 else 16        # noqa: E731
    ok = lambda c: 1 <= c <= 256 and c > 16 * (ks(c) - 1)                                             # noqa: E731
    ends = sorted(f(c for c in range(1, 257) if ok(c) and ks(c) == k) for k in (1, 2, 4, 8, 16) for f in (min, max))
    assert ends == sorted(c["k"] for c in DC.BF16_1X1), ends
    assert {c["n"] for c in DC.BF16_1X1} == {1, 63, 64, 65, 130} and {c["h"] * c["w"] for c in DC.BF16_1X1} == {4, 60, 64, 68}
    assert {c["cin"] for c in DC.BF16_3X3 if c["kind"] == "3x3"} == {1, 8, 31, 32, 33, 70}
    assert {(c["h"], c["w"]) for c in DC.BF16_3X3 if c["kind"] == "3x3"} == {(1, 16), (2, 20), (5, 36), (3, 188)}
    for c in DC.WINO2:
        assert c["cin"] % 32 == 0 and c["cout"] % 32 == 0 and c["h"] % 2 == 0 and c["w"] >= 64 and c["w"] % 4 == 0
    assert {(c["h"], c["w"]) for c in DC.WINO2} == {(2, 64), (2, 68), (4, 64), (6, 72), (10, 100)}


def test_gemm1x1_cases_run_every_block_width_and_the_split_form():
    src = DC.hip_source("conv2d_wino4.hip")
    assert "if (geo != 1 && hw % 128 == 0) return launch_w4_gemm<2, 2, 2, kKC, 1>(P, dbg, stream);" in src
    assert "switch (w4_pick_wn(hw, Cout, batch, true)) {" in src
    widths = {DC.w4_pick_wn(c["h"] * c["w"], c["cout"], c["b"], True) * 32 for c in DC.GEMM1X1}
    assert widths == {64, 96, 128, 160}, widths                      # (64 columns win every tie: 192 is never picked here)
    assert {c["h"] * c["w"] for c in DC.GEMM1X1} >= {64, 96, 128, 160, 192}
    big = [c for c in DC.GEMM1X1 if DC.w4_pick_wn(c["h"] * c["w"], c["cout"], c["b"], True) == 4][0]
    assert not any(DC.w4_pick_wn(hw, big["cout"], big["b"], True) == 4 for hw in range(64, big["h"] * big["w"], 32))
    assert sum((c["h"] * c["w"]) % 128 == 0 for c in DC.GEMM1X1) >= 2
    assert {c["cout"] for c in DC.GEMM1X1} == {128, 384} and {c["cin"] for c in DC.GEMM1X1} == {32, 64}


def test_wino4_cases_sit_on_their_blocks():
    src = DC.hip_source("conv2d_wino4.hip")
    for line in ("if (c >= 2 && c <= 6) return W4Tile{0, c, 1, kKC, 2};", "if (c >= 11 && c <= 13) return W4Tile{1, c - 10, 2, kKC, 2};",
                 "if (c == 14) return W4Tile{1, 2, 2, 16, 2};", "if (c == 15) return W4Tile{1, 2, 3, 16, 4};",
                 "if (c == 16) return W4Tile{1, 2, 4, 16, 4};", "if (c == 1) return W4Tile{0, w4_pick_wn(T, Cout), 1, kKC, 2};",
                 "if (c == 0 && w4_wide_pays(T, Cout)) return W4Tile{1, 2, 3, 16, 4};",
                 "const long small = 36L * (Cout / kBM) * cdiv(T, 128), wide = 36L * (Cout / (2 * kBM)) * cdiv(T, 192);",
                 "return 2 * ((wide + 511) / 512) < (small + 511) / 512;"):
        assert line in src, line
    per_geo = {}
    for c in DC.WINO4:
        T = c["b"] * (c["h"] // 4) * (c["w"] // 4)
        bn = DC.w4_block(T, c["cout"], c["geo"])
        assert bn == c["bn"], c["name"]
        which = c["name"].split("-")[1]
        if which == "b3":
            per = T // 3
            assert c["b"] == 3 and bn < T <= bn + 3 and per % bn and (2 * per) % bn
        else:
            assert T == {"one": 1, "below": bn - 1, "block": bn, "above": bn + 1}[which]
        per_geo.setdefault(c["geo"], []).append(c)
    assert sorted(per_geo) == [1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15, 16]
    for geo, cs in per_geo.items():
        assert len(cs) == 5 and {c["kind"] for c in cs} == {"lattice", "randn", "one_live"}
        assert {c["cin"] for c in cs} == {32, 64} and {c["cout"] for c in cs} == {256, 512}
    for c in DC.WINO4_DEFAULT:
        T = (c["h"] // 4) * (c["w"] // 4)
        assert T == c["T"] and DC.w4_wide_pays(T, c["cout"]) == c["wide"]
        assert DC.w4_wide_pays(T + 1, c["cout"]) and not DC.w4_wide_pays(T - 1 - c["wide"], c["cout"])
    assert [c["cout"] for c in DC.TAIL] == [1, 5, 28, 63, 64]
