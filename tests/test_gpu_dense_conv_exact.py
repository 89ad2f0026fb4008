"""-m gpu: the dense conv kernels alone on the lattice cases of tests/dense_conv_cases.py, with ZERO tolerance.  Integers in
[-4, 4], power-of-two scales and quarter shifts make every product and partial sum exactly representable (proved on the CPU in
test_dense_conv_cases_cpu.py), so each kernel must equal the float64 reference bit for bit at every element, whatever its
tiling or summation order: a wrong index, halo, tile edge, channel pad, k-tail, epilogue channel or batch stride is an
integer-sized error.  x lies in NaN (a stray read is in bounds and poisons the output), y in 7.0, and the bytes around both are
checked after every call.  Every case runs with scale and shift, with shift only and with neither, with and without the ReLU
wherever the entry point has one."""
import pytest
import torch

from sassd import _C
from sassd import autograd as AG
from sassd import kernels as K

import dense_conv_cases as DC

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _same(got, ref, what):
    got, ref = got.cpu(), ref.cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    if torch.equal(got, ref):
        return
    bad = (got != ref).nonzero()
    i = tuple(bad[0].tolist())
    raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, reference %r (largest difference %g)"
                         % (what, len(bad), ref.numel(), i, got[i].item(), ref[i].item(),
                            (got.double() - ref.double()).abs().nan_to_num(nan=float("inf")).max().item()))


def _run(c, dev, call, relus=(False, True), forms=DC.FORMS, out_dtype=torch.float32, x_dtype=torch.float32, misalign=0, what=""):
    """call(x, scale, shift, relu, y) on the case in every epilogue form; x in NaN, y in 7.0"""
    xb, x = DC.embed(c["x"].to(x_dtype), poison=NAN, device=dev, misalign=misalign)
    shape = tuple(c["acc"].shape)
    for form in forms:
        sc, sh = (None if t is None else t.to(dev) for t in DC.form_args(c, form))
        for relu in relus:
            yb, y = DC.embed(torch.full(shape, 7.0, dtype=out_dtype), poison=7.0, device=dev)
            call(x, sc, sh, relu, y)
            torch.cuda.synchronize()
            _same(y, DC.lattice_ref(c, form, relu, out_dtype), "%s %s relu=%d" % (what, form, relu))
            DC.check_surround(yb, y, 7.0)
    DC.check_surround(xb, x, NAN)


def _ids(table):
    return [c["name"] for c in table]


@pytest.mark.parametrize("case", DC.CONV2D, ids=_ids(DC.CONV2D))
def test_conv2d_fwd(dev, case):
    """conv2d_kernel<CT, TAPS, VEC> as named in the id (DC.conv2d_plan restates the dispatch); the edge is case['edge']"""
    c = DC.lattice_case("3x3" if case["ks"] == 3 else "1x1", case["b"], case["cin"], case["cout"], case["h"], case["w"], 7)
    wp = K.conv2d_pack_weight(c["w"].to(dev))
    _run(c, dev, lambda x, sc, sh, relu, y: K.conv2d_fwd(x, wp, case["cout"], case["ks"], sc, sh, relu, y),
         misalign=case.get("misalign", 0), what=case["name"])


@pytest.mark.parametrize("case", DC.CONV2D_REFUSED, ids=_ids(DC.CONV2D_REFUSED))
def test_conv2d_fwd_refuses_one_past_the_edge(dev, case):
    """one quad wider than an accepted edge (and W = 2 on the wide forms): an error before any launch, y untouched"""
    assert not DC.conv2d_plan(case["cout"], case["ks"], case["h"], case["w"])["ok"]
    x = torch.ones(1, case["cin"], case["h"], case["w"], device=dev)
    wp = K.conv2d_pack_weight(torch.ones(case["cout"], case["cin"], case["ks"], case["ks"], device=dev))
    yb, y = DC.embed(torch.full((1, case["cout"], case["h"], case["w"]), 7.0), poison=7.0, device=dev)
    with pytest.raises(RuntimeError, match="sassd_conv2d_fwd failed with code %d" % _C.EINVAL):
        K.conv2d_fwd(x, wp, case["cout"], case["ks"], None, None, False, y)
    torch.cuda.synchronize()
    assert bool((yb == 7.0).all())


@pytest.mark.parametrize("case", DC.NARROW, ids=_ids(DC.NARROW))
def test_conv1x1_narrow_fwd(dev, case):
    c = DC.lattice_case("1x1", case["b"], case["cin"], case["cout"], case["h"], case["w"], 7)
    assert K.conv1x1_narrow_supported(case["cin"], case["cout"])
    wt = K.conv1x1_narrow_pack_weight(c["w"].to(dev))
    _run(c, dev, lambda x, sc, sh, relu, y: K.conv1x1_narrow_fwd(x, wt, case["cout"], sc, sh, relu, y), what=case["name"])


@pytest.mark.parametrize("case", DC.WINO2, ids=_ids(DC.WINO2))
def test_conv2d_wino_fwd(dev, case):
    """Winograd F(2x2, 3x3): G holds 1 and 1/2, B and A only +-1 -- exact on the lattice"""
    c = DC.lattice_case("3x3", case["b"], case["cin"], case["cout"], case["h"], case["w"], 7)
    assert K.conv2d_wino_supported(case["cin"], case["cout"], case["h"], case["w"])
    wp = K.conv2d_wino_pack_weight(c["w"].to(dev))
    _run(c, dev, lambda x, sc, sh, relu, y: K.conv2d_wino_fwd(x, wp, case["cout"], sc, sh, relu, y), what=case["name"])


@pytest.mark.parametrize("geo", [1, 0, 12], ids=["fp32-mfma", "split-default", "split-word-12"])
@pytest.mark.parametrize("case", DC.GEMM1X1, ids=_ids(DC.GEMM1X1))
def test_conv1x1_gemm_fwd(dev, case, geo):
    """both MFMA forms against the same reference (so they also equal each other): a lattice value is an exact bf16 number and
    splits as (v, 0, 0).  The entry reads only `geo != 1` of the word (the split form where H W % 128 == 0)."""
    c = DC.lattice_case("1x1", case["b"], case["cin"], case["cout"], case["h"], case["w"], 7)
    assert K.conv1x1_gemm_supported(case["cin"], case["cout"], case["h"], case["w"])
    wp = K.conv1x1_gemm_pack_weight(c["w"].to(dev))
    _run(c, dev, lambda x, sc, sh, relu, y: K.conv1x1_gemm_fwd(x, wp, case["cout"], sc, sh, relu, y, cfg=K.wino4_cfg(geo)),
         what="%s word %d" % (case["name"], geo))


@pytest.mark.parametrize("nwg", [0, 1, 3], ids=["default-launch", "nwg1", "nwg3"])
@pytest.mark.parametrize("case", DC.BF16_3X3, ids=_ids(DC.BF16_3X3))
def test_conv2d_bf16_fwd(dev, case, nwg):
    """the training form (fp32 maps, bias only) under the default launch and the forced workgroup counts cfg = nwg << 8 (the
    launcher rounds them up to 8: every workgroup walks a long run of tiles); the data gradient through the transposed,
    tap-mirrored pack autograd builds, against conv_transpose2d"""
    c = DC.lattice_case(case["kind"], case["b"], case["cin"], case["cout"], case["h"], case["w"], 7)
    wd = c["w"].to(dev)
    pk = AG._bf16_pack(wd, True) if c["dgrad"] else K.conv2d_bf16_pack_weight(wd)
    assert K.conv2d_bf16_supported(c["x"].shape[1], c["nout"], case["h"], case["w"])
    _run(c, dev, lambda x, sc, sh, relu, y: K.conv2d_bf16_fwd(x, pk, c["nout"], sh, y, cfg=nwg << 8), relus=(False,),
         forms=("shift", "none"), what="%s nwg %d" % (case["name"], nwg))


@pytest.mark.parametrize("transposed", [False, True], ids=["forward", "transposed-pack"])
@pytest.mark.parametrize("case", DC.BF16_1X1, ids=_ids(DC.BF16_1X1))
def test_conv1x1_bf16_fwd(dev, case, transposed):
    """k = the contracted channels, n = the output channels; transposed: the forward layer's [k][n] array read as its transpose"""
    k, n = case["k"], case["n"]
    assert K.conv1x1_bf16_supported(k, n, case["h"] * case["w"])
    if transposed:
        c = DC.lattice_case("1x1_dgrad", case["b"], n, k, case["h"], case["w"], 7)
    else:
        c = DC.lattice_case("1x1", case["b"], k, n, case["h"], case["w"], 7)
    pk = K.conv1x1_bf16_pack_weight(c["w"].to(dev), transposed)
    _run(c, dev, lambda x, sc, sh, relu, y: K.conv1x1_bf16_fwd(x, pk, n, sh, y), relus=(False,), forms=("shift", "none"),
         what=case["name"])


@pytest.mark.parametrize("out_bf16", [False, True], ids=["fp32-store", "bf16-store"])
@pytest.mark.parametrize("case", DC.INFER_3X3, ids=_ids(DC.INFER_3X3))
def test_conv2d_bf16_infer_fwd(dev, case, out_bf16):
    """bf16 map in; the bf16 store must be round-to-nearest-even of the exactly known value (lattice sums land on ties)"""
    c = DC.lattice_case("3x3", case["b"], case["cin"], case["cout"], case["h"], case["w"], 7)
    assert K.conv2d_bf16_infer_supported(case["cin"], case["cout"], case["h"], case["w"])
    pk = K.conv2d_bf16_infer_pack_weight(c["w"].to(dev))
    if out_bf16:
        r64 = DC.lattice_ref(c, "scale+shift", False, torch.float64)
        assert int((r64.float().bfloat16().double() != r64).sum()) > 0, "the case rounds somewhere"
    _run(c, dev, lambda x, sc, sh, relu, y: K.conv2d_bf16_infer_fwd(x, pk, case["cout"], sc, sh, relu, y, out_bf16),
         out_dtype=torch.bfloat16 if out_bf16 else torch.float32, x_dtype=torch.bfloat16, what=case["name"])


@pytest.mark.parametrize("out_bf16", [False, True], ids=["fp32-store", "bf16-store"])
@pytest.mark.parametrize("case", DC.INFER_1X1, ids=_ids(DC.INFER_1X1))
def test_conv1x1_bf16_infer_fwd(dev, case, out_bf16):
    c = DC.lattice_case("1x1", case["b"], case["cin"], case["cout"], case["h"], case["w"], 7)
    assert K.conv1x1_bf16_infer_supported(case["cin"], case["cout"], case["h"] * case["w"])
    pk = K.conv1x1_bf16_pack_weight(c["w"].to(dev))
    _run(c, dev, lambda x, sc, sh, relu, y: K.conv1x1_bf16_infer_fwd(x, pk, case["cout"], sc, sh, relu, y, out_bf16),
         out_dtype=torch.bfloat16 if out_bf16 else torch.float32, x_dtype=torch.bfloat16, what=case["name"])


def test_bf16_store_ties_round_to_even(dev):
    """a tie on purpose: acc = 257 = 0x1.01p8 lies exactly between the bf16 neighbours 256 and 258 -> 256 (even); 259 -> 260"""
    x = torch.zeros(1, 17, 1, 4)
    x[0, :, 0, 0], x[0, :, 0, 1] = 4.0, 4.0
    x[0, 16, 0, 0], x[0, 16, 0, 1] = 1.0, 3.0
    w = torch.full((1, 17, 1, 1), 4.0)
    w[0, 16] = 1.0
    acc = torch.nn.functional.conv2d(x.double(), w.double())
    assert acc[0, 0, 0].tolist() == [257.0, 259.0, 0.0, 0.0]
    pk = K.conv1x1_bf16_pack_weight(w.to(dev))
    y = K.conv1x1_bf16_infer_fwd(x.bfloat16().to(dev), pk, 1, None, None, False, None, True)
    assert y.cpu().float()[0, 0, 0].tolist() == [256.0, 260.0, 0.0, 0.0]
