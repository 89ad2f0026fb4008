"""The 3..8-feature sparse input layer without a GPU: the C ABI of include/sassd.h "Sparse input layer" exists and checks its
arguments before it touches a device, pipeline.input_features_of reads the width from a state dict, and the stream's input
check still holds a cloud to the stream's own width."""
import ctypes as C

import numpy as np
import pytest
import torch

import sassd  # noqa: F401
from sassd import _C

EINVAL = -1
NAMES = ("sassd_spconv_in_supported", "sassd_spconv_in_packed_floats", "sassd_spconv_in_pack_weight", "sassd_spconv_in_fwd",
         "sassd_spconv_in_bwd_weight_workspace_bytes", "sassd_spconv_in_bwd_weight")


def test_symbols_exist_and_are_bound():
    L = _C.lib()
    for name in NAMES:
        assert name in _C.EXPORTS
        assert getattr(L, name) is not None


def test_supported_is_exactly_27_3to8_16():
    L = _C.lib()
    for k in (1, 8, 26, 27, 28):
        for cin in range(0, 18):
            for cout in (4, 8, 16, 32, 64):
                want = 1 if (k == 27 and 3 <= cin <= 8 and cout == 16) else 0
                assert L.sassd_spconv_in_supported(k, cin, cout) == want, (k, cin, cout)


def test_host_side_sizes():
    L = _C.lib()
    for cin in range(3, 9):
        cp = (cin + 3) // 4 * 4
        assert L.sassd_spconv_in_packed_floats(27, cin, 16) == 27 * cp * 16
        # one [27, Cin, 16] partial per workgroup of >= 128 rows
        per = 27 * cin * 16 * 4
        ws = L.sassd_spconv_in_bwd_weight_workspace_bytes(1000, 27, cin, 16)
        assert ws % per == 0 and per <= ws <= 8 * per
        big = L.sassd_spconv_in_bwd_weight_workspace_bytes(400000, 27, cin, 16)
        assert big % per == 0 and big // per <= 512              # the partials stay bounded at Waymo scale
    assert L.sassd_spconv_in_packed_floats(27, 4, 16) == L.sassd_spconv_packed_floats(27, 4, 16)
    for bad in ((27, 2, 16), (27, 9, 16), (27, 5, 32), (1, 5, 16)):
        assert L.sassd_spconv_in_packed_floats(*bad) == 0
        assert L.sassd_spconv_in_bwd_weight_workspace_bytes(1000, *bad) == 0


def test_argument_checks_answer_einval_without_a_device():
    L = _C.lib()
    null, p = None, C.c_void_p(256)

    def fwd(x=p, nbr=p, n=p, cap=100, w=p, k=27, cin=5, cout=16, y=p, y_bf16=0):
        return L.sassd_spconv_in_fwd(x, nbr, n, cap, w, k, cin, cout, null, null, 0, y, y_bf16, null)

    def pack(w=p, k=27, cin=5, cout=16, packed=p):
        return L.sassd_spconv_in_pack_weight(w, k, cin, cout, packed, null)

    def wgrad(x=p, dy=p, nbr=p, n=p, cap=100, k=27, cin=5, cout=16, dw=p, ws=p, wsb=None):
        if wsb is None:
            wsb = L.sassd_spconv_in_bwd_weight_workspace_bytes(cap, 27, 5, 16)
        return L.sassd_spconv_in_bwd_weight(x, dy, nbr, n, cap, k, cin, cout, dw, 0, ws, wsb, null)

    # NULL pointers
    for kw in (dict(x=null), dict(nbr=null), dict(n=null), dict(w=null), dict(y=null)):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(w=null), dict(packed=null)):
        assert pack(**kw) == EINVAL, kw
    for kw in (dict(x=null), dict(dy=null), dict(nbr=null), dict(n=null), dict(dw=null), dict(ws=null)):
        assert wgrad(**kw) == EINVAL, kw
    # unsupported shapes: Cin 2 and 9, Cout 32, K 1
    for kw in (dict(cin=2), dict(cin=9), dict(cout=32), dict(k=1)):
        assert fwd(**kw) == EINVAL, kw
        assert pack(**kw) == EINVAL, kw
        assert wgrad(wsb=1 << 30, **kw) == EINVAL, kw
    assert fwd(cap=0) == EINVAL and wgrad(cap=0) == EINVAL
    # a misaligned packed image
    assert fwd(w=C.c_void_p(260)) == EINVAL
    assert fwd(w=C.c_void_p(260), y_bf16=1) == EINVAL
    assert pack(packed=C.c_void_p(264)) == EINVAL
    # a workspace one byte short
    need = L.sassd_spconv_in_bwd_weight_workspace_bytes(100, 27, 5, 16)
    assert need > 0 and wgrad(wsb=need - 1) == EINVAL


def test_existing_entry_points_keep_their_answers():
    L = _C.lib()
    p = C.c_void_p(256)
    for cin in (3, 5, 8):            # the (4, 16)-only table of the older entry points is unchanged
        assert L.sassd_spconv_fwd(p, p, p, 100, p, 27, cin, 16, None, None, 0, p, 0, None) == EINVAL
        assert L.sassd_spconv_pack_weight(p, 27, cin, 16, p, None) == EINVAL
        assert L.sassd_spconv_bwd_weight(p, p, p, p, 100, 27, cin, 16, p, 0, 0, p, 1 << 30, None) == EINVAL
        assert L.sassd_spconv_bf16_supported(27, cin, 16, 100) == 0


def _sd(shape):
    return {"neck.backbone.conv0.0.weight": torch.zeros(*shape), "other": torch.zeros(1)}


def test_input_features_of():
    from sassd.pipeline import INPUT_WEIGHT_KEY, input_features_of
    for cin in (3, 4, 5, 8):
        assert input_features_of(_sd((3, 3, 3, cin, 16))) == cin
    for shape in ((3, 3, 3, 2, 16), (3, 3, 3, 9, 16), (27, 5, 16, 1), (3, 3, 3, 5, 32), (1, 3, 3, 5, 16)):
        with pytest.raises(ValueError, match=INPUT_WEIGHT_KEY.replace(".", r"\.")):
            input_features_of(_sd(shape))
    with pytest.raises(ValueError, match=INPUT_WEIGHT_KEY.replace(".", r"\.")):
        input_features_of({"other": torch.zeros(1)})


def test_routing_rule():
    from sassd import kernels as K
    for cin in range(0, 20):
        assert K.spconv_in_routed(27, cin, 16) == (cin in (3, 5, 6, 7, 8)), cin      # width 4 keeps its own calls
    assert not K.spconv_in_routed(1, 5, 16) and not K.spconv_in_routed(27, 5, 32)


def test_check_frame_inputs_holds_clouds_to_the_stream_width():
    from sassd.stream import check_frame_inputs
    five = [np.zeros((10, 5), np.float32)]
    assert check_frame_inputs(five, None, 1, 5, 100) is None
    with pytest.raises(ValueError, match=r"expected \[N, 5\]"):
        check_frame_inputs([np.zeros((10, 4), np.float32)], None, 1, 5, 100)
    with pytest.raises(ValueError, match=r"expected \[N, 4\]"):
        check_frame_inputs(five, None, 1, 4, 100)


def test_narrow_layer_forms_name_the_layer():
    from sassd import spconv
    x = spconv.SparseConvTensor(torch.zeros(2, 5), torch.zeros(2, 4, dtype=torch.int32), (4, 4, 4), 1)
    for layer in (spconv.SubMConv3d(5, 16, 1, bias=False, indice_key="pw5"),
                  spconv.SparseConv3d(5, 16, 3, 2, padding=1, bias=False, indice_key="down5"),
                  spconv.SubMConv3d(5, 32, 3, bias=False, indice_key="wide5")):
        with pytest.raises(NotImplementedError, match=layer.indice_key):
            layer(x)
