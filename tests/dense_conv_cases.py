"""Cases and references of the kernel-level tests of the dense BEV convolutions (numpy / torch-CPU only; nothing here touches
a GPU).  tests/test_dense_conv_cases_cpu.py proves what is claimed here; tests/test_gpu_dense_conv_exact.py and
tests/test_gpu_wino4_elementwise.py hold the kernels to it.

**Lattice cases: zero tolerance.**  `lattice_case` draws x and w as integers in [-4, 4] (x: one value in nine is 0), `scale` from
{-1, 0.5, 1, 2, 4} and `shift` as multiples of 0.25 in [-8, 8].  Every product and every partial sum that the direct fp32 MFMA
kernel, the bf16 MFMA kernels (operands <= 3 significant bits: exact in bf16), the split-operand GEMM (an exact bf16 value splits
as (v, 0, 0)), the scalar-weight streaming kernel or Winograd F(2x2, 3x3) (G holds 1 and 1/2, B and A only +-1) can form is then a
multiple of 2^-3 (2^-2 from G g G^T, times the 0.5 scale) no larger than the case's `bound`, which is below 2^24 of those units:
every intermediate is exactly representable in fp32, so the result equals the float64 reference BIT FOR BIT at every element in
any tiling and any summation order.  The bound is 81 A max|scale| + max|shift| for the 3x3 cases (A = the largest sum over the
contracted channels of max|x_c| max|w_c|; 81 = F(2x2)'s gains: 4 on V, 9/4 on U, 9 terms in an output sum; the nine taps of the
direct form fit under it) and A max|scale| + max|shift| for the 1x1 cases.

**F(4x4, 3x3): per element.**  Its B^T is not dyadic, so the kernels round.  `wino4_twin` restates conv2d_wino4.hip's g_row, bt_vec
and at_vec (same constants, same grouping of the additions) with the channel sum in channel order; in float64 it equals conv2d to
1e-12, in float32 it is the yardstick: |y - y64| <= max(4 x the twin's figure, 4 x 2^-24) x scale_of at EVERY element, the figure
being the largest |err| / scale_of of the twin on the case's own inputs (the rule of train_tail_cases.py / head_cases.py).
`scale_of` is the float64 conv of |x| and |w| maximised over each 4x4 output tile (a Winograd tile mixes its 36 patch values),
carried through the epilogue as S |scale| + |shift|.  `wino4_twin_two_pieces` drops the third bf16 piece of V (a 2^-16 error) and
exists for the CPU sharpness check only: it passes the whole-tensor 1e-4 max|ref| bar of test_gpu_wino4.py and misses this one.

The case tables (one per kernel; the edge each case sits on is in its `edge` string):

  CONV2D        conv2d_fwd: all eight conv2d_kernel<CT 4|1, TAPS 9|1, VEC 4|1>; Cin 1, 5, 8, 9, 17, 40 (ragged last K chunk of 8 and of
                16); Cout 1, 31, 32, 33, 64, 65, 128, 129 (pad to 32 / to 128, a second cout group); H W below a tile, one pixel / one
                quad above it, B = 3 tile tails, W = 2 x H = 150 (narrow: a 160-pixel tile spans 80 rows; the wide form refuses W = 2
                -- its staged patch of 147 rows needs 184 KB of LDS -- so the wide 1-pixel-stride case is W = 3 x H = 100: 96 rows),
                W % 4 != 0 with wide Cout, the widest W of every VEC = 4 form (312: `ps == MAXPJ * 4 * 256` exactly; 248 is the
                widest W with five patch rows, 204 with three at KC = 16 -- each with its first refused width), x misaligned by
                one float (the register-staged VEC = 1 form)
  NARROW        conv1x1_narrow_fwd: Cout at every pad and the first channel after it, Cin 1, 3, 4, 5, 7, 256, H W 1, 63, 64, 65, B = 3
  WINO2         conv2d_wino_fwd: Cin 32 / 64, Cout 32 / 64 / 96 (half-filled 64-cout workgroup), maps from the smallest legal (2, 64)
                to (10, 100): a 32-tile group ends mid-row, spans two tile rows, crosses an image
  GEMM1X1       conv1x1_gemm_fwd: H W = every block width (64 .. 192), 384 on the split form, and 5504 x B = 3, the smallest map
                whose fp32-MFMA form runs 128-column blocks (the 192-column form is never picked from this entry)
  BF16_3X3      conv2d_bf16_fwd: Cin 1 .. 70 around the 32-channel chunk, Cout 32 / 64 / 96, H = 1, odd H, partial last tile column,
                forced workgroup counts; the data gradient through autograd's transposed, tap-mirrored pack
  BF16_1X1      conv1x1_bf16_fwd: both ends of every k-step range of Cin, a masked last 64-channel group, partial pixel tiles; forward
                and the transposed pack
  INFER_3X3 / INFER_1X1   the bf16-map inference forms: Cout 1, 20, 28, 32, 33 (zero rows up to 32), fp32 and bf16 store -- the
                bf16 store is round-to-nearest-even of an exactly known value, and lattice sums land on exact ties
  WINO4         conv2d_wino4_fwd per geometry word 1..6, 11..16: T = 1, block - 1, block, block + 1 tiles and a B = 3 shape whose
                images end inside a block; word 0 on each side of w4_wide_pays; lattice, randn and one-live-channel inputs in turn
  CHAIN / TAIL  conv2d_wino4_chain for one and two layers (with a tile map over an input that is zero in a band),
                conv2d_wino4_chain_tail at Cout 1, 5, 28, 63, 64

Measured on an MI355X (per family the case nearest its bar; figures are the largest |err| / scale_of over the elements; twin =
float32 wino4_twin on the same inputs; bar = max(4 x twin, 4 x 2^-24)):

  family                                                   kernel     fp32 twin   bar
  every lattice family (133 tests of the exact file)       bit-equal  -           0
  wino4_fwd words 1..6 (fp32 MFMA), lattice                4.80e-07   4.25e-07    1.70e-06
  wino4_fwd words 1..6, randn                              5.85e-07   5.00e-07    2.00e-06
  wino4_fwd words 1..6, one live channel                   1.79e-06   1.59e-06    6.37e-06
  wino4_fwd words 11..16 (split operands), lattice         5.51e-07   4.46e-07    1.78e-06
  wino4_fwd words 11..16, randn                            5.72e-07   4.33e-07    1.73e-06
  wino4_fwd words 11..16, one live channel                 1.50e-06   9.99e-07    4.00e-06
  wino4_fwd word 0, T = 896 (128-column blocks), randn     7.03e-07   6.59e-07    2.64e-06
  wino4_fwd word 0, T = 897 (wide tile), one live channel  1.95e-06   2.17e-06    8.67e-06
  chain, one layer                                         1.47e-06   1.29e-06    5.15e-06
  chain, two layers end to end                             1.50e-08   1.90e-08    2.38e-07 (the floor)
  chain, the second layer alone on the first one's map     4.33e-07   4.36e-07    1.74e-06
  chain tail, both layers end to end                       4.04e-08   3.96e-08    2.38e-07 (the floor)
  chain tail, y_prev (the previous layer's map)            6.12e-07   4.63e-07    1.85e-06
  chain tail, the tail layer alone on y_prev               2.27e-07   1.74e-07    6.97e-07

No kernel is above 0.38 of its bar.  The end-to-end figures of two layers are small because the scale of the first layer, pushed
through |w| of the second, is a worst case that random signs never reach: their bar is the floor, and a GEMM that drops one of the
eight piece products passes it.  The layer-alone rows hold the second layer on the very map it consumed and do catch it.
"""
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

Q = 3                                   # lattice grid 2^-Q: 2^-2 (F(2x2)'s G g G^T) x the 0.5 scale
FLOOR = 4.0 * 2.0 ** -24
SCALES = (-1.0, 0.5, 1.0, 2.0, 4.0)
HIP_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sa-ssd_amd", "csrc")


def bar(fp32_figure):
    return max(4.0 * fp32_figure, FLOOR)


# ------------------------------------------------------------------------------------------------- lattice cases
def epilogue(acc, scale, shift, relu):
    """relu?(acc * scale + shift) per output channel in the dtype of acc (float64 for the references)"""
    y = acc
    if scale is not None:
        y = y * scale.to(acc.dtype).view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.to(acc.dtype).view(1, -1, 1, 1)
    return torch.relu(y) if relu else y


FORMS = ("scale+shift", "shift", "none")


def form_args(c, form):
    """(scale, shift) of one of the three epilogue forms every case runs in"""
    return {"scale+shift": (c["scale"], c["shift"]), "shift": (None, c["shift"]), "none": (None, None)}[form]


@functools.lru_cache(maxsize=None)
def lattice_case(kind, b, cin, cout, h, w, seed):
    """kind: '3x3' | '1x1' (forward: x [b, cin, h, w] -> [b, cout, h, w]) or '3x3_dgrad' | '1x1_dgrad' (data gradient of that layer:
    x is dy [b, cout, h, w] -> [b, cin, h, w] = conv_transpose2d).  w is always the forward layer's [cout, cin, k, k].
    -> dict(x, w, scale, shift (per OUTPUT channel), acc = the float64 reference before the epilogue, bound, nout)."""
    ks = 3 if kind.startswith("3x3") else 1
    dgrad = kind.endswith("_dgrad")
    g = torch.Generator().manual_seed(seed)
    nin, nout = (cout, cin) if dgrad else (cin, cout)
    x = torch.randint(0, 9, (b, nin, h, w), generator=g).float() - 4.0            # one value in nine is 0
    wt = torch.randint(-4, 5, (cout, cin, ks, ks), generator=g).float()
    scale = torch.tensor(SCALES)[torch.randint(0, len(SCALES), (nout,), generator=g)]
    shift = torch.randint(-32, 33, (nout,), generator=g).float() * 0.25
    if dgrad:
        acc = F.conv_transpose2d(x.double(), wt.double(), None, 1, ks // 2)
    else:
        acc = F.conv2d(x.double(), wt.double(), None, 1, ks // 2)
    c = dict(kind=kind, ks=ks, dgrad=dgrad, x=x, w=wt, scale=scale, shift=shift, acc=acc, nout=nout)
    c["bound"] = lattice_bound(c)
    return c


def lattice_bound(c):
    """largest |value| any of the algorithms can form on this case, in units of 2^-Q (docstring above)"""
    xm = c["x"].abs().amax(dim=(0, 2, 3)).double()                                 # per contracted channel
    wm = c["w"].abs().amax(dim=(2, 3)).double()                                     # [cout, cin]
    a = (wm * xm.view(-1, 1)).sum(0).max() if c["dgrad"] else (wm * xm.view(1, -1)).sum(1).max()
    gain = 81.0 if c["ks"] == 3 else 1.0
    return float((gain * a * c["scale"].abs().max() + c["shift"].abs().max()) * 2.0 ** Q)


def lattice_ref(c, form, relu, dtype=torch.float32):
    sc, sh = form_args(c, form)
    return epilogue(c["acc"], sc, sh, relu).to(dtype)


# ------------------------------------------------------------------------------------------------- poison around a tensor
_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}


def embed(t, pad_elems=96, poison=float("nan"), device=None, misalign=0):
    """t as a contiguous view inside a larger buffer filled with `poison` (NaN around inputs: a stray read is in bounds and turns
    the output into NaN; 7.0 around outputs).  The view starts 16-byte aligned, or `misalign` elements past such an address.
    -> (buffer, view)"""
    device = t.device if device is None else device
    n, esz = t.numel(), t.element_size()
    buf = torch.full((n + 2 * pad_elems + 16 // esz + misalign,), poison, dtype=t.dtype, device=device)
    off = pad_elems
    while (buf.data_ptr() + off * esz) % 16:
        off += 1
    off += misalign
    view = buf[off:off + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and (view.data_ptr() - misalign * esz) % 16 == 0
    return buf, view


def check_surround(buf, view, poison):
    """every byte of `buf` outside `view` still holds the poison"""
    esz = buf.element_size()
    off, n = (view.data_ptr() - buf.data_ptr()) // esz, view.numel()
    bits = buf.view(_BITS[buf.dtype])
    want = torch.full((1,), poison, dtype=buf.dtype).view(_BITS[buf.dtype]).item()
    bad = int((bits[:off] != want).sum().item()) + int((bits[off + n:] != want).sum().item())
    assert bad == 0, "%d elements around the tensor were overwritten" % bad


# ------------------------------------------------------------------------------------------------- F(4x4, 3x3) twin
# conv2d_wino4.hip: the constants of bt_vec as the rationals its comment names, next to the literals of the source
BT_CONST = {"3.00444444f": (676, 225), "1.13777778f": (256, 225), "1.54890756f": (4608, 2975), "0.688403361f": (2048, 2975),
            "0.968067227f": (576, 595), "0.430252101f": (256, 595), "0.119514472f": (128, 1071), "0.0466853408f": (50, 1071),
            "0.179271709f": (64, 357), "0.0700280112f": (25, 357), "0.87890625f": (225, 256), "2.640625f": (169, 64)}


def _k(name, dt):
    n, d = BT_CONST[name]
    return dt(n / d) if dt is np.float64 else dt(np.float32(float(name[:-1])))


def g_row(g0, g1, g2, dt):
    e, f = g0 + dt(0.390625) * g2, dt(0.625) * g1
    e2, f2 = g0 + dt(2.25) * g2, dt(1.5) * g1
    return [g0, e + f, e - f, e2 + f2, e2 - f2, g2]


def bt_vec(d, dt):
    k = lambda s: _k(s, dt)                                                                  # noqa: E731
    o0 = d[0] - k("3.00444444f") * d[2] + k("1.13777778f") * d[4]
    s, t = k("1.54890756f") * d[2] - k("0.688403361f") * d[4], k("0.968067227f") * d[1] - k("0.430252101f") * d[3]
    u, v = k("0.119514472f") * d[4] - k("0.0466853408f") * d[2], k("0.179271709f") * d[3] - k("0.0700280112f") * d[1]
    o5 = k("0.87890625f") * d[1] - k("2.640625f") * d[3] + d[5]
    return [o0, s + t, s - t, u + v, u - v, o5]


def at_vec(m, dt):
    s1, d1, s2, d2 = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4]
    return [m[0] + s1 + s2, dt(0.625) * d1 + dt(1.5) * d2, dt(0.390625) * s1 + dt(2.25) * s2,
            dt(0.244140625) * d1 + dt(3.375) * d2 + m[5]]


def _bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a)).bfloat16().float().numpy()


def wino4_twin(x, w, dtype, scale=None, shift=None, relu=False, pieces=3):
    """F(4x4, 3x3) pad-1 conv of x [B, C, H, W] with w [Cout, C, 3, 3] (+ the epilogue) in `dtype` (np.float64: proves the
    matrices; np.float32: the twin), written as conv2d_wino4.hip computes it: wino4_pack_kernel (g_row down the filter's columns,
    then along the rows), wino4_in_kernel (bt_vec on the patch's columns, then on its rows), the channel sum in channel order,
    wino4_out_kernel (at_vec on the columns, then the rows, then o * scale + shift and the ReLU).  pieces = 2: V loses its third
    bf16 piece."""
    dt = dtype
    x = np.asarray(x, dt)
    w = np.asarray(w, dt)
    B, C, H, W = x.shape
    cout = w.shape[0]
    th, tw = H // 4, W // 4
    T = B * th * tw
    t = [g_row(w[:, :, 0, c], w[:, :, 1, c], w[:, :, 2, c], dt) for c in range(3)]            # t[c][r] : [cout, C]
    U = np.empty((6, 6, C, cout), dt)
    for r in range(6):
        o = g_row(t[0][r], t[1][r], t[2][r], dt)
        for c in range(6):
            U[r, c] = o[c].T
    xp = np.zeros((B, C, H + 2, W + 2), dt)
    xp[:, :, 1:-1, 1:-1] = x
    d = [[xp[:, :, i:i + 4 * th:4, j:j + 4 * tw:4] for j in range(6)] for i in range(6)]      # d[i][j] : [B, C, th, tw]
    u = [[None] * 6 for _ in range(6)]
    for j in range(6):
        o = bt_vec([d[i][j] for i in range(6)], dt)
        for i in range(6):
            u[i][j] = o[i]
    V = np.empty((6, 6, C, T), dt)
    for i in range(6):
        o = bt_vec(u[i], dt)
        for j in range(6):
            V[i, j] = o[j].transpose(1, 0, 2, 3).reshape(C, T)
    if pieces == 2:
        assert dt is np.float32
        v1 = _bf16_round(V)
        V = v1 + _bf16_round(V - v1)
    M = np.zeros((6, 6, cout, T), dt)
    for ci in range(C):
        M += U[:, :, ci, :, None] * V[:, :, ci, None, :]
    v = [[None] * 6 for _ in range(4)]
    for j in range(6):
        o = at_vec([M[i, j] for i in range(6)], dt)
        for i in range(4):
            v[i][j] = o[i]
    y = np.empty((B, cout, H, W), dt)
    sc = None if scale is None else np.asarray(scale, dt).reshape(1, -1, 1, 1)
    sh = None if shift is None else np.asarray(shift, dt).reshape(1, -1, 1, 1)
    for i in range(4):
        o = at_vec(v[i], dt)
        for j in range(4):
            y[:, :, i::4, j::4] = o[j].reshape(cout, B, th, tw).transpose(1, 0, 2, 3)
    if sc is not None:
        y = y * sc
    if sh is not None:
        y = y + sh
    if relu:
        y = np.maximum(y, dt(0))
    assert y.dtype == dt
    return y


def wino4_twin_two_pieces(x, w, scale=None, shift=None, relu=False):
    return wino4_twin(x, w, np.float32, scale, shift, relu, pieces=2)


def tile_max(s, tile=4):
    """s [B, C, H, W] -> the same shape, every element the maximum of its tile x tile block"""
    b, c, h, w = s.shape
    m = s.reshape(b, c, h // tile, tile, w // tile, tile).amax(dim=(3, 5), keepdim=True)
    return m.expand(b, c, h // tile, tile, w // tile, tile).reshape(b, c, h, w)


def scale_of(x, w, scale=None, shift=None, tile=4):
    """float64 conv2d of |x| and |w| (pad k/2), for F(4x4) maximised over each 4x4 output tile (tile = 0: per element), carried
    through the epilogue: S |scale| + |shift|"""
    ks = w.shape[-1]
    s = F.conv2d(torch.as_tensor(x).double().abs(), torch.as_tensor(w).double().abs(), None, 1, ks // 2)
    if tile:
        s = tile_max(s, tile)
    if scale is not None:
        s = s * torch.as_tensor(scale).double().abs().view(1, -1, 1, 1)
    if shift is not None:
        s = s + torch.as_tensor(shift).double().abs().view(1, -1, 1, 1)
    return s


def figure(y, ref, scale):
    """largest |y - ref| / scale over the elements; where the scale is 0 the value must be exactly the reference"""
    y, ref, scale = (np.asarray(a, np.float64) for a in (y, ref, scale))
    live = scale > 0
    assert np.all(np.isfinite(y)), "not finite"
    assert np.array_equal(y[~live], ref[~live]), "a value with no terms differs from the reference"
    return float((np.abs(y - ref)[live] / scale[live]).max()) if live.any() else 0.0


def wino4_inputs(kind, b, cin, cout, h, w, seed):
    """-> x, w, scale, shift (torch fp32).  'lattice': the exact-file operands (the reference is known exactly, only the
    transforms round); 'randn': full-mantissa operands at the BEV layers' weight scale; 'one_live': one input channel carries
    data, so sum |x| |w| is small next to the transforms' intermediate values"""
    g = torch.Generator().manual_seed(seed)
    if kind == "lattice":
        x = torch.randint(0, 9, (b, cin, h, w), generator=g).float() - 4.0
        wt = torch.randint(-4, 5, (cout, cin, 3, 3), generator=g).float()
        sc = torch.tensor(SCALES)[torch.randint(0, len(SCALES), (cout,), generator=g)]
        sh = torch.randint(-32, 33, (cout,), generator=g).float() * 0.25
        return x, wt, sc, sh
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    if kind == "one_live":
        live = int(torch.randint(0, cin, (1,), generator=g))
        keep = torch.zeros(cin)
        keep[live] = 1.0
        x = x * keep.view(1, -1, 1, 1)
    else:
        assert kind == "randn"
    sc = torch.rand(cout, generator=g) + 0.5
    sc[::3] *= -1.0                                                     # the ReLU behind a sign change
    sh = torch.randn(cout, generator=g) * 0.1
    return x, wt, sc, sh


def layer_alone(x, wt, sc, sh, relu=True):
    """one F(4x4) layer on the map x (fp32, possibly a kernel's own output): the float64 reference, the scale, the fp32 twin's
    figure and the bar it gives"""
    ref = epilogue(F.conv2d(x.double(), wt.double(), None, 1, 1), sc, sh, relu).numpy()
    s = scale_of(x, wt, sc, sh).numpy()
    twin = wino4_twin(x.numpy(), wt.numpy(), np.float32, sc.numpy(), sh.numpy(), relu)
    fig = figure(twin, ref, s)
    return dict(x=x, w=wt, scale=sc, shift=sh, relu=relu, ref=ref, scale_of=s, twin_figure=fig, bar=bar(fig))


@functools.lru_cache(maxsize=None)
def wino4_case(kind, b, cin, cout, h, w, seed, relu=True):
    """one F(4x4) layer on the inputs of wino4_inputs"""
    return layer_alone(*wino4_inputs(kind, b, cin, cout, h, w, seed), relu)


# ------------------------------------------------------------------------------------------------- host arithmetic, restated
def cdiv(a, b):
    return (a + b - 1) // b


def conv2d_plan(cout, ks, h, w, aligned=True):
    """sassd_conv2d_fwd_cfg + launch_conv of conv2d.hip restated: -> dict(inst=(CT, TAPS, VEC), ok, ps, NPR, PW, lds).
    conv2d.hip:  P.PW = (P.W + 8 + 3) / 4 * 4;  P.NPR = (C::PIX - 1 + P.W - 1) / P.W + 1 + 2 * C::HALO;
                 ps = (KC * NPR * PW + 255) / 256 * 256;  stage = 2 * (WS + ps) * 4;  red = KSPLIT ? 4 * NSEG * 16 * 64 * 4 : 0;
                 lds = max(stage, red) + 1024;  if (lds > 160 * 1024) return SASSD_EINVAL;
                 if (VEC == 4 ? (ps > MAXPJ * 4 * 256) : (KC * NPR * W > 256 * MAXLP)) return SASSD_EINVAL;"""
    cout_pad = cdiv(cout, 128) * 128 if cout > 64 else cdiv(cout, 32) * 32
    ct = 4 if cout_pad % 128 == 0 else 1
    taps = ks * ks
    vec = 4 if (w % 4 == 0 and aligned) else 1
    nseg, kc, halo = (9 if ct == 4 else 5), (8 if taps == 9 else 16), (1 if taps == 9 else 0)
    pix, ws = nseg * 32, taps * kc * ct * 32
    pw = (w + 8 + 3) // 4 * 4
    npr = (pix - 1 + w - 1) // w + 1 + 2 * halo
    ps = cdiv(kc * npr * pw, 256) * 256
    stage = 2 * (ws + ps) * 4
    red = 4 * nseg * 16 * 64 * 4 if ct == 1 else 0
    lds = max(stage, red) + 1024
    ok = h >= 1 and w >= 2 and lds <= 160 * 1024
    ok = ok and (ps <= 10 * 4 * 256 if vec == 4 else kc * npr * w <= 256 * 40)
    return dict(inst=(ct, taps, vec), ok=ok, ps=ps, NPR=npr, PW=pw, lds=lds, pix=pix, kc=kc)


def w4_pick_wn(T, cout, np_=36, exact=False):
    """w4_pick_wn of conv2d_wino4.hip: the fp32-MFMA GEMM's block width in 32-column units"""
    best, best_cost = (0 if exact else 4), 1e30
    for wn in range(2, 7):
        bn = 32 * wn
        if exact and T % bn:
            continue
        lds = 2 * (128 + bn) * 32 * 4
        wgs = max(1, min(160 * 1024 // lds, 32 // (2 * wn)))
        units = np_ * (cout // 128) * cdiv(T, bn)
        rounds = (units + 256 * wgs - 1) // (256 * wgs)
        cost = float(rounds * wgs * bn)
        if cost < best_cost - 1e-9:
            best_cost, best = cost, wn
    return best


def w4_wide_pays(T, cout):
    """conv2d_wino4.hip:  small = 36L * (Cout / kBM) * cdiv(T, 128), wide = 36L * (Cout / (2 * kBM)) * cdiv(T, 192);
                          return 2 * ((wide + 511) / 512) < (small + 511) / 512;"""
    small, wide = 36 * (cout // 128) * cdiv(T, 128), 36 * (cout // 256) * cdiv(T, 192)
    return 2 * ((wide + 511) // 512) < (small + 511) // 512


def w4_block(T, cout, geo):
    """columns per workgroup of the Winograd GEMM under geometry word `geo` (w4_tile(...).bn())"""
    if 2 <= geo <= 6:
        return 32 * geo
    if 11 <= geo <= 13:
        return 64 * (geo - 10)
    if geo == 14:
        return 128
    if geo == 15:
        return 192
    if geo == 16:
        return 256
    if geo == 1:
        return 32 * w4_pick_wn(T, cout)
    return 192 if w4_wide_pays(T, cout) else 128


def hip_source(name):
    with open(os.path.join(HIP_DIR, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------- the case tables
def _c(name, edge, **kw):
    return dict(name=name, edge=edge, **kw)


CONV2D = [
    _c("<1,9,4>-below-a-tile", "H W = 24 < 160, Cin 1, Cout 1", ks=3, b=1, cin=1, cout=1, h=3, w=8),
    _c("<1,9,4>-quad-above-a-tile", "H W = 164 = 160 + 4, B = 3, Cout 33: two cout groups, the second one padded", ks=3, b=3, cin=9,
       cout=33, h=41, w=4),
    _c("<1,9,4>-widest", "W = 312: ps == 10240 exactly (four patch rows)", ks=3, b=1, cin=8, cout=32, h=3, w=312),
    _c("<1,9,1>-one-above-a-tile", "H W = 161, W = 23, B = 3, Cin 5 (ragged chunk of 8), Cout 31", ks=3, b=3, cin=5, cout=31, h=7, w=23),
    _c("<1,9,1>-W2-H150", "a 160-pixel tile spans 80 rows", ks=3, b=1, cin=8, cout=32, h=150, w=2),
    _c("<1,9,1>-misaligned-x", "x one float past a 16-byte address, W % 4 == 0", ks=3, b=1, cin=8, cout=32, h=5, w=8, misalign=1),
    _c("<1,1,4>-quad-above-a-tile", "H W = 164, B = 3, Cin 17 (ragged chunk of 16), Cout 64", ks=1, b=3, cin=17, cout=64, h=41, w=4),
    _c("<1,1,4>-widest", "W = 312: ps == 10240 exactly (two patch rows)", ks=1, b=1, cin=17, cout=31, h=3, w=312),
    _c("<1,1,1>-one-above-a-tile", "H W = 161, Cin 40, Cout 33", ks=1, b=1, cin=40, cout=33, h=7, w=23),
    _c("<1,1,1>-W2-H150", "a 160-pixel tile spans 80 rows, Cout 1", ks=1, b=3, cin=17, cout=1, h=150, w=2),
    _c("<4,9,4>-below-a-tile", "H W = 24 < 288, Cin 40, Cout 129: two 128-cout groups", ks=3, b=1, cin=40, cout=129, h=3, w=8),
    _c("<4,9,4>-quad-above-a-tile", "H W = 292 = 288 + 4, B = 3, Cin 9, Cout 65", ks=3, b=3, cin=9, cout=65, h=73, w=4),
    _c("<4,9,4>-widest", "W = 312: ps == 10240 exactly (four patch rows)", ks=3, b=1, cin=9, cout=65, h=3, w=312),
    _c("<4,9,4>-widest-five-rows", "W = 248: ps == 10240 exactly with five patch rows", ks=3, b=1, cin=5, cout=128, h=3, w=248),
    _c("<4,9,1>-one-above-a-tile", "H W = 289, W = 17: W % 4 != 0 with wide Cout, B = 3, Cin 17", ks=3, b=3, cin=17, cout=128, h=17, w=17),
    _c("<4,9,1>-W3-H100", "a 288-pixel tile spans 96 rows", ks=3, b=1, cin=5, cout=65, h=100, w=3),
    _c("<4,1,4>-row-above-a-tile", "H W = 296 = 288 + one row of W = 8 (W = 4 needs 73 patch rows of 16 channels: refused), Cin 40, "
       "Cout 129", ks=1, b=1, cin=40, cout=129, h=37, w=8),
    _c("<4,1,4>-widest", "W = 312: ps == 10240 exactly (two patch rows)", ks=1, b=1, cin=5, cout=128, h=3, w=312),
    _c("<4,1,4>-widest-three-rows", "W = 204: the widest W with three patch rows", ks=1, b=1, cin=8, cout=65, h=3, w=204),
    _c("<4,1,1>-one-above-a-tile", "H W = 289, W = 17, B = 3, Cin 1, Cout 65", ks=1, b=3, cin=1, cout=65, h=17, w=17),
    _c("<4,1,1>-misaligned-x", "x one float past a 16-byte address", ks=1, b=1, cin=9, cout=128, h=5, w=8, misalign=1),
]
# widths launch_conv must refuse (the first one past an accepted edge; W = 2 on the wide forms: the patch does not fit the LDS)
CONV2D_REFUSED = [
    _c("<1,9,4>-316", "one quad past the widest", ks=3, cin=8, cout=32, h=3, w=316),
    _c("<1,1,4>-316", "one quad past the widest", ks=1, cin=8, cout=32, h=3, w=316),
    _c("<4,9,4>-316", "one quad past the widest", ks=3, cin=8, cout=128, h=3, w=316),
    _c("<4,1,4>-316", "one quad past the widest", ks=1, cin=8, cout=128, h=3, w=316),
    _c("<4,9,4>-252", "one quad past the widest five-row width", ks=3, cin=8, cout=128, h=3, w=252),
    _c("<4,1,4>-208", "one quad past the widest three-row width", ks=1, cin=8, cout=128, h=3, w=208),
    _c("<4,9,1>-W2", "147 patch rows: 184 KB of LDS", ks=3, cin=8, cout=128, h=150, w=2),
    _c("<4,1,1>-W2", "145 patch rows of 16 channels", ks=1, cin=8, cout=128, h=150, w=2),
]

_NARROW_COUT = (1, 8, 9, 16, 17, 20, 21, 24, 25, 28, 29, 32)
_NARROW_CIN = (1, 3, 4, 5, 7, 256)
_NARROW_HW = ((1, 1), (7, 9), (8, 8), (5, 13))
NARROW = [_c("cout%d-cin%d-hw%d" % (co, _NARROW_CIN[i % 6], _NARROW_HW[(i + i // 6) % 4][0] * _NARROW_HW[(i + i // 6) % 4][1]),
             "pad %s, wave shares of ceil(Cin / 4) channels" % ("full" if co in (8, 16, 20, 24, 28, 32) else "first channel after a pad"),
             b=3, cin=_NARROW_CIN[i % 6], cout=co, h=_NARROW_HW[(i + i // 6) % 4][0], w=_NARROW_HW[(i + i // 6) % 4][1])
          for i, co in enumerate(_NARROW_COUT)]

WINO2 = [
    _c("smallest-map", "H = 2, W = 64: one tile row of 32 tiles", b=1, cin=32, cout=32, h=2, w=64),
    _c("group-ends-mid-row", "TW = 34: every 32-tile group ends inside a row; B = 2", b=2, cin=64, cout=64, h=2, w=68),
    _c("two-tile-rows-b3", "B = 3, Cout 96: a half-filled 64-cout workgroup", b=3, cin=32, cout=96, h=4, w=64),
    _c("group-spans-rows", "TW = 36, TH = 3: groups span two tile rows", b=1, cin=64, cout=96, h=6, w=72),
    _c("group-crosses-image", "TW = 50, TH = 5: 250 tiles per image, groups cross the images of B = 2", b=2, cin=32, cout=64, h=10, w=100),
    _c("mid-row-b3", "TW = 34, B = 3: 102 tiles, the last group holds 6", b=3, cin=64, cout=32, h=2, w=68),
]

GEMM1X1 = [
    _c("hw64", "only the 64-column block divides H W", b=1, cin=32, cout=128, h=8, w=8),
    _c("hw96", "only the 96-column block", b=3, cin=64, cout=384, h=8, w=12),
    _c("hw160", "only the 160-column block", b=3, cin=32, cout=384, h=10, w=16),
    _c("hw128", "128 columns: the split form unless the fp32 MFMA is asked for", b=1, cin=64, cout=128, h=8, w=16),
    _c("hw192", "64, 96 and 192 divide H W", b=1, cin=32, cout=384, h=12, w=16),
    _c("hw384-b3", "three 128-column blocks per image on the split form, B = 3", b=3, cin=64, cout=128, h=16, w=24),
    _c("hw5504-b3", "the smallest map whose fp32-MFMA form takes 128-column blocks (w4_pick_wn's rounds model: 64-column blocks win "
       "every tie, so 128 needs 769 units; 192 columns never win from this entry)", b=3, cin=32, cout=384, h=43, w=128),
]

BF16_3X3 = [
    _c("cin1-h1", "Cin 1, H = 1, one 16-column tile", kind="3x3", b=3, cin=1, cout=32, h=1, w=16),
    _c("cin8-w20", "partial last tile column (W = 20)", kind="3x3", b=3, cin=8, cout=64, h=2, w=20),
    _c("cin31-odd-h", "Cin 31, odd H, W = 36, Cout 96", kind="3x3", b=3, cin=31, cout=96, h=5, w=36),
    _c("cin32-w188", "one whole chunk, the 188-wide map", kind="3x3", b=3, cin=32, cout=32, h=3, w=188),
    _c("cin33-odd-h", "one channel into the second chunk", kind="3x3", b=3, cin=33, cout=64, h=5, w=36),
    _c("cin70-w20", "three chunks, the last holds 6 channels", kind="3x3", b=3, cin=70, cout=96, h=2, w=20),
    _c("dgrad-33-to-32", "data gradient: dy with 33 channels -> 32", kind="3x3_dgrad", b=3, cin=32, cout=33, h=5, w=36),
    _c("dgrad-8-to-96", "data gradient: dy with 8 channels -> 96", kind="3x3_dgrad", b=3, cin=96, cout=8, h=2, w=20),
]

_C1_CIN = (1, 16, 17, 32, 49, 64, 113, 128, 241, 256)
_C1_COUT = (1, 63, 64, 65, 130)
_C1_HW = ((1, 4), (5, 12), (8, 8), (4, 17))
BF16_1X1 = [_c("k%d-n%d-hw%d" % (ci, _C1_COUT[i % 5], _C1_HW[(i + i // 5) % 4][0] * _C1_HW[(i + i // 5) % 4][1]),
               "Cin at an end of a k-step range; 64-channel groups: %d" % cdiv(_C1_COUT[i % 5], 64),
               b=2, k=ci, n=_C1_COUT[i % 5], h=_C1_HW[(i + i // 5) % 4][0], w=_C1_HW[(i + i // 5) % 4][1])
            for i, ci in enumerate(_C1_CIN)]

_INF_COUT = (1, 20, 28, 32, 33)
INFER_3X3 = [_c("cout%d" % co, "Cout padded to 32 with zero rows", b=2, cin=(8, 33)[i % 2], cout=co, h=(5, 2)[i % 2], w=(36, 20)[i % 2])
             for i, co in enumerate(_INF_COUT)]
INFER_1X1 = [_c("cout%d" % co, "a masked 64-channel group", b=2, cin=(17, 64, 113)[i % 3], cout=co, h=(5, 4)[i % 2], w=(12, 17)[i % 2])
             for i, co in enumerate(_INF_COUT)]


def _tiles_shape(T):
    """(H, W) with (H / 4) (W / 4) = T: the squarest factorisation (a prime T is one tile row)"""
    a = max(d for d in range(1, int(math.isqrt(T)) + 1) if T % d == 0)
    return 4 * a, 4 * (T // a)


_W4_KINDS = ("lattice", "randn", "one_live")


def _wino4_cases():
    out = []
    n = 0
    for geo in (1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15, 16):
        for which in ("one", "below", "block", "above", "b3"):
            cin, cout = (32, 64)[n % 2], (256, 512)[(n // 2) % 2]
            kind = _W4_KINDS[n % 3]
            # the block of word 1 depends on T itself: settle it at the block width T is chosen from
            bn = next(bn for bn in (64, 96, 128, 160, 192, 256) if w4_block(bn, cout, geo) == bn) if geo == 1 else w4_block(0, cout, geo)
            if which == "b3":
                per = bn // 3 + 1                                    # three images of `per` tiles: 3 per = bn + 1 .. bn + 3
                b, (h, w) = 3, _tiles_shape(per)
                edge = "B = 3, %d tiles per image: images end inside the %d-column blocks" % (per, bn)
            else:
                T = {"one": 1, "below": bn - 1, "block": bn, "above": bn + 1}[which]
                b, (h, w) = 1, _tiles_shape(T)
                edge = "T = %d against %d-column blocks" % (T, bn)
            out.append(_c("geo%d-%s" % (geo, which), edge, geo=geo, kind=kind, b=b, cin=cin, cout=cout, h=h, w=w, bn=bn, seed=1000 + n))
            n += 1
    return out


WINO4 = _wino4_cases()


def _wide_edge(cout):
    """smallest T at which w4_wide_pays(T, cout) holds"""
    return next(T for T in range(1, 100000) if w4_wide_pays(T, cout))


def _wino4_default_cases():
    out = []
    for cout, cin in ((512, 32),):                                    # (Cout 256 has its edge at T = 1793: a slower twin)
        te = _wide_edge(cout)
        for (T, side), kind in zip(((te - 1, "narrow"), (te, "wide")), ("randn", "one_live")):
            h, w = _tiles_shape(T)
            out.append(_c("geo0-cout%d-%s" % (cout, side), "T = %d: w4_wide_pays is %s" % (T, side == "wide"), geo=0, kind=kind, b=1,
                          cin=cin, cout=cout, h=h, w=w, T=T, wide=side == "wide", seed=2000 + T))
    return out


WINO4_DEFAULT = _wino4_default_cases()

CHAIN = [
    _c("one-layer-lattice", "conv2d_wino4_chain with its own output transform", layers=1, kind="lattice", b=1, cin=32, h=8, w=12, tile_map=False),
    _c("one-layer-b3", "B = 3, 15 tiles per image", layers=1, kind="one_live", b=3, cin=64, h=12, w=20, tile_map=False),
    _c("two-layers", "the map between the layers stays in the transform domain", layers=2, kind="randn", b=2, cin=32, h=8, w=16, tile_map=False),
    _c("two-layers-tile-map", "input zero in a band of rows, tile map, NaN workspace", layers=2, kind="randn", b=2, cin=64, h=16, w=12,
       tile_map=True),
]
TAIL = [_c("cout%d" % co, "narrow tail layer on a 64-channel block", cout=co, b=(1, 3)[i % 2], cin=32, h=8, w=(12, 8)[i % 2],
           kind=_W4_KINDS[i % 3]) for i, co in enumerate((1, 5, 28, 63, 64))]


@functools.lru_cache(maxsize=None)
def chain_case(kind, b, cin, h, w, seed, layers, tail_cout=0, band=False):
    """`layers` chained 3x3 layers cin -> 256 (-> 256), ReLU after each, optionally a narrow tail 256 -> tail_cout behind them:
    weights, the float64 reference of the LAST layer, its scale (the scale of every earlier layer, which bounds that layer's
    activations, pushed through |w| of the next one: ReLU is 1-Lipschitz, so an error in a map reaches the next layer through
    |w| at most), and the fp32 twin's figure over the same stack."""
    x, w0, sc0, sh0 = wino4_inputs(kind, b, cin, 256, h, w, seed)
    if band:
        x[:, :, : h // 2] = 0.0                                       # the tile map's inactive tiles
    ws, scs, shs = [w0], [sc0], [sh0]
    couts = [256] * layers + ([tail_cout] if tail_cout else [])
    for i, co in enumerate(couts[1:]):
        _, wi, sci, shi = wino4_inputs("randn", 1, 256, co, 4, 4, seed + 17 * (i + 1))
        ws.append(wi), scs.append(sci), shs.append(shi)
    a64, s, a32 = x.double(), None, x.numpy()
    for wi, sci, shi in zip(ws, scs, shs):
        s_in = a64.abs() if s is None else s
        s = tile_max(F.conv2d(s_in, wi.double().abs(), None, 1, 1)) * sci.double().abs().view(1, -1, 1, 1) + shi.double().abs().view(1, -1, 1, 1)
        a64 = epilogue(F.conv2d(a64, wi.double(), None, 1, 1), sci, shi, True)
        a32 = wino4_twin(a32, wi.numpy(), np.float32, sci.numpy(), shi.numpy(), True)
    fig = figure(a32, a64.numpy(), s.numpy())
    return dict(x=x, ws=ws, scales=scs, shifts=shs, ref=a64.numpy(), scale_of=s.numpy(), twin_figure=fig, bar=bar(fig))

