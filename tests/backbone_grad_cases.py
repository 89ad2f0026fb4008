"""References, fp32 twins, host geometry and seeded inputs of the fp32 backbone gradient kernel tests (test_backbone_grad_cases_cpu.py,
test_gpu_backbone_grad_kernels.py): numpy / torch-CPU only, nothing here touches a GPU.

A. sparse fp32 gradients (sassd_spconv_bwd_weight in both formulations, sassd_rulebook_transpose, sassd_spconv_bwd_data)
------------------------------------------------------------------------------------------------------------------------------
References are wgrad64 / transpose_table / sparse_conv64 of the bf16 tests on the fp32 operands.  Every operand is rounded to 12
significant bits (q12), so that a product is exact in fp32 (24 bits) as it is in the bf16 tests, and every rounding of a kernel is
one of its ADDITIONS.  Per element the bar is  min(d, m - 1) * 2^-24 * sum |terms|  (float64), m the number of products of the
element and d the longest chain of dependent fp32 additions of the kernel as built, counted as _wgrad_depth of
test_gpu_bf16_sparse_train.py counts it (the products inside one MFMA once, then one addition per MFMA step):

  weight gradient, offset per wave (default)   spconv_wgrad_offset_kernel compacts the pairs of one offset over a chunk of
      wg_rows = wgrad_rows_per_wg(cap) rows and runs v_mfma_f32_16x16x4_f32 steps of 4 pairs into one accumulator tile:
      4 products inside a step, ceil(min(wg_rows, n) / 4) steps at most; wgrad_reduce_kernel adds every 16th chunk per
      accumulator (ceil(nwg / 16)), its two accumulators (1), the 8 partial lanes (8) and the base of `accumulate` (1)
  weight gradient, tile per wave (cfg bit 5)    spconv_wgrad_kernel walks its 128-row chunk in 4-ROW steps, one MFMA per live
      offset and step: the same count with wg_rows = 128 (a step of rows without a pair adds zeros)
  data gradient (the forward kernels on the transposed table, or on the forward table of a submanifold layer)
      spconv_gs_kernel and the balanced kernel of spconv_gq.h accumulate a row's contributions in wave-private slab rows: the slab
      value is the C operand of a chain of C / 4 16x16x4 steps per pair (C the channels of dy), and the <= 8 slabs are added in
      wave order.  Which offsets share a wave depends on the dispatch and on the pair counts, so the chain is bounded by ALL steps
      of the row:  d = 4 + p * C / 4 + 7  with p the pairs of the row

B. BatchNorm + ReLU pairs (sassd_bn_relu_fwd / _bwd, sassd_bn2d_relu_fwd / _bwd, sassd_bn2d_stats)
------------------------------------------------------------------------------------------------------------------------------
bn_ref is float64 numpy on the fp32 inputs, channel-major [C, N]: mean, biased variance, invstd, running statistics (unbiased
variance, the biased one for N = 1), y, dbeta, dgamma, dx; with dt=np.float32 it is the fp32 twin (two-pass variance, cascaded
fp32 sums along the contiguous axis).  bn_case keeps every pre-activation z = (x - mean) * invstd * gamma + beta at least
Z_MARGIN away from 0:  Z_MARGIN[c] = Z_ULPS * 2^-24 * (max |x[c]| * invstd[c] * |gamma[c]| + |beta[c]|),  Z_ULPS = 256 ulp of the
largest term of z (the kernel's fp32 mean alone is wrong by up to max |x| * 2^-24, times invstd * gamma).  Offending x are moved
outward to 4 x the margin, the statistics recomputed, until none is left; |beta| >= 0.05 covers N = 1, where z = beta.  With the
margin the ReLU mask of the reference IS the kernel's, and gradients are compared unmasked.  Bars: bar() of the twin, references
divided by their scale (max |ref| for y and dx; the float64 sum of |terms| for the sums), never below FLOOR.

C. dense weight gradient (sassd_conv2d_bwd_weight, _bf16, _bf16_bnrelu)
------------------------------------------------------------------------------------------------------------------------------
Per element against float64 conv2d autograd (_wgrad_ref of test_gpu_bf16.py), scale = the same reference on |x|, |dy|, bar = bar()
of the same autograd on fp32 CPU tensors; the bf16 kernels against the reference (and twin) on the rounded operands; the
BatchNorm-in-the-loader form on relu(batchnorm(x)) as its loader forms it in fp32 from the affine triple, rounded to bf16.

Measured on the MI355X (largest figure of the family | its bar; the kernels add in double or in short fp32 chains and land far
below the worst-case bars, which stay where the rule puts them):

  family                                 figure   | bar      (the worst figure / bar ratio of the family over all its cases)
  sparse weight gradient
    rows                               5.95e-08 | 5.96e-08
    accumulate                         5.96e-08 | 5.96e-08
    rows, tile                         5.95e-08 | 5.96e-08
    accumulate, tile                   5.96e-08 | 5.96e-08
    empty offsets                      1.87e-07 | 2.80e-06
    empty offsets, tile                1.87e-07 | 2.80e-06
    ragged last step                   1.83e-07 | 2.80e-06
    ragged last step, tile             1.83e-07 | 2.80e-06
    reduce edges                       9.88e-08 | 1.19e-07
    reduce edges, tile                 9.88e-08 | 1.19e-07
    grown chunks                       7.84e-08 | 3.76e-06
    grown chunks, tile                 6.85e-08 | 2.80e-06
    waymo regime                       1.40e-07 | 1.04e-05
    waymo regime, tile                 4.52e-08 | 2.80e-06
    dynamic LDS                        1.08e-07 | 1.71e-05
    dynamic LDS, tile                  3.21e-08 | 2.86e-06
  sparse data gradient
    transposed table, down             1.39e-07 | 4.95e-06
    transposed table, subm             6.22e-08 | 3.28e-06
    forward table, subm                8.69e-08 | 5.42e-06
  bn_relu, C = 4 .. 256
    y                                  9.01e-08 | 3.30e-07
    mean                               5.94e-08 | 2.38e-07
    var                                3.68e-07 | 9.49e-07
    rmean                              5.55e-08 | 2.38e-07
    rvar                               5.45e-08 | 2.38e-07
    dbeta                              5.68e-08 | 2.38e-07
    dgamma                             2.31e-07 | 5.09e-07
    dx                                 2.08e-07 | 5.72e-07
  bn_relu (70001, 256)
    y                                  3.16e-06 | 1.30e-05
    mean                               4.04e-08 | 5.70e-07
    var                                2.06e-07 | 1.15e-06
    rmean                              5.12e-08 | 3.57e-07
    rvar                               5.84e-08 | 3.84e-07
    dbeta                              1.32e-09 | 2.38e-07
    dgamma                             6.36e-08 | 2.54e-07
    dx                                 1.82e-07 | 3.95e-07
  bn_relu (4099, 16)
    y                                  5.68e-07 | 2.28e-06
    mean                               2.76e-08 | 2.38e-07
    var                                9.58e-08 | 8.86e-07
    rmean                              3.69e-08 | 2.71e-07
    rvar                               5.24e-08 | 2.85e-07
    dbeta                              2.09e-09 | 2.38e-07
    dgamma                             1.96e-06 | 7.85e-06
    dx                                 8.68e-08 | 3.47e-07
  bn2d, the five small maps
    y                                  1.24e-07 | 4.56e-07
    mean                               3.44e-08 | 2.38e-07
    var                                7.23e-07 | 1.30e-06
    rmean                              4.21e-08 | 2.38e-07
    rvar                               3.95e-08 | 2.40e-07
    dbeta                              4.30e-08 | 2.38e-07
    dgamma                             1.88e-07 | 1.03e-06
    dx                                 2.46e-07 | 5.43e-07
  bn2d (1,512,132,256)
    y                                  4.64e-07 | 1.13e-05
    mean                               4.30e-08 | 5.84e-07
    var                                1.17e-07 | 1.28e-06
    rmean                              5.51e-08 | 4.47e-07
    rvar                               5.77e-08 | 4.23e-07
    dbeta                              2.92e-09 | 2.38e-07
    dgamma                             8.55e-07 | 2.08e-05
    dx                                 7.49e-08 | 4.73e-07
  dense weight gradient
    fp32 k=3                           8.42e-08 | 2.42e-07
    fp32 k=1                           5.27e-08 | 2.38e-07
    fp32 k=3 accumulate                6.38e-08 | 2.80e-07
    fp32 k=1 accumulate                7.24e-08 | 4.09e-07
    bf16 k=3                           4.16e-08 | 2.38e-07
    bf16 k=1                           3.08e-08 | 2.38e-07
    bf16 k=3 accumulate                5.40e-08 | 2.38e-07
    bf16 k=1 accumulate                4.14e-08 | 2.38e-07
    bf16 bnrelu k=3                    4.15e-08 | 2.38e-07
    bf16 bnrelu k=3 accumulate         6.11e-08 | 3.16e-07
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from train_tail_cases import figure, bar, FLOOR                                     # noqa: F401
from test_bf16_sparse_train_cpu import transpose_table, wgrad64
from test_bf16_sparse_infer_cpu import sparse_conv64
from test_gpu_bf16_sparse import _rand_rulebook
from test_gpu_bf16 import _wgrad_ref

U = 2.0 ** -24
KK = 27


def cdiv(a, b):
    return -(-a // b)


# ---- host geometry, restated (the cases are named for the regime they hit) ----------------------------------------------------
def wgrad_rows_per_wg(cap):
    r = ((cap + 511) // 512 + 63) // 64 * 64
    return min(max(r, 128), 2048)


def sparse_wgrad_geometry(n, cap, tile=False):
    """rows per chunk, chunks that hold rows, dynamic LDS of the pair lists (offset formulation), partials workspace"""
    rows = 128 if tile else wgrad_rows_per_wg(cap)
    return dict(wg_rows=rows, nchunk=cdiv(n, rows), lds_bytes=0 if tile else 8 * 2 * rows * 4, ws_chunks=cdiv(max(cap, 1), 128))


BN_MAX_BLOCKS = 1024


def bn_blocks(n, c):
    """-> (blocks, rows per block, most rows one thread adds)"""
    rl = 1024 // c
    it = min(max(n // (512 * rl), 2), 16)
    nb = min(max(cdiv(n, it * rl), 1), BN_MAX_BLOCKS)
    rpb = cdiv(n, nb)
    return cdiv(n, rpb), rpb, cdiv(min(rpb, n), rl)


BN2D_MAX_SPLIT = 16


def bn2d_geometry(c, hw):
    """-> (S, chunk, most float4 one thread adds per image)"""
    s = min(max(cdiv(1024, c), 1), BN2D_MAX_SPLIT)
    quads = hw // 4
    s = min(s, quads)
    chunk = cdiv(quads, s) * 4
    return cdiv(hw, chunk), chunk, cdiv(min(chunk, hw), 1024)


def wgrad_plan(b, cin, cout, h, w):
    nseg, n_ci_t, n_co_t = cdiv(w, 44), cdiv(cin, 64), cdiv(cout, 64)
    base = n_ci_t * n_co_t * b * nseg
    best, rows_per, nrange = -1, h, 1
    for nr in range(1, min(h, 64) + 1):
        rp = cdiv(h, nr)
        nrr = cdiv(h, rp)
        cost = cdiv(base * nrr, 512) * (rp + 2)
        if best < 0 or cost < best:
            best, rows_per, nrange = cost, rp, nrr
    return dict(nseg=nseg, nrange=nrange, rows_per=rows_per, n_ci_t=n_ci_t, n_co_t=n_co_t, nsplit=b * nseg * nrange,
                last_rows=h - (nrange - 1) * rows_per, last_cols=w - (nseg - 1) * 44)


# ---- A. sparse ------------------------------------------------------------------------------------------------------------------
WGRAD_PAIRS = [(16, 16), (16, 32), (32, 64), (64, 64)]
DGRAD_LAYERS = [(16, 16), (32, 16), (64, 32), (64, 64)]          # (Cin, Cout) of the layer: dy has Cout channels, dx Cin
DGRAD_ROWS = (1, 5, 31, 257, 4099)
EMPTY_OFFSETS = (0, 1, 2, 5, 20, 26)
MOD4_COUNTS = {3: 1, 4: 2, 6: 3, 7: 5, 8: 6, 9: 7, 10: 4}         # offset -> pairs, all inside the first 128-row chunk


DYN_LDS_CAP = 1088 * 512     # 1088-row chunks: 68 KB of pair lists, past the 64 KB a kernel gets without the dynamic-LDS opt-in
#                              (the 640-row chunks of the Waymo-scale capacity 317 000 take 40 KB: 64 bytes per row)


def q12(t):
    """fp32 tensor rounded to 12 significant bits: the product of two such values is exact in fp32"""
    m, e = torch.frexp(t.float())
    return torch.ldexp(torch.round(m * 4096.0) / 4096.0, e)


def wgrad_depth(n, cap, tile=False):
    g = sparse_wgrad_geometry(max(n, 1), cap, tile)
    return 4 + cdiv(min(g["wg_rows"], max(n, 1)), 4) + cdiv(g["nchunk"], 16) + 1 + 8 + 1


def dgrad_depth(pairs, c_dy):
    """pairs: array of pair counts per row -> the chain bound of each row"""
    return 4 + np.asarray(pairs, np.int64) * (c_dy // 4) + 7


def wgrad_cases(cin, cout):
    """(family, n, capacity, kind, empty offsets, planted pair counts) of one channel pair"""
    cases = [("rows", n, n + 50, kind, (), None) for n in (1, 3, 4, 5, 63, 64, 65, 127, 128, 129) for kind in ("down", "subm")]
    cases.append(("empty offsets", 200, 250, "down", EMPTY_OFFSETS, None))
    cases.append(("ragged last step", 200, 250, "down", (), tuple(sorted(MOD4_COUNTS.items()))))
    if (cin, cout) == (16, 16):
        cases += [("reduce edges", 128 * c - 125, 128 * c - 75, "down", (), None) for c in (1, 8, 9, 16, 17, 25)]
    cases.append(("grown chunks", 1000, 70000, "down", (7,), None))
    if (cin, cout) in ((16, 16), (16, 32)):
        cases.append(("waymo regime", 1500, 317000, "subm", (), None))
    if (cin, cout) == (16, 16):
        cases.append(("dynamic LDS", 2500, DYN_LDS_CAP, "down", (), None))
    return cases


@functools.lru_cache(maxsize=None)
def wgrad_case(cin, cout, n, cap, kind="down", empty=(), counts=None, seed=0):
    """-> (x [n_in, cin], dy [cap, cout], nbr [cap, 27] int32, n_in).  dy rows past n and x rows that no pair of the first n
    rows references are NaN; table rows past n hold valid indices; every index is -1 or inside [0, n_in)."""
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + n + cap + seed)
    n_in = n if kind == "subm" else n + n // 3 + 1
    nbr = _rand_rulebook(cap, n_in, kind, g, density=0.4)
    if kind == "subm":
        nbr[n:, 13] = 0
    for k in empty:
        nbr[:, k] = -1
    for k, c in (counts or ()):
        nbr[:n, k] = -1
        rows = torch.randperm(min(n, 100), generator=g)[:c]
        nbr[rows, k] = torch.randint(0, n_in, (c,), generator=g).int()
    x = q12(torch.randn(n_in, cin, generator=g))
    dy = q12(torch.randn(cap, cout, generator=g))
    dy[n:] = float("nan")
    used = torch.zeros(n_in, dtype=torch.bool)
    live = nbr[:n][nbr[:n] >= 0].long()
    used[live] = True
    x[~used] = float("nan")
    return x, dy, nbr, n_in


def wgrad_twin(x, dy, nbr, n):
    """fp32 twin: numpy float32, the pairs of an offset accumulated left to right (rows ascending)"""
    x, dy, nbr = x.numpy(), dy.numpy(), nbr.numpy()
    dw = np.zeros((KK, x.shape[1], dy.shape[1]), np.float32)
    for k in range(KK):
        for o in np.flatnonzero(nbr[:n, k] >= 0):
            dw[k] = dw[k] + np.outer(x[nbr[o, k]], dy[o]).astype(np.float32)
    return torch.from_numpy(dw)


def wgrad_check(dw, base, x, dy, nbr, n, d):
    """-> (largest |err| / sum |terms|, largest bar of an element, elements over their bar, pairs per offset)"""
    ref, mag, cnt = wgrad64(x.double(), dy[:n].double(), nbr[:n].numpy())
    m = torch.as_tensor(cnt, dtype=torch.float64).view(-1, 1, 1)
    lim = torch.minimum(torch.full_like(m, float(d)), (m - 1).clamp_min(0) + (0 if base is None else 1)) * U
    tot = ref if base is None else ref + base.double()
    amag = mag if base is None else mag + base.double().abs()
    got = dw.double().cpu()
    assert bool(torch.isfinite(got).all()), "a NaN of a row past the count or of an unreferenced row reached dw"
    err = (got - tot).abs()
    bad = int((err > lim * amag).sum())
    return float((err / amag.clamp_min(1e-300)).max()), float(lim.max()), bad, cnt


def injective_columns(nbr, n_rows, n_in, g, alive=None):
    """the pairs of `nbr` (rows below n_rows) with every column made injective: a real rulebook pairs an input row with at most
    one output row per offset, and the transposed table has one slot per (input row, offset)"""
    alive = torch.arange(n_in) if alive is None else alive
    assert alive.numel() >= n_rows
    for k in range(KK):
        rows = torch.nonzero(nbr[:n_rows, k] >= 0).view(-1)
        nbr[rows, k] = alive[torch.randperm(alive.numel(), generator=g)[:rows.numel()]].int()
    return nbr


@functools.lru_cache(maxsize=None)
def dgrad_case(cin, cout, n_in, kind="down", seed=0):
    """-> (dy [cap_out, cout], w [27, cin, cout], nbr [cap_out, 27] int32, n_out, cap_in).  "down": n_out < n_in rows, injective
    columns, the input rows i % 7 == 3 unreferenced.  "subm": a SYMMETRIC table (nbr[o][k] = i  <=>  nbr[i][26 - k] = o) with a full centre
    column, as a submanifold rulebook is -- the forward-table data gradient is defined for those.  dy rows past n_out are NaN."""
    g = torch.Generator().manual_seed(77 * cin + 3 * cout + n_in + seed)
    n_out = n_in if kind == "subm" else max(1, (3 * n_in) // 4)
    cap_out = n_out + 37
    nbr = _rand_rulebook(cap_out, n_in, "down", g, density=0.4)
    nbr[n_out:] = torch.where(nbr[n_out:] >= 0, torch.zeros_like(nbr[n_out:]), nbr[n_out:])
    injective_columns(nbr, n_out, n_in, g, None if kind == "subm" else torch.nonzero(torch.arange(n_in) % 7 != 3).view(-1))
    if kind == "subm":
        nbr[:n_out, 13] = torch.arange(n_out).int()
        nbr[n_out:, 13] = 0
        for k in range(13):
            nbr[:n_out, 26 - k] = -1
            o = torch.nonzero(nbr[:n_out, k] >= 0).view(-1)
            nbr[nbr[o, k].long(), 26 - k] = o.int()
    w = q12(torch.randn(KK, cin, cout, generator=g) / math.sqrt(8 * cin))
    dy = q12(torch.randn(cap_out, cout, generator=g))
    dy[n_out:] = float("nan")
    return dy, w, nbr, n_out, n_in + 50


def dgrad_ref(dy, nbr, w, n_out, n_in):
    """float64 data gradient on the transposed table -> (dx, sum |terms|, pairs per input row, the transposed table)"""
    t = transpose_table(nbr[:n_out].numpy().astype(np.int64), n_in)
    dx, mag = sparse_conv64(dy[:n_out].double(), t, w.double().transpose(1, 2).contiguous())
    return dx, mag, (t >= 0).sum(1), t


def dgrad_twin(dy, t, w):
    """fp32 twin on the transposed table t: offsets ascending, the channels of a product row left to right"""
    dy, w = dy.numpy(), w.numpy()
    dx = np.zeros((t.shape[0], w.shape[1]), np.float32)
    for k in range(KK):
        i = np.flatnonzero(t[:, k] >= 0)
        rows = dy[t[i, k]]
        for c in range(w.shape[2]):
            dx[i] = dx[i] + rows[:, c, None] * w[k, :, c][None]
    return torch.from_numpy(dx)


def dgrad_check(dx, ref, mag, pairs, c_dy):
    """-> (largest |err| / sum |terms|, largest bar, elements over their bar)"""
    m = torch.as_tensor(pairs * c_dy, dtype=torch.float64).view(-1, 1)
    d = torch.as_tensor(dgrad_depth(pairs, c_dy), dtype=torch.float64).view(-1, 1)
    lim = torch.minimum(d, (m - 1).clamp_min(0)) * U
    got = dx.double().cpu()
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    bad = int((err > lim * mag).sum())
    dead = torch.as_tensor(pairs == 0)
    assert int((got[dead] != 0).sum()) == 0, "an input row no output references has a gradient"
    return float((err / mag.clamp_min(1e-300)).max()), float(lim.max()), bad


# ---- B. BatchNorm + ReLU --------------------------------------------------------------------------------------------------------
Z_ULPS = 256.0
EPS_BN, MOMENTUM = float(np.float32(1e-3)), float(np.float32(0.01))      # as the kernels get them: fp32 arguments
BN1D_ROWS = {4: (1, 2, 3, 255, 256, 257, 513), 8: (1, 2, 127, 128, 129, 257, 8196), 16: (1, 2, 3, 63, 64, 65, 129, 513),
             32: (1, 2, 31, 33, 65, 8196), 64: (1, 2, 3, 15, 16, 17, 33, 513), 128: (1, 2, 7, 8, 9, 17, 8196),
             256: (1, 2, 3, 4, 5, 9, 513)}
BN1D_CAP = (70001, 256)                                            # past kBnMaxBlocks: 69 rows per block, 18 per thread
BN1D_CANCEL = (BN1D_CAP, (4099, 16))                               # (the capped case IS the first cancelling one)
CANCEL_1D = (3, 7, 9)                                              # mean 40 / std 0.1, mean -1000 / std 0.5, near-constant + outlier
BN2D_SHAPES = [(1, 1, 2, 2), (2, 3, 2, 6), (1, 5, 4, 17), (2, 300, 4, 8), (1, 1025, 4, 4), (1, 512, 132, 256)]
BN2D_REGIME = {(1, 1, 2, 2): (1, 4, 1), (2, 3, 2, 6): (3, 4, 1), (1, 5, 4, 17): (9, 8, 1), (2, 300, 4, 8): (4, 8, 1),
               (1, 1025, 4, 4): (1, 16, 1), (1, 512, 132, 256): (2, 16896, 17)}       # (S, chunk, float4 per thread)
CANCEL_2D = (3, 5)


def bn_ref(xc, gamma, beta, dyc, rm=None, rv=None, dt=np.float64, eps=EPS_BN, momentum=MOMENTUM):
    """xc, dyc [C, N] (channel-major), gamma / beta / rm / rv [C] -> dict of results and of the scales of the summed ones (numpy
    arrays of dtype dt).  Evaluated with torch's CPU tensors of that dtype (the large cases have 18 M elements): elementwise
    IEEE arithmetic, sums along the contiguous axis (cascaded, like numpy's pairwise ones)."""
    tdt = torch.float64 if dt == np.float64 else torch.float32
    as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(tdt)                # noqa: E731
    x, dy = as_t(xc), as_t(dyc)
    g, b = as_t(gamma)[:, None], as_t(beta)[:, None]
    n = x.shape[1]
    mean = x.sum(1, keepdim=True) / n
    s_mean = x.abs().sum(1) / n
    d = x - mean
    var = (d * d).sum(1, keepdim=True) / n
    invstd = 1.0 / torch.sqrt(var + eps)
    xh = d.mul_(invstd)
    z = xh * g + b
    dz = torch.where(z > 0, dy, torch.zeros((), dtype=tdt))
    dbeta = dz.sum(1, keepdim=True)
    s_dbeta = dz.abs().sum(1)
    t = dz * xh
    dgamma = t.sum(1, keepdim=True)
    s_dgamma = t.abs_().sum(1)
    dx = (dz - dbeta / n - xh * (dgamma / n)).mul_(g * invstd)
    out = dict(mean=mean[:, 0], var=var[:, 0], invstd=invstd[:, 0], z=z, y=torch.relu(z), dbeta=dbeta[:, 0], dgamma=dgamma[:, 0],
               dx=dx, s_mean=s_mean, s_var=var[:, 0] + eps, s_dbeta=s_dbeta, s_dgamma=s_dgamma)
    if rm is not None:
        unb = var[:, 0] * n / (n - 1) if n > 1 else var[:, 0]
        rm, rv = as_t(rm), as_t(rv)
        out.update(rmean=(1 - momentum) * rm + momentum * mean[:, 0], rvar=(1 - momentum) * rv + momentum * unb,
                   s_rmean=(1 - momentum) * rm.abs() + momentum * s_mean, s_rvar=(1 - momentum) * rv.abs() + momentum * unb)
    return {k: v.numpy() for k, v in out.items()}


def z_margin(xc, gamma, beta, eps=EPS_BN):
    """-> (z [C, N] float64, Z_MARGIN [C])"""
    x = np.asarray(xc, np.float64)
    mean = x.mean(1, keepdims=True)
    invstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(1, keepdims=True) + eps)
    g, b = np.asarray(gamma, np.float64)[:, None], np.asarray(beta, np.float64)[:, None]
    z = (x - mean) * invstd * g + b
    return z, Z_ULPS * U * (np.abs(x).max(1) * invstd[:, 0] * np.abs(g[:, 0]) + np.abs(b[:, 0]))


def _bn_case(c, n, cancel, seed, max_rounds=20):
    r = np.random.default_rng(seed)
    x = r.standard_normal((c, n), dtype=np.float32)
    x *= r.uniform(0.5, 2.0, (c, 1)).astype(np.float32)
    x += r.uniform(-1.0, 1.0, (c, 1)).astype(np.float32)
    if cancel:
        a, b_, k = cancel
        x[a] = 40.0 + 0.1 * r.standard_normal(n)
        x[b_] = -1e3 + 0.5 * r.standard_normal(n)
        x[k] = 0.2 + 1e-3 * r.standard_normal(n)
        x[k, 0] = 3.0
    gamma = (r.uniform(0.5, 1.5, c) * np.where(r.uniform(size=c) < 0.25, -1.0, 1.0)).astype(np.float32)
    beta = (r.uniform(0.05, 0.3, c) * np.where(r.uniform(size=c) < 0.5, -1.0, 1.0)).astype(np.float32)
    dy = r.standard_normal((c, n), dtype=np.float32)
    rm, rv = r.standard_normal(c).astype(np.float32), r.uniform(0.5, 1.5, c).astype(np.float32)
    g64, b64 = gamma.astype(np.float64), beta.astype(np.float64)
    rounds = 0
    while True:
        x64 = x.astype(np.float64)
        mean = x64.mean(1)
        x64 -= mean[:, None]
        s = g64 / np.sqrt((x64 * x64).mean(1) + EPS_BN)
        mar = Z_ULPS * U * (np.abs(x).max(1).astype(np.float64) * np.abs(s) + np.abs(b64))
        x64 *= s[:, None]
        x64 += b64[:, None]                                                       # = z
        ch, i = np.nonzero(np.abs(x64) < mar[:, None])
        if not len(ch):
            break
        rounds += 1
        assert rounds <= max_rounds and n > 1, "the margin loop does not converge"
        sign = np.where(x64[ch, i] >= 0, 1.0, -1.0)
        x[ch, i] = (mean[ch] + (sign * 4.0 * mar[ch] - b64[ch]) / s[ch]).astype(np.float32)
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv, rounds=rounds)


@functools.lru_cache(maxsize=None)
def bn1d_case(n, c, cancel=False):
    """channel-major arrays x, dy [c, n] (the kernels get the transposes), gamma, beta, rm, rv, and the rounds the margin took"""
    return _bn_case(c, n, CANCEL_1D if cancel else None, 31 * n + c + (7 if cancel else 0))


@functools.lru_cache(maxsize=None)
def bn2d_case(shape):
    b, c, h, w = shape
    cancel = (CANCEL_2D[0], CANCEL_2D[1], 7) if shape == BN2D_SHAPES[-1] else None
    return _bn_case(c, b * h * w, cancel, 17 * c + h * w + b)


def to_nchw(a, shape):
    b, c, h, w = shape
    return np.ascontiguousarray(a.reshape(c, b, h, w).transpose(1, 0, 2, 3))


def from_nchw(a):
    return np.ascontiguousarray(np.asarray(a).transpose(1, 0, 2, 3).reshape(a.shape[1], -1))


BN_FIELDS = (("y", None), ("mean", "s_mean"), ("var", "s_var"), ("rmean", "s_rmean"), ("rvar", "s_rvar"), ("dbeta", "s_dbeta"),
             ("dgamma", "s_dgamma"), ("dx", None))


def bn_figures(got, ref):
    """got: dict of arrays named as bn_ref names them (var = 1 / invstd^2 - the variance behind invstd, eps included) ->
    {field: figure}; the scale of y and dx is max |ref| (1 where the reference is all zero: then the value must be zero too)"""
    out = {}
    for name, sname in BN_FIELDS:
        if name not in got or name not in ref:
            continue
        if sname:
            out[name] = figure(got[name], np.asarray(ref[name], np.float64) + (EPS_BN if name == "var" else 0.0), ref[sname])
            continue
        r = torch.as_tensor(ref[name]).double()                   # (18 M elements in the large cases: torch's threads)
        scale = float(r.abs().max())
        err = float((torch.as_tensor(got[name]).double() - r).abs_().max())
        assert scale > 0 or err == 0, "a value with no terms is not exactly 0"
        out[name] = err / scale if scale > 0 else 0.0
    return out


def bn_twin_as_got(tw):
    """the twin's results in the form bn_figures takes the kernel's: its invstd rounded to fp32 like a saved one"""
    out = {k: np.asarray(tw[k], np.float64) for k, _ in BN_FIELDS if k in tw and k != "var"}
    out["var"] = 1.0 / np.asarray(tw["invstd"], np.float64) ** 2
    return out


# ---- C. dense weight gradient -------------------------------------------------------------------------------------------------
DENSE_SHAPES = [(1, 1, 1, 1, 1), (1, 3, 2, 1, 7), (2, 5, 6, 2, 1), (1, 3, 2, 3, 43), (1, 3, 2, 3, 44), (1, 3, 2, 3, 45),
                (1, 2, 3, 2, 89), (1, 65, 63, 5, 45), (1, 5, 6, 71, 3), (1, 3, 2, 130, 2), (3, 64, 64, 4, 46)]
DENSE_SHAPES_BF16 = [s for s in DENSE_SHAPES if s[4] % 2 == 0] + [(1, 3, 2, 3, 46), (1, 2, 3, 2, 90), (1, 65, 63, 5, 46)]
DENSE_ACCUMULATE = [(1, 65, 63, 5, 45), (1, 5, 6, 71, 3)]
DENSE_ACCUMULATE_BF16 = [(1, 65, 63, 5, 46), (1, 3, 2, 130, 2)]
# (nseg, columns of the last strip, nrange, rows_per, rows of the last range, cin tiles, cout tiles)
DENSE_REGIME = {(1, 1, 1, 1, 1): (1, 1, 1, 1, 1, 1, 1), (1, 3, 2, 1, 7): (1, 7, 1, 1, 1, 1, 1), (2, 5, 6, 2, 1): (1, 1, 2, 1, 1, 1, 1),
                (1, 3, 2, 3, 43): (1, 43, 3, 1, 1, 1, 1), (1, 3, 2, 3, 44): (1, 44, 3, 1, 1, 1, 1),
                (1, 3, 2, 3, 45): (2, 1, 3, 1, 1, 1, 1), (1, 2, 3, 2, 89): (3, 1, 2, 1, 1, 1, 1),
                (1, 65, 63, 5, 45): (2, 1, 5, 1, 1, 2, 1), (1, 5, 6, 71, 3): (1, 3, 36, 2, 1, 1, 1),
                (1, 3, 2, 130, 2): (1, 2, 44, 3, 1, 1, 1), (3, 64, 64, 4, 46): (2, 2, 4, 1, 1, 1, 1),
                (1, 3, 2, 3, 46): (2, 2, 3, 1, 1, 1, 1), (1, 2, 3, 2, 90): (3, 2, 2, 1, 1, 1, 1),
                (1, 65, 63, 5, 46): (2, 2, 5, 1, 1, 2, 1)}


def bf16r(t):
    return t.bfloat16().float()


@functools.lru_cache(maxsize=None)
def dense_case(shape, seed=0):
    """-> (x [B, Cin, H, W], dy [B, Cout, H, W]) fp32"""
    b, cin, cout, h, w = shape
    g = torch.Generator().manual_seed(sum(p * q for p, q in zip(shape, (1, 7, 13, 101, 1009))) + seed)
    return torch.randn(b, cin, h, w, generator=g), torch.randn(b, cout, h, w, generator=g)


def dense_twin(x, dy, ks):
    """the same autograd on fp32 CPU tensors"""
    w = torch.zeros(dy.shape[1], x.shape[1], ks, ks, dtype=torch.float32, requires_grad=True)
    F.conv2d(x.float(), w, None, 1, ks // 2).backward(dy.float())
    return w.grad


def dense_refs(x, dy, ks, base=None):
    """-> (float64 reference, per-element scale, fp32 twin), the base of `accumulate` added to all three"""
    ref, scale, twin = _wgrad_ref(x, dy, ks), _wgrad_ref(x.abs(), dy.abs(), ks), dense_twin(x, dy, ks)
    if base is not None:
        ref, scale, twin = ref + base.double(), scale + base.double().abs(), twin + base
    return ref, scale, twin


def dead_taps(h, w, ks):
    """taps (ky, kx) of a k x k kernel that reach no pixel of an h x w map"""
    if ks == 1:
        return []
    return [(ky, kx) for ky in range(3) for kx in range(3) if (h == 1 and ky != 1) or (w == 1 and kx != 1)]


def bn_affine_operand(x, aff):
    """relu(batchnorm(x)) as the loaders of sassd_conv2d_bwd_weight_bf16_bnrelu form it, from the affine triple [3, Cin] (mean |
    invstd * gamma | beta): z = fmaf(x - mean, scale, beta) in fp32 -- the difference rounded to fp32, product and sum rounded
    once (float64 holds the 48-bit product exactly) -- then the ReLU; the caller rounds to bf16"""
    a = aff.double().cpu()
    d = (x.float() - a[0].float().view(1, -1, 1, 1)).double()
    z = (d * a[1].view(1, -1, 1, 1) + a[2].view(1, -1, 1, 1)).float()
    return torch.relu(z)


def host_affine(x, gamma, beta, eps=EPS_BN):
    """the affine triple from float64 statistics, rounded to fp32 (for maps sassd_bn2d_stats does not take: H * W % 4 != 0)"""
    x64 = x.double()
    mean, var = x64.mean((0, 2, 3)), x64.var((0, 2, 3), unbiased=False)
    return torch.stack([mean, gamma.double() / torch.sqrt(var + eps), beta.double()]).float()
