"""BEV conv0 straight from the sparse tensor (include/sassd.h: sassd_wino4_sparse_prepare, sassd_conv2d_wino4_chain_sparse), the part
that needs no GPU: the symbols are declared, bound and exported, the size queries are host arithmetic, and every argument set the
entry points cannot run is refused with SASSD_EINVAL BEFORE any launch (the pointers below are made-up addresses: a launch on them
could not return an error code from a machine without a device, let alone the right one)."""
import ctypes as C
import os
import re

import sassd  # noqa: F401
from sassd import _C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOSPC = -1, -2
NEW = ("sassd_wino4_sparse_grid_ints", "sassd_wino4_sparse_prepare", "sassd_conv2d_wino4_chain_sparse")


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "sassd.h")).read()
    L = _C.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), "%s is not declared in include/sassd.h" % name
        assert name in _C.EXPORTS, "%s is not bound in _C.py" % name
        assert getattr(L, name) is not None
    # the entry it is measured against keeps its documented signature
    assert len(_C._SIGS["sassd_conv2d_wino4_chain"][1]) == 22


def test_size_queries():
    L = _C.lib()
    assert L.sassd_wino4_sparse_grid_ints(1, 5, 200, 176) == 5 * 200 * 176          # int32 [B][D][H][W]
    assert L.sassd_wino4_sparse_grid_ints(4, 8, 188, 188) == 4 * 8 * 188 * 188
    assert L.sassd_wino4_sparse_grid_ints(1, 9, 200, 176) == 0                        # D <= 8 is a documented precondition
    assert L.sassd_wino4_sparse_grid_ints(1, 0, 200, 176) == 0 and L.sassd_wino4_sparse_grid_ints(0, 5, 200, 176) == 0
    assert L.sassd_wino4_sparse_grid_ints(1, 5, 202, 176) == 0 and L.sassd_wino4_sparse_grid_ints(1, 5, 200, 178) == 0
    # the tile map: head + tpos[T] + tlist[T] + T flag bytes (16-byte pieces); no longer capped by one workgroup's LDS
    for b, h, w in ((1, 200, 176), (2, 8, 36), (1, 4, 4), (8, 400, 352)):
        t = b * (h // 4) * (w // 4)
        n = L.sassd_wino4_tile_map_ints(b, h, w)
        assert n >= 4 + 2 * t + (t + 3) // 4 and n % 4 == 0, (b, h, w, n)
    assert L.sassd_wino4_tile_map_ints(8, 400, 352) > 0                              # 70400 tiles (was refused above 65536)
    assert L.sassd_wino4_tile_map_ints(1, 202, 176) == 0


def test_refusals_come_before_any_launch():
    L = _C.lib()
    p = C.c_void_p(256)                      # an aligned made-up address
    odd = C.c_void_p(260)                    # 4-byte aligned only
    big = 1 << 40

    def chain(feats=p, c=64, d=5, grid=p, w=p, y=p, batch=1, cin=320, cout=256, cmax=320, h=200, wd=176, tmap=p, ws=p,
              wsb=big):
        return L.sassd_conv2d_wino4_chain_sparse(feats, c, d, grid, w, None, None, 1, y, batch, cin, cout, cmax, h, wd, tmap, 0,
                                                 ws, wsb, None)
    assert chain(cin=256, cmax=256) == EINVAL                 # C * D != Cin
    assert chain(c=12, d=4, cin=48, cmax=256) == EINVAL       # Cin % 32 != 0
    assert chain(c=32, d=9, cin=288) == EINVAL                # D > 8
    assert chain(c=66, d=16, cin=1056, cmax=1056) == EINVAL   # (D > 8 and C % 4 != 0)
    assert chain(tmap=None) == EINVAL                         # no tile map
    assert chain(grid=None) == EINVAL and chain(feats=None) == EINVAL and chain(w=None) == EINVAL and chain(ws=None) == EINVAL
    for name in ("feats", "grid", "w", "y", "tmap", "ws"):    # misaligned pointers
        assert chain(**{name: odd}) == EINVAL, name
    assert chain(cout=128) == EINVAL and chain(h=202) == EINVAL and chain(cmax=256) == EINVAL      # shapes the GEMM refuses
    assert chain(batch=0) == EINVAL
    # the same arguments in order pass every check and stop at the workspace size -- still without a launch
    assert chain(wsb=1024) == ENOSPC
    assert chain(y=None, wsb=1024) == ENOSPC                  # y is optional (products stay for the next chain call)

    def prepare(idx=p, n=p, cap=100, batch=1, d=5, h=200, w=176, grid=p, tmap=p):
        return L.sassd_wino4_sparse_prepare(idx, n, cap, batch, d, h, w, grid, tmap, None)
    assert prepare(idx=None) == EINVAL and prepare(n=None) == EINVAL and prepare(grid=None) == EINVAL
    assert prepare(tmap=None) == EINVAL and prepare(cap=0) == EINVAL
    assert prepare(d=9) == EINVAL and prepare(d=0) == EINVAL and prepare(h=202) == EINVAL and prepare(batch=0) == EINVAL
    assert prepare(grid=odd) == EINVAL and prepare(tmap=odd) == EINVAL and prepare(idx=odd) == EINVAL
    assert L.sassd_wino4_tile_map(None, p, 100, 1, 200, 176, p, None) == EINVAL
    assert L.sassd_wino4_tile_map(p, p, 100, 1, 200, 176, odd, None) == EINVAL
