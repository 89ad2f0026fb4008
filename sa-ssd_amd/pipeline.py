"""Device-resident whole-frame inference plan: raw points (or reference-style voxel inputs) -> detections.

This is the production path of the drop-in: the same kernels the per-op facades call, chained on ONE HIP stream
with every data-dependent size kept in device memory, so a frame is a fixed launch sequence with zero host syncs
between the first kernel and the final result read-back (the reference path has >= 6 syncs per sample,
SURVEY.md 3.1).  Eval-mode BatchNorm is folded into per-channel (scale, shift) applied in the conv epilogues.

Stages / reference lines:
  voxelize + mean      points_ops.py:104-164, vxnet.py:110-116          sassd_voxelize
  rulebooks x7         cmn.py:147-173 (spconv get_indice_pairs)         sassd_hash_build / rulebook_subm / rulebook_conv
  sparse convs x14     cmn.py:192-231 (+BN1d+ReLU)                      sassd_spconv_fwd
  dense()              cmn.py:112-114                                   sassd_densify (d-major channels, conv0 permuted); the
                                                                        default fp32 plan builds no dense map: BEV conv0 gathers
                                                                        the sparse rows (sassd_conv2d_wino4_chain_sparse)
  BEVNet x8            cmn.py:233-282                                   sassd_conv2d_fwd (fp32 MFMA)
  SSD head (fused 1x1) ssd_rotate_head.py:218-235                       sassd_conv2d_fwd
  anchors_mask         kitti.py:333-343                                 sassd_anchor_mask
  guided anchors       ssd_rotate_head.py:307-372                       sassd_decode_filter
  PSWarp               ssd_rotate_head.py:416-447                       sassd_conv2d_fwd x2 + sassd_pswarp_sample; the default fp32
                                                                        plan runs the two convs at the sampled pixels only
                                                                        (sassd_ps_pixel_list + sassd_ps_head_sampled)
  rescore + NMS        ssd_rotate_head.py:487-533                       sassd_rescore_nms

precision="bf16" runs every dense conv (densify, BEVNet x8, the fused head, both part-sensitive convs) on bf16 operands with
fp32 accumulation: sassd_densify_bf16, sassd_conv2d_bf16_infer_fwd (3x3), sassd_conv1x1_bf16_infer_fwd (1x1).  The weights are
the raw conv weights rounded once at construction (BatchNorm is not folded into them: it is applied in fp32 to the
accumulator, relu(acc * scale + shift)), and the maps between two dense convs are stored as bf16 -- rounding at the store is
the rounding the consumer would apply at its load.  Everything else (voxelizer, rulebooks, sparse convs, anchor mask, decode,
PSWarp sampling, rescore / NMS) and the head / part-sensitive outputs it reads stay fp32.

sparse_precision="bf16" (independent of `precision`) runs the 14 sparse convs on bf16 features: sassd_spconv_fwd_bf16 with weights
from sassd_spconv_bf16_pack_weight.  The first layer (Cin -> 16, voxel means in metres) keeps fp32 operands and stores bf16; every
other layer reads bf16 features and raw weights rounded once to bf16, accumulates in fp32, applies relu(acc * scale + shift) in
fp32 and stores bf16.  The feature ping-pong buffers (and `middle`) hold bf16; densify copies the level-3 features unchanged into
the bf16 map, or widens them exactly into the fp32 one (sassd_densify_from_bf16).  Voxels, rulebooks and anchor masks are those of
the fp32 plan.
"""
import numpy as np

import torch

from . import kernels as K
from . import anchors as A
from .stream import CALIB_DOUBLES, stage_layout
from .fuse import check_fuse_iou
from .tta import MAX_POOL, check_views

BN_EPS = 1e-3

# (state-dict prefix under neck.backbone, bn prefix, kind, Cin, Cout, rulebook key) -- VxNet, cmn.py:197-212
VXNET = [
    ("conv0.0", "conv0.1", "subm", 4, 16, "subm0"), ("conv0.3", "conv0.4", "subm", 16, 16, "subm0"),
    ("down0.0", "down0.1", "down", 16, 32, "down0"),
    ("conv1.0", "conv1.1", "subm", 32, 32, "subm1"), ("conv1.3", "conv1.4", "subm", 32, 32, "subm1"),
    ("down1.0", "down1.1", "down", 32, 64, "down1"),
    ("conv2.0", "conv2.1", "subm", 64, 64, "subm2"), ("conv2.3", "conv2.4", "subm", 64, 64, "subm2"),
    ("conv2.6", "conv2.7", "subm", 64, 64, "subm2"),
    ("down2.0", "down2.1", "down", 64, 64, "down2"),
    ("conv3.0", "conv3.1", "subm", 64, 64, "subm3"), ("conv3.3", "conv3.4", "subm", 64, 64, "subm3"),
    ("conv3.6", "conv3.7", "subm", 64, 64, "subm3"),
    ("extra_conv.0", "extra_conv.1", "1x1", 64, 64, None),
]


INPUT_WEIGHT_KEY = "neck.backbone.conv0.0.weight"


def input_features_of(state_dict):
    """Features per voxel the detector reads: Cin of the input layer's weight [3, 3, 3, Cin, 16] (neck.num_input_features /
    backbone.num_input_features of the config that built it).  ValueError for a missing or malformed weight and for a width
    outside 3..8 (the sparse input-layer kernels, include/sassd.h "Sparse input layer")."""
    w = state_dict.get(INPUT_WEIGHT_KEY)
    if w is None:
        raise ValueError("state dict has no %s" % INPUT_WEIGHT_KEY)
    shape = tuple(int(s) for s in w.shape)
    if len(shape) != 5 or shape[:3] != (3, 3, 3) or shape[4] != 16:
        raise ValueError("%s has shape %s, expected [3, 3, 3, Cin, 16]" % (INPUT_WEIGHT_KEY, list(shape)))
    if not 3 <= shape[3] <= 8:
        raise ValueError("%s reads %d features per voxel; 3 to 8 are supported" % (INPUT_WEIGHT_KEY, shape[3]))
    return shape[3]


def fold_bn(sd, prefix, eps=BN_EPS):
    g, b = sd[prefix + ".weight"].float(), sd[prefix + ".bias"].float()
    m, v = sd[prefix + ".running_mean"].float(), sd[prefix + ".running_var"].float()
    scale = g / torch.sqrt(v + eps)
    return scale.contiguous(), (b - m * scale).contiguous()


def _bev_weight(sd, i, D3):
    w = sd["neck.fcn.conv%d.weight" % i].float()
    if i == 0:      # densify writes d-major channels (d*C + c); reference order is c*D + d (cmn.py:113-114)
        cout, cin = w.shape[:2]
        c = cin // D3
        w = w.view(cout, c, D3, 3, 3).permute(0, 2, 1, 3, 4).reshape(cout, cin, 3, 3)
    return w.contiguous()


class InferencePlan:
    """Pre-packed weights + pre-allocated buffers for a fixed (batch_size, config)."""

    def __init__(self, state_dict, *, batch_size=1, num_class=1, voxel_size=(0.05, 0.05, 0.1),
                 point_cloud_range=(0, -40., -3., 70.4, 40., 1.), max_num_points=5, max_voxels=20000,
                 sparse_shape=(40, 1600, 1408), anchors=None, anchors_bv=None, anchor_area_threshold=1,
                 anchors_per_loc=2, grid_offsets=(0., 40.), featmap_stride=0.4, rpn_thr=0.1, score_thr=0.3,
                 iou_thr=0.1, cap_k=4096, cap_d=512, device=None, level_cap_factor=2, overlap=True, winograd=True,
                 fused_rulebooks=True, chain_bev=True, pyramid_persistent=False, spconv_cfg=None, wino4_cfg=None,
                 skip_inactive_tiles=True, rb_sync_levels=(0, 1, 2, 3), ps_tail=False, precision="fp32",
                 sparse_precision="fp32", dense_entry=False, ps_sampled=True, tta=None,
                 fuse_iou=None):
        """precision: "fp32" (default) or "bf16" (module docstring).  In bf16 mode the fp32 kernel-selection knobs
        (winograd, chain_bev, wino4_cfg, ps_tail, skip_inactive_tiles) are ignored, and a shape the bf16 kernels do not
        support raises ValueError here (there is no fp32 fall-back).
        sparse_precision: "fp32" (default) or "bf16" -- the 14 sparse convs on bf16 features (module docstring), independent
        of `precision`; spconv_cfg selects among the fp32 sparse kernels only.
        dense_entry: False (default) -- in the fp32 / fp32-sparse plan whose conv0 runs on a tile map, conv0's Winograd input
        transform gathers the level-3 rows through a pixel -> row index grid (sassd_conv2d_wino4_chain_sparse): no dense map is
        cleared, scattered into and read back, bit-identical.  True: the dense map of every other mode (A/B, tests).
        ps_sampled: True (default) -- a precision="fp32" plan (whatever its sparse_precision) computes the part-sensitive head
        only at the pixels PSWarp samples: post() lists them from the frame's candidates (sassd_ps_pixel_list) and runs both
        part-sensitive convs there (sassd_ps_head_sampled), bit-identical to the dense kernels at every pixel that is read, so
        logits and detections are unchanged.  `ps_t` then materialises the dense maps on read.  False: the two dense launches
        in bev_and_heads (A/B, tests).  Ignored (dense) with precision="bf16", with ps_tail=True and for head shapes the
        sampled kernel does not take.
        tta: None (default) or a test-time augmentation spec, a list of 1..8 views (flip, angle, scale) whose first is the
        identity (sassd.tta; include/sassd.h "Test-time augmentation").  The plan then takes `batch_size` clouds per frame and
        returns `batch_size` result sets as before -- `b_user`, the outer batch: det, results(), the frame record, the
        annotations and the staging block are sized for it -- while everything from the voxelizer to PSWarp runs on the INNER
        batch `B` = b_user * V, inner sample s * V + v being view v of cloud s.  sassd_tta_views_dev writes the clouds of the
        views in front of the voxelizer, sassd_tta_pool gathers the candidates of a cloud's views, back in the sensor frame,
        into `pool` ([b_user, capP = min(V * capK, 4096)] rows) behind PSWarp, and the unchanged rescore / NMS runs on the
        pool: the views are suppressed together.  A cloud whose views yield more than capP candidates sets
        SASSD_ST_BOX_OVERFLOW.  The views are fixed here, for the life of the plan.  ValueError for a malformed spec and for
        an inner batch the sparse index space cannot hold, before anything is allocated.
        fuse_iou: None (default: every path makes the calls it made before) or a number inside (0, 1) (sassd.fuse;
        include/sassd.h "Box fusion").  post() then launches sassd_box_fuse behind rescore / NMS, one kernel: every detection
        becomes the score-weighted mean of the candidates of its label -- of `pool` under tta, of `df` otherwise -- whose
        rotated BEV IoU with it is at least fuse_iou.  The fused boxes are `fused` [b_user, capD, 7]; `out` is what leaves the
        plan -- `det` with those boxes, scores / labels / counts shared -- and what results(), the frame record and the
        annotations read, and what run_* return.  `det` keeps the unfused boxes for inspection.  ValueError for a value outside
        (0, 1)."""
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' or 'bf16', got %r" % (precision,))
        if sparse_precision not in ("fp32", "bf16"):
            raise ValueError("sparse_precision must be 'fp32' or 'bf16', got %r" % (sparse_precision,))
        self.precision, self.bf16 = precision, precision == "bf16"
        self.sparse_precision, self.sparse_bf16 = sparse_precision, sparse_precision == "bf16"
        # b_user: the clouds per frame and the result sets per frame (the outer batch).  B: the samples the detector runs
        # on (the inner batch), b_user * V under test-time augmentation and b_user otherwise
        self.tta = None if tta is None else check_views(tta)
        self.fuse_iou = check_fuse_iou(fuse_iou)
        self.V = 1 if self.tta is None else len(self.tta)
        self.b_user = int(batch_size)
        if self.tta is not None:
            cells = float(np.prod([float(v) for v in sparse_shape])) * self.b_user * self.V
            if self.b_user < 1 or cells >= 4294967294.0:        # lin_fits of csrc/rulebook.hip: linear voxel indices are 32-bit
                raise ValueError("tta: %d views of %d clouds are an inner batch of %d samples, which a sparse shape of %s "
                                 "cannot index" % (self.V, self.b_user, self.b_user * self.V, tuple(sparse_shape)))
        dev = torch.device(device if device is not None else "cuda:0")
        self.dev, self.B, self.ncls, self.A = dev, self.b_user * self.V, int(num_class), int(anchors_per_loc)
        self.voxel_size = np.asarray(voxel_size, np.float32)
        self.pc_range = np.asarray(point_cloud_range, np.float32)
        self.T, self.max_voxels = int(max_num_points), int(max_voxels)
        self.shape0 = tuple(int(s) for s in sparse_shape)
        self.rpn_thr, self.score_thr, self.iou_thr = float(rpn_thr), float(score_thr), float(iou_thr)
        self.grid_offsets, self.spatial_scale = grid_offsets, 1.0 / featmap_stride
        self.area_thr = anchor_area_threshold
        self.capK, self.capD = int(cap_k), int(cap_d)
        self.cin = input_features_of(state_dict)            # features per voxel: 4 for KITTI, 3..8 supported
        sd = {k: v.detach().to(dev) for k, v in state_dict.items()}

        # ---- level geometry / capacities ----------------------------------------------------------
        self.shapes = [self.shape0]
        for _ in range(3):
            self.shapes.append(K.conv_out_shape(self.shapes[-1]))
        cap0 = self.B * self.max_voxels
        self.caps = [cap0] + [cap0 * level_cap_factor] * 3
        D3, self.H, self.W = self.shapes[3]
        self.D3 = D3

        # ---- sparse weights -----------------------------------------------------------------------
        self.sp = []
        lvl = 0
        for li, (wname, bnname, kind, cin, cout, key) in enumerate(VXNET):
            if li == 0:
                cin = self.cin                              # the input layer: the table row names the KITTI width
            w = sd["neck.backbone.%s.weight" % wname].float()
            k = 1 if kind == "1x1" else 27
            lvl += kind == "down"
            if self.sparse_bf16:
                # the raw weights rounded once to bf16 (the first layer keeps fp32 operands); BatchNorm stays in the epilogue
                if not K.spconv_bf16_supported(k, cin, cout, self.caps[lvl]):
                    raise ValueError("sparse_precision='bf16': %s (%s, %d -> %d) at a capacity of %d rows is not supported by "
                                     "the bf16 sparse-conv kernels" % (wname, kind, cin, cout, self.caps[lvl]))
                wp = K.spconv_bf16_pack_weight(w.reshape(k, cin, cout).contiguous())
            else:
                wp = K.spconv_pack_weight(w.reshape(k, cin, cout).contiguous())
            scale, shift = fold_bn(sd, "neck.backbone.%s" % bnname)
            self.sp.append((kind, cin, cout, key, wp, scale, shift))
        if self.sparse_bf16 and not K.densify_bf16_supported(64, self.shapes[3]):
            raise ValueError("sparse_precision='bf16': the dense map (64 x %d channels) on a %dx%d BEV map is not supported by "
                             "the bf16 densify" % (D3, self.H, self.W))

        # ---- dense weights ------------------------------------------------------------------------
        hw = torch.cat([sd["rpn_head.conv_box.weight"], sd["rpn_head.conv_cls.weight"],
                        sd["rpn_head.conv_dir_cls.weight"]], 0).float().contiguous()
        hb = torch.cat([sd["rpn_head.conv_box.bias"], sd["rpn_head.conv_cls.bias"],
                        sd["rpn_head.conv_dir_cls.bias"]], 0).float().contiguous()
        self.n_box = sd["rpn_head.conv_box.weight"].shape[0]
        self.n_cls = sd["rpn_head.conv_cls.weight"].shape[0]
        self.n_dir = sd["rpn_head.conv_dir_cls.weight"].shape[0]
        self.head_c = hw.shape[0]
        self.head_b = hb
        w0 = sd["extra_head.convs.0.weight"].float().contiguous()
        self.ps_parts = w0.shape[0]
        self.ps_s0, self.ps_b0 = fold_bn(sd, "extra_head.convs.1")
        w1 = sd["extra_head.convs.3.weight"].float().contiguous()
        if self.bf16:
            self._dense_weights_bf16(sd, hw, w0, w1)
        else:
            self._dense_weights_fp32(sd, hw, w0, w1, winograd, chain_bev, wino4_cfg, ps_tail, ps_sampled)

        # ---- anchors --------------------------------------------------------------------------------
        self.Atot = self.ncls * self.H * self.W * self.A
        if anchors is not None:
            an = np.asarray(anchors, np.float32).reshape(-1, 7)
            assert an.shape[0] == self.Atot, (an.shape, self.Atot)
            self.anchors = torch.from_numpy(np.ascontiguousarray(an)).to(dev)
            bv = anchors_bv if anchors_bv is not None else A.rbbox2d_to_near_bbox(an[:, [0, 1, 3, 4, 6]])
            self.anchors_bv = torch.from_numpy(np.ascontiguousarray(bv, np.float32)).to(dev)
        else:
            self.anchors = self.anchors_bv = None

        # ---- buffers --------------------------------------------------------------------------------
        B, H, W = self.B, self.H, self.W
        i32, f32 = torch.int32, torch.float32
        z = lambda *s, dt=f32: torch.zeros(*s, dtype=dt, device=dev)       # noqa: E731
        self.status = z(1, dt=i32)
        self.row_off = z(B + 1, dt=i32)
        self.vnum = z(B, dt=i32)
        self.n = [self.row_off[B:B + 1]] + [z(1, dt=i32) for _ in range(3)]       # device row counts per level
        self.idx = [z(c, 4, dt=i32) for c in self.caps]
        self.tables = [K.HashTable(c, dev) for c in self.caps]
        self.nbr = {key: z(self.caps[lvl], 27, dt=i32)
                    for key, lvl in (("subm0", 0), ("down0", 1), ("subm1", 1), ("down1", 2), ("subm2", 2),
                                     ("down2", 3), ("subm3", 3))}
        fdt = torch.bfloat16 if self.sparse_bf16 else f32   # sparse feature ping-pong (sparse bf16 mode: rounded at the store)
        self.feat = [z(max(self.caps), 64, dt=fdt), z(max(self.caps), 64, dt=fdt)]
        self.mean = z(self.caps[0], self.cin)               # per-voxel means, row stride Cin (the voxelizer's nfeat)
        mdt = torch.bfloat16 if self.bf16 else f32          # maps read by a dense conv (bf16 mode: rounded at the store)
        self._dense_shape, self._dense_dt = (B, 64 * D3, H, W), mdt
        self._dense = None                                  # the [B, 64 D, H, W] map: allocated by the plans that densify
        self.act = [z(B, 256, H, W, dt=mdt) for _ in range(3)]
        self.head_out = z(B, self.head_c, H, W)
        # the part-sensitive maps (3x3 output, 1x1 output).  A sampled plan writes the second at the listed pixels only and
        # never builds the first: `ps_t` materialises both from conv6 on read, into buffers of its own
        self._ps_t = [None if self.ps_sampled else z(B, self.ps_parts, H, W, dt=mdt), z(B, self.ps_parts, H, W)]
        self._ps_dense = None
        self.ps_list = K.ps_pixel_list_buffer(B, H, W, dev) if self.ps_sampled else None
        self.conv6 = None
        self.mask = z(B, self.Atot, dt=torch.uint8)
        self.df = dict(guided=z(B, self.capK, 7), labels=z(B, self.capK, dt=i32), scores=z(B, self.capK),
                       counts=z(B, dt=i32))
        self.logits = z(B, self.capK)
        # test-time augmentation: the candidates of a cloud's views, pooled for one rescore / NMS per cloud
        self.capP, self.pool, bu = None, None, self.b_user
        if self.tta is not None:
            self.capP = min(self.V * self.capK, MAX_POOL)
            self.pool = dict(guided=z(bu, self.capP, 7), logits=z(bu, self.capP), labels=z(bu, self.capP, dt=i32),
                             counts=z(bu, dt=i32))
        self.det = dict(boxes=z(bu, self.capD, 7), scores=z(bu, self.capD), labels=z(bu, self.capD, dt=i32),
                        counts=z(bu, dt=i32))
        # box fusion: the boxes that leave the plan are a buffer of their own; without it `out` IS `det`
        self.fused, self.out = None, self.det
        if self.fuse_iou is not None:
            self.fused = z(bu, self.capD, 7)
            self.out = dict(self.det, boxes=self.fused)
        self.middle = {}
        # all seven rulebooks through the fused pyramid (1 fill + 8 launches); the per-op chain (30) stays selectable for A/B
        self.pyr = None
        if fused_rulebooks:
            self.pyr = K.RulebookPyramid(self.idx, self.n, self.caps, self.shape0, B,
                                         [self.nbr["subm%d" % l] for l in range(4)],
                                         [None] + [self.nbr["down%d" % l] for l in range(3)], self.status)
        # True: the whole pyramid as ONE persistent launch (in-launch grid barriers) instead of two launches per level
        self.pyramid_persistent = bool(pyramid_persistent)
        # per-call kernel-selection words of the C ABI (None: the binding's default, 0 in production)
        self.spconv_cfg, self.wino4_cfg = spconv_cfg, wino4_cfg
        self.graph = None
        self.record = None         # device frame record: capture(seal=True)
        self.raw_cap = None        # capture(raw_cap=...): the frame crops raw sweeps
        self.sw_ring = None        # capture(sweeps=...): the frame merges sweeps from this device ring
        self._stage_block = None   # capture(): the frame's small inputs in one device block (sassd.stream.stage_layout)
        self._wsid = id(self)
        # coordinate-only work (rulebooks, anchors_mask) runs on a side stream, overlapping the feature path
        self.overlap = bool(overlap)
        self.side = torch.cuda.Stream(device=dev) if self.overlap else None
        self.rb_ev = {k: torch.cuda.Event() for k in self.nbr}
        self.mask_ev = torch.cuda.Event()
        # BEV conv0 reads the densified sparse map: its Winograd launch runs on the tiles that have an occupied pixel in their
        # 6x6 patch only (56 % on a KITTI frame; bit-identical, the others' products are exactly zero).  The map is built from
        # the level-3 coordinates on the side stream.
        self.tile_map = None
        if skip_inactive_tiles and not self.bf16 and self.bev[0][5] == 4:
            n_ints = K._C.lib().sassd_wino4_tile_map_ints(B, H, W)
            if n_ints:
                self.tile_map = z(n_ints, dt=i32)
        self.tmap_ev = torch.cuda.Event()
        # conv0 straight from the sparse rows (class docstring: dense_entry): needs the tile map; the bf16 modes, keep_middle and
        # anything that reads `self.dense` stay on (or materialise) the dense map
        self.sparse_grid = None
        if not dense_entry and self.tile_map is not None and not self.sparse_bf16 and not self.chain[0]:
            self.sparse_grid = K.wino4_sparse_grid(B, D3, H, W, dev)
        self.sparse_entry = self.sparse_grid is not None
        self._sparse_frame = False                          # the current frame took the sparse entry
        self._tmap_joined = False
        if not self.sparse_entry:
            self._dense_map()
        self.rb_sync_levels = tuple(sorted(int(l) for l in rb_sync_levels))   # levels whose completion the main stream waits
        assert self.rb_sync_levels and self.rb_sync_levels[-1] == 3           # for ((0, 1, 2, 3): one wait per level)
        self.prof = None           # set to {} to collect (name, start_event, end_event) tuples per frame
        self.prof_sparse_layers = False     # with prof: also one segment per sparse conv (sparse_conv0..13)

    def _dense_weights_fp32(self, sd, hw, w0, w1, winograd, chain_bev, wino4_cfg, ps_tail, ps_sampled):
        """precision="fp32": BEVNet on Winograd / fp32-MFMA kernels with BatchNorm folded into the epilogues, the heads on the
        narrow / direct fp32 kernels."""
        D3, dev = self.D3, self.dev
        self.bev = []
        for i in range(8):
            w = _bev_weight(sd, i, D3)
            scale, shift = fold_bn(sd, "neck.fcn.bn%d" % i)
            # 3x3 layers: Winograd F(4x4,3x3) (transform + 36 MFMA GEMMs + transform: 4x fewer multiplications) when the
            # shape allows, else the fused F(2x2,3x3) kernel (2.25x fewer), else the direct kernel.  `winograd` = 2
            # forces F(2x2), 0 / False the direct kernel (A/B)
            wino = 0
            if winograd and w.shape[2] == 3:
                if winograd != 2 and K.conv2d_wino4_supported(w.shape[1], w.shape[0], self.H, self.W):
                    wino = 4
                elif K.conv2d_wino_supported(w.shape[1], w.shape[0], self.H, self.W):
                    wino = 2
            if w.shape[2] == 1 and winograd and K.conv1x1_gemm_supported(w.shape[1], w.shape[0], self.H, self.W):
                wino = 1                             # 1x1 layer (conv7): the same MFMA GEMM kernel, one problem per image
            wp = (K.conv2d_wino4_pack_weight(w.contiguous()) if wino == 4 else
                  K.conv2d_wino_pack_weight(w.contiguous()) if wino == 2 else
                  K.conv1x1_gemm_pack_weight(w.contiguous()) if wino == 1 else K.conv2d_pack_weight(w.contiguous()))
            self.bev.append((wp, w.shape[0], w.shape[2], scale, shift, wino))
        self.wino4_ws = None
        # consecutive F(4x4) layers are chained: the map between two of them stays in the transform domain (fused output
        # -> input transform, sassd_conv2d_wino4_chain); `chain_bev=False` keeps three launches per layer (A/B)
        self.bev_cin = [int(sd["neck.fcn.conv%d.weight" % i].shape[1]) for i in range(8)]
        self.chain = [False] * 8                         # chain[i]: layer i reads the products layer i-1 left behind
        if any(l[5] == 4 for l in self.bev):
            self.cmax = max(max(self.bev_cin[i], self.bev[i][1]) for i in range(8) if self.bev[i][5] == 4)
            self.wino4_ws = K.conv2d_wino4_chain_workspace(self.B, self.cmax, self.H, self.W, dev)
            for i in range(1, 8):
                # (equal Cout on both sides of a boundary: the two layers then pad their tile count to one plane stride)
                self.chain[i] = bool(chain_bev and self.bev[i][5] == 4 and self.bev[i - 1][5] == 4 and i - 1 != 6 and
                                     self.bev[i - 1][1] == self.bev_cin[i] and self.bev[i - 1][1] == self.bev[i][1] and
                                     K.conv2d_wino4_chain_supported(self.bev_cin[i], self.bev[i][1], self.H, self.W))
        # 1x1 convs with <= 32 output channels (the single-class fused head, the second part-sensitive conv) stream on the
        # vector ALU (sassd_conv1x1_narrow_fwd); wider ones (three-class head: 60 maps) stay on the MFMA kernel
        self.head_narrow = K.conv1x1_narrow_supported(hw.shape[1], hw.shape[0])
        self.head_w = K.conv1x1_narrow_pack_weight(hw) if self.head_narrow else K.conv2d_pack_weight(hw)
        self.ps_w0 = K.conv2d_pack_weight(w0)
        # the part-sensitive 3x3 conv (256 -> 28) as a narrow TAIL of the Winograd chain on conv6's products (fused transform +
        # 64-channel GEMM block + output transform; conv6's own NCHW map is stored by the fused transform): when conv6 is a
        # chained F(4x4) layer with the default GEMM geometry.  OPT-IN (ps_tail=True): measured in round 6 at 205 us for conv6 +
        # tail against 143 + 77 us for conv6 + the direct fp32-MFMA conv -- 15 us per frame, 0.3 % of the frame rate, for 5 x the
        # direct kernel's error on the part-sensitive features (1.5e-5 vs 2.9e-6): not the default
        self.ps_tail = bool(ps_tail and chain_bev and self.bev[6][5] == 4 and self.chain[6] and self.ps_parts <= 64 and
                            w0.shape[2] == 3 and w0.shape[1] == self.bev[6][1] and not ((wino4_cfg or 0) & 0xff))
        self.ps_w0t = K.conv2d_wino4_pack_weight_narrow(w0) if self.ps_tail else None
        self.ps_narrow = K.conv1x1_narrow_supported(w1.shape[1], w1.shape[0])
        self.ps_w1 = K.conv1x1_narrow_pack_weight(w1) if self.ps_narrow else K.conv2d_pack_weight(w1)
        # the head at the sampled pixels only (class docstring: ps_sampled): repeats the direct 3x3 kernel and the narrow 1x1
        self.ps_sampled = bool(ps_sampled and not self.ps_tail and self.ps_narrow and w0.shape[2] == 3 and
                               self.ps_parts == 28 and K.ps_head_sampled_supported(w0.shape[1], self.ps_parts))

    def _dense_weights_bf16(self, sd, hw, w0, w1):
        """precision="bf16": the raw weights of every dense conv rounded once into bf16 packs (BatchNorm stays out of them),
        after checking that the bf16 inference kernels take every shape of the frame."""
        H, W = self.H, self.W

        def need(ok, what):
            if not ok:
                raise ValueError("precision='bf16': %s on a %dx%d BEV map is not supported by the bf16 inference kernels"
                                 % (what, H, W))
        need(K.densify_bf16_supported(64, self.shapes[3]), "the dense map (64 x %d channels)" % self.D3)
        self.bev, self.chain, self.wino4_ws, self.ps_tail, self.ps_w0t = [], [False] * 8, None, False, None
        self.head_narrow = self.ps_narrow = self.ps_sampled = False
        self.bev_cin = [int(sd["neck.fcn.conv%d.weight" % i].shape[1]) for i in range(8)]
        self.bev16 = []
        for i in range(8):
            w = _bev_weight(sd, i, self.D3)
            cout, cin, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
            if k == 3:
                need(K.conv2d_bf16_infer_supported(cin, cout, H, W), "BEV conv%d (3x3, %d -> %d)" % (i, cin, cout))
                wp = K.conv2d_bf16_infer_pack_weight(w)
            else:
                need(k == 1 and K.conv1x1_bf16_infer_supported(cin, cout, H * W),
                     "BEV conv%d (%dx%d, %d -> %d)" % (i, k, k, cin, cout))
                wp = K.conv1x1_bf16_pack_weight(w)
            scale, shift = fold_bn(sd, "neck.fcn.bn%d" % i)
            self.bev16.append((wp, cout, k, scale, shift))
        need(K.conv1x1_bf16_infer_supported(hw.shape[1], hw.shape[0], H * W), "the fused SSD head (%d -> %d)" % (hw.shape[1], hw.shape[0]))
        self.head_w = K.conv1x1_bf16_pack_weight(hw)
        need(w0.shape[2] == 3 and K.conv2d_bf16_infer_supported(w0.shape[1], w0.shape[0], H, W),
             "the part-sensitive conv (%d -> %d)" % (w0.shape[1], w0.shape[0]))
        self.ps_w0 = K.conv2d_bf16_infer_pack_weight(w0)
        need(K.conv1x1_bf16_infer_supported(w1.shape[1], w1.shape[0], H * W), "the part-sensitive 1x1 (%d -> %d)" % (w1.shape[1], w1.shape[0]))
        self.ps_w1 = K.conv1x1_bf16_pack_weight(w1)

    def _dense_map(self):
        if self._dense is None:
            self._dense = torch.zeros(*self._dense_shape, dtype=self._dense_dt, device=self.dev)
        return self._dense

    @property
    def ps_t(self):
        """The part-sensitive maps [3x3 output, 1x1 output] of the current frame, whole.  A sampled plan holds the second at
        the listed pixels only: a read runs the two dense convs on the conv6 map the frame left behind, into buffers of its
        own (inspection, tests) -- the frame path never pays for it."""
        if not self.ps_sampled:
            return self._ps_t
        if self._ps_dense is None:
            self._ps_dense = [torch.zeros(self.B, self.ps_parts, self.H, self.W, device=self.dev) for _ in range(2)]
        if self.conv6 is not None:
            K.conv2d_fwd(self.conv6, self.ps_w0, self.ps_parts, 3, self.ps_s0, self.ps_b0, True, self._ps_dense[0])
            K.conv1x1_narrow_fwd(self._ps_dense[0], self.ps_w1, self.ps_parts, None, None, False, self._ps_dense[1])
        return self._ps_dense

    @property
    def dense(self):
        """The densified level-3 map [B, 64 D, H, W] of the current frame.  A plan on the sparse entry does not build it on the
        frame path: a read materialises it from the frame's level-3 rows (inspection, tests, per-kernel timing)."""
        if self._sparse_frame:
            K.densify(self.sp_out, self.idx[3], self.n[3], self.caps[3], self.shapes[3], self.B, 1, self._dense_map())
        return self._dense_map()

    def _ev(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()                 # current stream == the stream every sassd kernel is launched on
        return e

    def _seg(self, name, e0):
        if self.prof is not None:
            self.prof.setdefault(name, []).append((e0, self._ev()))

    # ------------------------------------------------------------------------------------------------
    def voxelize(self, clouds, n_dev=None):
        """clouds: list of B device tensors [Ni, ndim] f32.  Fills idx[0] (b,z,y,x), mean, row_off.  With `n_dev`
        (device int32 [B], or a list of B one-word tensors) the clouds are capacity-sized staging buffers holding n_dev[b]
        points each."""
        assert len(clouds) == self.B
        for pts in clouds:
            if pts.shape[1] < self.cin:
                raise ValueError("the plan reads %d features per point, a cloud has %d columns" % (self.cin, pts.shape[1]))
        e0 = self._ev() if self.prof is not None else None
        self.row_off.fill_(0)                   # (a fill KERNEL: torch's zero_() is a memset, i.e. a memset node in a captured frame)
        for b, pts in enumerate(clouds):
            K.voxelize(pts, self.voxel_size, self.pc_range, self.T, self.max_voxels, batch_idx=b, coors_cols=4,
                       want_voxels=False, want_mean=True, nfeat=self.cin,
                       out=dict(coors=self.idx[0], mean=self.mean, voxel_num=self.vnum[b:b + 1],
                                num_points=self._numpts()),
                       row_offset=self.row_off[b:b + 2], status=self.status, cap=self.caps[0],
                       n_dev=None if n_dev is None else n_dev[b] if isinstance(n_dev, (list, tuple)) else n_dev[b:b + 1])
        self._seg("voxelize", e0)

    def _numpts(self):
        if not hasattr(self, "_np"):
            self._np = torch.zeros(self.caps[0], dtype=torch.int32, device=self.dev)
        return self._np

    def load_voxels(self, voxel_feats, coors4):
        """Reference-style inputs (single_stage.py:110-117): mean features [M,Cin] and coords [M,4] (b,z,y,x)."""
        if self.tta is not None:
            raise RuntimeError("a plan with tta transforms point clouds: it has no voxel entry (run_from_points, capture)")
        m = voxel_feats.shape[0]
        if voxel_feats.dim() != 2 or voxel_feats.shape[1] != self.cin:
            raise ValueError("the plan reads %d features per voxel, got features of shape %s"
                             % (self.cin, list(voxel_feats.shape)))
        assert m <= self.caps[0]
        self.mean[:m].copy_(voxel_feats)
        self.idx[0][:m].copy_(coors4.int())
        self.row_off.fill_(0)
        bc = torch.bincount(coors4[:, 0].long(), minlength=self.B).cumsum(0).int()
        self.row_off[1:].copy_(bc)

    def rulebooks(self):
        """All 7 rulebooks + 3 next-level hash tables.  They depend only on voxel COORDINATES, so they are issued on
        a side HIP stream and overlap the feature path; `self.rb_ev[key]` fires when a rulebook is ready."""
        B = self.B
        if self.pyr is not None:
            if self.pyramid_persistent:
                self.pyr.build(persistent=True)
                for ev in self.rb_ev.values():
                    ev.record()
                return
            for lvl in range(4):
                self._rulebook_level(lvl)
            return
        self.tables[0].build(self.idx[0], self.n[0], self.shapes[0], B, self.status)
        for lvl in range(4):
            K.rulebook_subm(self.idx[lvl], self.n[lvl], self.caps[lvl], self.shapes[lvl], B, self.tables[lvl],
                            self.nbr["subm%d" % lvl])
            self.rb_ev["subm%d" % lvl].record()
            if lvl < 3:
                K.rulebook_conv(self.idx[lvl], self.n[lvl], self.caps[lvl], self.shapes[lvl], B, self.tables[lvl],
                                self.caps[lvl + 1], self.idx[lvl + 1], self.n[lvl + 1], self.nbr["down%d" % lvl],
                                self.status)
                self.rb_ev["down%d" % lvl].record()
                self.tables[lvl + 1].build(self.idx[lvl + 1], self.n[lvl + 1], self.shapes[lvl + 1], B, self.status)

    def _rulebook_level(self, lvl):
        """level `lvl` of the fused pyramid on the CURRENT stream: the level's submanifold table (`subm<lvl>`) and, for lvl > 0,
        the strided table into it (`down<lvl-1>`) + its coordinates; fires their events."""
        self.pyr.build(lvl, lvl + 1)                    # level 0: clears + hash; l >= 1: ordered emit of level l; tables
        self.rb_ev["subm%d" % lvl].record()
        if lvl > 0:
            self.rb_ev["down%d" % (lvl - 1)].record()

    def backbone(self, keep_middle=False, anchors_mask=None, densify=True, masks=True, rulebooks=True, convs=True):
        """7 rulebooks + 14 sparse convs (+ densify).  Two streams: coordinate-only work (rulebook pyramid, anchors_mask) on the
        side stream, features on the main stream, which waits for each rulebook event once.  (Round 5 measured the alternative
        issue order -- pyramid level l+1 issued behind the first conv of level l, so that a conv never waits for more of the
        pyramid than it needs: 703 against 748 frames/s and 0.365 against 0.347 ms for the segment's graph on one box,
        profiles/r05_pyramid_issue_order.txt.  The pyramid in front it is.)"""
        main = torch.cuda.current_stream(self.dev)
        e0 = self._ev() if self.prof is not None else None
        sparse = self.sparse_entry and densify and not keep_middle
        self._sparse_frame, self._tmap_joined = sparse, False
        if self.overlap:
            self.side.wait_stream(main)                 # voxel coordinates are ready
            with torch.cuda.stream(self.side):
                if rulebooks:
                    self.rulebooks()
                if self.tile_map is not None and densify:
                    self._tile_map(sparse)
                    self.tmap_ev.record()
                if masks:
                    self.anchor_masks(anchors_mask)     # also coordinate-only work
                self.mask_ev.record()
        else:
            if rulebooks:
                self.rulebooks()
            if self.tile_map is not None and densify and not sparse:
                self._tile_map(False)
        if not convs:                                   # (measurement: the rulebook pyramid alone)
            return
        x = self.mean
        lvl = 0
        cur = 0
        # cross-stream waits: the main stream joins the side stream at `rb_sync_levels` -- a wait on level L's event covers
        # every level <= L (stream order).  Round 6 measured one wait per level (the default) against two (after levels 1 and
        # 3) and one (after level 3): sparse segment 0.320 / 0.332 / 0.334 ms, frames/s equal -- fewer graph edges do not pay
        # for the later start of the first convs (profiles/r06_pyramid_forms.txt).
        covered = -1
        for li, (kind, cin, cout, key, wp, scale, shift) in enumerate(self.sp):
            y = self.feat[cur]
            if kind == "down":
                lvl += 1
            if key is not None and self.overlap and rulebooks and lvl > covered:
                upto = min([l for l in self.rb_sync_levels if l >= lvl] or [3])
                main.wait_event(self.rb_ev["subm%d" % upto])
                covered = upto
            el = self._ev() if self.prof is not None and self.prof_sparse_layers else None
            if self.sparse_bf16:
                K.spconv_fwd_bf16(x, None if key is None else self.nbr[key], self.n[lvl], self.caps[lvl], wp,
                                  1 if key is None else 27, cin, cout, scale, shift, True, y)
            elif kind == "subm" or kind == "down":
                K.spconv_fwd(x, self.nbr[key], self.n[lvl], self.caps[lvl], wp, 27, cin, cout, scale, shift, True, y,
                             cfg=self.spconv_cfg)
            else:
                K.spconv_fwd(x, None, self.n[lvl], self.caps[lvl], wp, 1, cin, cout, scale, shift, True, y, cfg=self.spconv_cfg)
            if el is not None:
                self._seg("sparse_conv%d" % li, el)
            if keep_middle:
                self.middle[li] = (y.clone(), lvl, cout)
            x = y
            cur ^= 1
        self.sp_out = x
        self._seg("sparse", e0)
        if not densify:
            return
        e1 = self._ev() if self.prof is not None else None
        if sparse:
            # no dense map: conv0 gathers the rows itself.  What is left of this stage is the index grid (+ tile map): built
            # from the coordinates on the side stream, joined here -- or built here, on a plan without a side stream
            if self.overlap:
                main.wait_event(self.tmap_ev)
                self._tmap_joined = True
            else:
                self._tile_map(True)
        elif self.sparse_bf16:          # the bf16 features unchanged: copied into a bf16 map, widened exactly into an fp32 one
            K.densify_from_bf16(x, self.idx[3], self.n[3], self.caps[3], self.shapes[3], self.B, 1, self._dense_map(),
                                  out_bf16=self.bf16)
        elif self.bf16:
            K.densify_bf16(x, self.idx[3], self.n[3], self.caps[3], self.shapes[3], self.B, 1, self._dense_map())
        else:
            K.densify(x, self.idx[3], self.n[3], self.caps[3], self.shapes[3], self.B, 1, self._dense_map())
        self._seg("densify", e1)

    def _tile_map(self, sparse):
        """conv0's active-tile map from the level-3 coordinates; `sparse`: with the index grid of the sparse entry."""
        if sparse:
            K.wino4_sparse_prepare(self.idx[3], self.n[3], self.caps[3], self.B, self.D3, self.H, self.W, self.sparse_grid,
                                   self.tile_map)
        else:
            K.wino4_tile_map(self.idx[3], self.n[3], self.caps[3], self.B, self.H, self.W, out=self.tile_map)

    def bev_and_heads(self):
        if self.bf16:
            return self._bev_and_heads_bf16()
        x = None if self._sparse_frame else self._dense_map()
        for i, (wp, cout, ks, scale, shift, wino) in enumerate(self.bev):
            y = self.act[i % 2] if i < 7 else self.act[2]
            e0 = self._ev() if self.prof is not None else None
            if wino == 4:
                # layer i hands its products to layer i+1 (no NCHW map in between) unless its output is needed: conv6
                # feeds the part-sensitive head, the last F(4x4) layer feeds a 1x1 / direct layer
                keep = (i + 1 < 8 and self.chain[i + 1]) or (i == 6 and self.ps_tail)
                prev = self.bev[i - 1][3:5] + (True,) if self.chain[i] else None
                tmap = self.tile_map if i == 0 else None                     # conv0: the active tiles of the sparse map only
                ptmap = self.tile_map if (i == 1 and self.chain[1]) else None   # conv1 reads conv0's compacted products
                if tmap is not None and self.overlap and not self._tmap_joined:
                    torch.cuda.current_stream(self.dev).wait_event(self.tmap_ev)
                if i == 0 and self._sparse_frame:
                    K.conv2d_wino4_chain_sparse(self.sp_out, self.D3, self.sparse_grid, wp, self.bev_cin[0], cout, self.cmax,
                                                self.B, self.H, self.W, scale, shift, True, None if keep else y, self.wino4_ws,
                                                tmap, cfg=self.wino4_cfg)
                else:
                    K.conv2d_wino4_chain(None if self.chain[i] else x, prev, wp, self.bev_cin[i], cout, self.cmax, self.B,
                                         self.H, self.W, scale, shift, True, None if keep else y, self.wino4_ws,
                                         cfg=self.wino4_cfg, tile_map=tmap, prev_tile_map=ptmap)
            elif wino == 2:
                K.conv2d_wino_fwd(x, wp, cout, scale, shift, True, y)
            elif wino == 1:
                K.conv1x1_gemm_fwd(x, wp, cout, scale, shift, True, y, cfg=self.wino4_cfg)
            else:
                K.conv2d_fwd(x, wp, cout, ks, scale, shift, True, y)
            if i == 6 and self.ps_tail:
                # conv6's products stay in the workspace: the tail call stores conv6's activation map (for conv7) and runs the
                # part-sensitive 3x3 conv on them
                K.conv2d_wino4_chain_tail(self.bev[6][3:5] + (True,), y, self.ps_w0t, cout, self.ps_parts, self.cmax, self.B,
                                          self.H, self.W, self.ps_s0, self.ps_b0, True, self._ps_t[0], self.wino4_ws,
                                          cfg=self.wino4_cfg)
            self._seg("bev_conv%d" % i, e0)
            x = y
            if i == 6:
                self.conv6 = y
        self.x = x
        e0 = self._ev() if self.prof is not None else None
        if self.head_narrow:
            K.conv1x1_narrow_fwd(x, self.head_w, self.head_c, None, self.head_b, False, self.head_out)
        else:
            K.conv2d_fwd(x, self.head_w, self.head_c, 1, None, self.head_b, False, self.head_out)
        if self.ps_sampled:             # post() runs both part-sensitive convs, at the pixels the candidates sample
            self._seg("heads", e0)
            return
        if not self.ps_tail:
            K.conv2d_fwd(self.conv6, self.ps_w0, self.ps_parts, 3, self.ps_s0, self.ps_b0, True, self._ps_t[0])
        if self.ps_narrow:
            K.conv1x1_narrow_fwd(self._ps_t[0], self.ps_w1, self.ps_parts, None, None, False, self._ps_t[1])
        else:
            K.conv2d_fwd(self._ps_t[0], self.ps_w1, self.ps_parts, 1, None, None, False, self._ps_t[1])
        self._seg("heads", e0)

    def _bev_and_heads_bf16(self):
        x = self._dense_map()
        for i, (wp, cout, ks, scale, shift) in enumerate(self.bev16):
            y = self.act[i % 2] if i < 7 else self.act[2]
            e0 = self._ev() if self.prof is not None else None
            if ks == 3:
                K.conv2d_bf16_infer_fwd(x, wp, cout, scale, shift, True, y)
            else:
                K.conv1x1_bf16_infer_fwd(x, wp, cout, scale, shift, True, y)
            self._seg("bev_conv%d" % i, e0)
            x = y
            if i == 6:
                self.conv6 = y
        self.x = x
        e0 = self._ev() if self.prof is not None else None
        K.conv1x1_bf16_infer_fwd(x, self.head_w, self.head_c, None, self.head_b, False, self.head_out, out_bf16=False)
        K.conv2d_bf16_infer_fwd(self.conv6, self.ps_w0, self.ps_parts, self.ps_s0, self.ps_b0, True, self._ps_t[0])
        K.conv1x1_bf16_infer_fwd(self._ps_t[0], self.ps_w1, self.ps_parts, None, None, False, self._ps_t[1], out_bf16=False)
        self._seg("heads", e0)

    def anchor_masks(self, masks=None):
        if masks is not None:
            self.mask.copy_(masks.view(self.B, -1).to(torch.uint8))
            return
        H0, W0 = self.shape0[1], self.shape0[2]
        K.anchor_mask_batch(self.idx[0], self.row_off, self.B, H0, W0, self.anchors_bv, self.voxel_size, self.pc_range,
                            self.area_thr, self.mask)

    def post(self):
        e0 = self._ev() if self.prof is not None else None
        HW = self.H * self.W
        ho = self.head_out
        base = ho.view(-1)
        box = base
        cls = base[self.n_box * HW:]
        dirp = base[(self.n_box + self.n_cls) * HW:]
        K.decode_filter(box, cls, dirp, self.head_c * HW, self.B, self.ncls, self.A, self.H, self.W, self.anchors,
                        self.mask, self.rpn_thr, self.capK, self.df, self.status)
        if self.ps_sampled:
            K.ps_pixel_list(self.df["guided"], self.df["counts"], self.capK, self.B, self.H, self.W, self.grid_offsets,
                            self.spatial_scale, out=self.ps_list)
            K.ps_head_sampled(self.conv6, self.ps_w0, self.ps_s0, self.ps_b0, True, self.ps_w1, None, None, False,
                              self.ps_list, self._ps_t[1])
        K.pswarp_sample(self._ps_t[1], self.df["guided"], self.df["counts"], self.capK, self.grid_offsets,
                        self.spatial_scale, self.logits)
        cand, logits = self.df, self.logits
        if self.tta is not None:        # the views of a cloud as one candidate list in the sensor frame: pooled NMS
            cand = K.tta_pool(self.df["guided"], self.logits, self.df["labels"], self.df["counts"], self.tta, self.capP,
                              out=self.pool, status=self.status)
            logits = cand["logits"]
        K.rescore_nms(cand["guided"], logits, cand["labels"], cand["counts"], self.score_thr,
                      self.iou_thr, self.capD, self.det, self.status)
        if self.fuse_iou is not None:   # the candidates NMS dropped move the box that stood for them
            K.box_fuse(cand["guided"], logits, cand["labels"], cand["counts"], self.score_thr, self.fuse_iou, self.det,
                       out=self.fused)
        self._seg("post", e0)

    def sparse_work(self):
        """Algorithmic work of the sparse path for the CURRENT frame (SURVEY.md 8d formulas): per layer
        B_gs = 4P(Cin+Cout) + 8P + 4K*Cin*Cout + 4*Nout*Cout, B_min, flops = 2*P*Cin*Cout; rulebook bytes."""
        n = [int(t.item()) for t in self.n]
        pairs = {}
        lvl_of = dict(subm0=0, down0=1, subm1=1, down1=2, subm2=2, down2=3, subm3=3)
        for key, t in self.nbr.items():
            pairs[key] = int((t[:n[lvl_of[key]]] >= 0).sum().item())
        bgs = bmin = flops = rb = 0
        lvl = 0
        seen = set()
        for kind, cin, cout, key, *_ in self.sp:
            if kind == "down":
                nin, lvl = n[lvl], lvl + 1
            else:
                nin = n[lvl]
            nout = n[lvl]
            p = pairs[key] if key else nout
            k = 27 if key else 1
            bgs += 4 * p * (cin + cout) + 8 * p + 4 * k * cin * cout + 4 * nout * cout
            bmin += 4 * nin * cin + 4 * nout * cout + 4 * k * cin * cout + 8 * p
            flops += 2 * p * cin * cout
            if key and key not in seen:
                seen.add(key)
                rb += (16 * nin + 8 * p) if kind == "subm" else (16 * nin + 16 * nout + 8 * p)
        return dict(n=n, pairs=pairs, bytes_gs=bgs, bytes_min=bmin, flops=flops, rulebook_bytes=rb)

    # ------------------------------------------------------------------------------------------------
    def _tail(self, anchors_mask):
        self.bev_and_heads()
        if self.overlap:
            torch.cuda.current_stream(self.dev).wait_event(self.mask_ev)
        else:
            self.anchor_masks(anchors_mask)
        self.post()
        return self.out

    def _view_clouds(self, clouds):
        """The inner batch of an eager frame: every cloud followed by its views 1 .. V-1 (sassd_tta_views_dev)."""
        if self.tta is None:
            return clouds
        if len(clouds) != self.b_user:
            raise ValueError("a batch of %d clouds for a plan of batch_size %d" % (len(clouds), self.b_user))
        inner = []
        for pts in clouds:
            views = [torch.empty_like(pts) for _ in range(self.V - 1)]
            if self.V > 1 and pts.shape[0]:
                n = torch.full((self.V,), int(pts.shape[0]), dtype=torch.int32, device=self.dev)
                K.tta_views(pts, n[0:1], self.tta, views, [n[v:v + 1] for v in range(1, self.V)])
            inner += [pts] + views
        return inner

    def run_from_points(self, clouds, anchors_mask=None):
        """One frame batch, raw device point clouds in -> device detection buffers out (no host sync)."""
        with K.ws_scope(self._wsid):
            self.voxelize(self._view_clouds(clouds))
            self.backbone(anchors_mask=anchors_mask)
            return self._tail(anchors_mask)

    def run_from_voxels(self, voxel_feats, coors4, anchors_mask=None):
        with K.ws_scope(self._wsid):
            self.load_voxels(voxel_feats, coors4)
            self.backbone(anchors_mask=anchors_mask)
            return self._tail(anchors_mask)

    # ---- hipGraph: the whole frame as ONE launch ---------------------------------------------------------
    def capture(self, points_cap, ndim=4, stages=("voxelize", "backbone", "tail"), seal=False, raw_cap=None, annos=False,
                sweeps=None):
        """Capture the frame (raw points -> detections, side stream included) into a hipGraph.  Input staging:
        `self.pts_in[b]` [points_cap, ndim] f32 and `self.npts` int32 [B]; `run_graph(clouds)` fills them and replays.
        `stages` lets a caller capture a sub-range (e.g. only the sparse backbone for a roofline measurement).
        Staging: the frame's small inputs -- crop planes, calibration, seq, counts -- are views into ONE device block,
        `self._stage_block` (uint8), cut by sassd.stream.stage_layout(B, raw_cap is not None, annos, seal), so that they
        travel in one copy (sassd.stream.FrameStream).
        seal=True: the frame's last node is sassd_frame_seal -- `self.record` (device uint8) then holds the frame record of
        include/sassd.h after every replay, its `seq` word echoed from the device word `self._seq`.
        The launch sequence that was captured stays on the plan as `_frame_fn`, for inspection only (a test captures it once
        more into a plain hipGraph to count its node types); nothing on the frame path calls it.
        raw_cap: the frame starts at a raw sweep.  Its input is `self.raw_in[b]` [raw_cap, ndim] f32, `self.nraw` int32 [B] and
        `self.crop_planes` [B,6,4] f64 (`self.crop_f32_math`, a host flag read at capture, says how they are evaluated:
        False, the float64 test of geometry.frustum_planes); its first nodes are one sassd_crop_polytope_dev per sample
        (two kernels each), which write `pts_in[b]` and `npts[b]` for the unchanged voxelizer.  A sweep that keeps more than
        points_cap points sets SASSD_ST_POINT_OVERFLOW.  The block's counts are then `nraw`; `npts` is a tensor of its own.
        annos=True (needs seal=True): the frame's tail is sassd_frame_seal_kitti -- the record is layout version 2, the
        KITTI annotation block of include/sassd.h behind the version 1 record.  Its input is `self.calib` [B,36] f64
        (Tr_velo_to_cam 12, R0_rect 9, P2 12, img_w, img_h, one pad per sample).
        sweeps=dict(ring=<[B,R,sweep_cap,ndim_in] f32 device, shared by the plans of a stream>, S=, sweep_cap=, time_feature=):
        the frame's cloud is merged from the ring (include/sassd.h "Multi-sweep merge").  `ndim` is the width of the MERGED
        cloud, ndim_in + (1 if time_feature else 0), and the width check above applies to it.  The descriptors -- `self.sw_slot`,
        `sw_count`, `sw_xform` [B,S] i32, `sw_T` [B,S,3,4] f64, `sw_dt` [B,S] f32 -- are views into the staging block; the
        frame's first nodes are one sassd_merge_sweeps_dev per sample (one kernel each), which write `pts_in[b]` and `npts[b]`
        for the unchanged voxelizer.  A merged cloud above points_cap sets SASSD_ST_POINT_OVERFLOW.  `npts` is a tensor of its
        own; the block's counts are not read by the frame.  Excludes raw_cap.
        A plan with tta (class docstring) is fed exactly like one without: `pts_in`, `npts`, `raw_in`, the ring, the staging
        block and the record are those of its b_user clouds.  Behind the crop / merge nodes and in front of the voxelizer the
        frame holds one sassd_tta_views_dev per cloud, which writes `pts_views[b][v - 1]` and `npts_views[b, v - 1]` from
        `pts_in[b]` and `npts[b]`; the voxelizer reads all B clouds."""
        dev = self.dev
        S, self.sw_ring = 0, None
        if sweeps is not None:
            if raw_cap is not None:
                raise ValueError("sweeps and raw_cap exclude each other: merged clouds are not cropped")
            ring, S, tf = sweeps["ring"], int(sweeps["S"]), bool(sweeps["time_feature"])
            if "voxelize" not in stages or not 1 <= S <= 16:
                raise ValueError("sweeps needs 1..16 entries and the voxelize stage")
            if (ring.dim() != 4 or ring.shape[0] != self.b_user or ring.shape[2] != int(sweeps["sweep_cap"])
                    or ring.dtype != torch.float32 or not ring.is_cuda or not ring.is_contiguous()):
                raise ValueError("sweeps: the ring must be a contiguous [B, R, sweep_cap, ndim_in] float32 device tensor")
            ndim_out = ring.shape[3] + (1 if tf else 0)
            if int(ndim) != ndim_out:
                raise ValueError("sweeps: the merged cloud has %d columns, capture(ndim=%d)" % (ndim_out, int(ndim)))
        if int(ndim) < self.cin:
            raise ValueError("the plan reads %d features per point: capture(ndim=%d) is too narrow" % (self.cin, int(ndim)))
        if annos and not seal:
            raise ValueError("annos=True writes the annotation block into the frame record: it needs seal=True")
        self.pts_cap = int(points_cap)
        self.raw_cap = None if raw_cap is None else int(raw_cap)
        if self.raw_cap is not None and (self.raw_cap < 1 or "voxelize" not in stages):
            raise ValueError("raw_cap must be >= 1 and needs the voxelize stage")
        bu, V = self.b_user, self.V
        self.pts_in = [torch.zeros(self.pts_cap, ndim, dtype=torch.float32, device=dev) for _ in range(bu)]
        L = stage_layout(bu, self.raw_cap is not None, annos, seal, **(dict(sweeps=S) if S else {}))
        block = self._stage_block = torch.zeros(L["total"], dtype=torch.uint8, device=dev)
        counts = block[L["counts"]:L["counts"] + 4 * bu].view(torch.int32)
        if seal:
            self._seq = block[L["seq"]:L["counts"]].view(torch.int32)
        if annos:
            self.calib = block[L["calib"]:L.get("sweep_T", L["words"])].view(torch.float64).view(bu, CALIB_DOUBLES)
        if self.raw_cap is not None:
            self.raw_in = [torch.zeros(self.raw_cap, ndim, dtype=torch.float32, device=dev) for _ in range(bu)]
            self.crop_planes = block[L["planes"]:L["calib"]].view(torch.float64).view(bu, 6, 4)
            self.crop_f32_math = False
            self.nraw = counts
            self.npts = torch.zeros(bu, dtype=torch.int32, device=dev)      # written by the crop, read by the voxelizer
        elif S:
            self.sw_ring, self.sw_time = ring, tf
            self.sw_T = block[L["sweep_T"]:L["words"]].view(torch.float64).view(bu, S, 3, 4)
            self.sw_slot, self.sw_count, self.sw_xform = (
                block[L[k]:L[k] + 4 * bu * S].view(torch.int32).view(bu, S)
                for k in ("sweep_slot", "sweep_count", "sweep_xform"))
            self.sw_dt = block[L["sweep_dt"]:L["total"]].view(torch.float32).view(bu, S)
            self.sw_slot.fill_(-1)                  # until the first descriptors arrive, every entry is absent
            self.npts = torch.zeros(bu, dtype=torch.int32, device=dev)      # written by the merge, read by the voxelizer
        else:
            self.npts = counts
        if annos:
            self.record = torch.zeros(K.frame_record_kitti_bytes(bu, self.capD), dtype=torch.uint8, device=dev)
        elif seal:
            self.record = torch.zeros(K.frame_record_bytes(bu, self.capD), dtype=torch.uint8, device=dev)
        # test-time augmentation: `pts_in` / `npts` stay the clouds the caller (or the crop, or the merge) fills -- the identity
        # views; the other views have staging of their own, written inside the frame, and the voxelizer reads all B of them
        self.pts_views = [[torch.zeros(self.pts_cap, ndim, dtype=torch.float32, device=dev) for _ in range(V - 1)]
                          for _ in range(bu)]
        self.npts_views = torch.zeros(bu, V - 1, dtype=torch.int32, device=dev) if V > 1 else None
        pts_inner = [t for b in range(bu) for t in [self.pts_in[b]] + self.pts_views[b]]
        npts_inner = [t for b in range(bu) for t in [self.npts[b:b + 1]] + [self.npts_views[b, v:v + 1] for v in range(V - 1)]]
        assert self.prof is None, "per-stage event timing and graph capture exclude each other"

        def frame():
            with K.ws_scope(self._wsid):
                if self.raw_cap is not None:
                    for b in range(bu):
                        K.crop_polytope(self.raw_in[b], self.nraw[b:b + 1], self.crop_planes[b], self.crop_f32_math,
                                        self.pts_in[b], self.npts[b:b + 1], self.status)
                if S:
                    for b in range(bu):
                        K.merge_sweeps(self.sw_ring[b], self.sw_slot[b], self.sw_count[b], self.sw_xform[b], self.sw_T[b],
                                       self.sw_dt[b], self.sw_time, self.pts_in[b], self.npts[b:b + 1], self.status)
                if V > 1 and "voxelize" in stages:
                    for b in range(bu):
                        K.tta_views(self.pts_in[b], self.npts[b:b + 1], self.tta, self.pts_views[b], npts_inner[b * V + 1:(b + 1) * V])
                if "voxelize" in stages:
                    self.voxelize(pts_inner, n_dev=self.npts if self.tta is None else npts_inner)
                if "backbone" in stages:
                    self.backbone()
                elif "sparse" in stages:              # rulebooks + the 14 sparse convs only (roofline measurement)
                    self.backbone(densify=False, masks=False)
                elif "sparse_convs" in stages:        # the 14 sparse convs on the rulebooks of the previous pass (floor model)
                    self.backbone(densify=False, masks=False, rulebooks=False)
                elif "pyramid" in stages:             # the rulebook pyramid alone
                    self.backbone(densify=False, masks=False, convs=False)
                if "tail" in stages:
                    self._tail(None)
                elif self.overlap:
                    torch.cuda.current_stream(self.dev).wait_event(self.mask_ev)      # join the side stream
                if annos:
                    K.frame_seal_kitti(self.out, self._seq, self.status, self.calib, self.record)
                elif seal:
                    K.frame_seal(self.out, self._seq, self.status, self.record)

        # capture needs a non-default stream (the legacy null stream cannot be captured)
        cap = torch.cuda.Stream(device=dev)
        cap.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(cap):
            frame()                               # warm-up: every workspace / lazily created event exists
            cap.synchronize()
            self.graph = K.Graph().capture(frame)
        self._frame_fn = frame                     # the captured launch sequence (tools / tests capture it again to inspect it)
        # the graph holds raw pointers into this plan's grow-only kernel workspaces: keep the tensors it was captured
        # with alive, so that a later eager call that regrows a workspace cannot free memory the graph still replays on
        self._graph_ws = K.scoped_workspaces(self._wsid)
        torch.cuda.current_stream(dev).wait_stream(cap)
        return self.graph

    def stage_inputs(self, clouds):
        if self.raw_cap is not None:
            raise RuntimeError("a plan captured with raw_cap is fed through raw_in / nraw / crop_planes (sassd.stream.FrameStream)")
        if self.sw_ring is not None:
            raise RuntimeError("a plan captured with sweeps is fed through its ring and descriptors (sassd.stream.FrameStream)")
        for b, pts in enumerate(clouds or ()):
            n = pts.shape[0]
            if n > self.pts_cap:            # never detect on a silently truncated cloud
                raise ValueError("cloud %d has %d points, the captured graph was sized for %d (plan.capture(points_cap))"
                                 % (b, n, self.pts_cap))
            self.pts_in[b][:n].copy_(pts, non_blocking=True)
            self.npts[b:b + 1].fill_(n)

    def run_graph(self, clouds=None):
        """Replay the captured frame (after staging `clouds`, unless the caller filled pts_in / npts itself)."""
        if clouds is not None:
            self.stage_inputs(clouds)
        self.graph.launch()
        return self.out

    def results(self):
        """The only host sync of a frame: D2H of the (small) detection buffers, like
        ssd_rotate_head.py:529-531.  Returns per-sample (boxes[k,7], scores[k], labels[k]) numpy or None."""
        counts = self.out["counts"].cpu().numpy()
        st = int(self.status.item())
        if st:
            raise RuntimeError("sassd pipeline status flags 0x%x (capacity overflow / hash full)" % st)
        out = []
        for b in range(self.b_user):
            k = int(counts[b])
            if k == 0:
                out.append((None, None, None))
                continue
            out.append((self.out["boxes"][b, :k].cpu().numpy(), self.out["scores"][b, :k].cpu().numpy(),
                        self.out["labels"][b, :k].cpu().numpy().astype(np.int64)))
        return out
