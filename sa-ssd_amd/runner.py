"""The loops around the hot path: `train_one_epoch` / `train_model` (tools/train_utils/__init__.py:36-118) and
`single_test` + KITTI evaluation (tools/test.py:19-99,131-158) -- library functions, not a CLI.

One process per GPU.  Training: every rank iterates its DistributedGroupSampler share (sassd.loader), gradients meet in
ONE all-reduce over the flat buffer per step (sassd.train.GradSync), rank 0 logs and writes checkpoints.  Testing: the
reference walks the val split serially on one GPU; here `single_test` takes this rank's round-robin share of the frames
(no data-path collective) and the per-frame result annotations are gathered on the host in dataset order."""
import glob
import os
from collections import deque

import torch

from . import dist as D
from . import kitti_common as kitti
from . import train as T
from .loader import FrameLoader


def train_one_epoch(model, optimizer, train_loader, lr_scheduler, sync, accumulated_iter, train_epoch, rank=0,
                    logger=None, log_interval=20, lr_warmup_scheduler=None):
    """-> accumulated_iter after the epoch.  Loss terms are kept on the device and only read every `log_interval`
    iterations (the reference calls .item() on every term of every iteration, train_utils/__init__.py:8-25)."""
    if hasattr(train_loader, 'sampler') and hasattr(train_loader.sampler, 'set_epoch'):
        train_loader.sampler.set_epoch(train_epoch - 1)
    window = []
    for i, batch in enumerate(train_loader):
        warm = lr_warmup_scheduler is not None and accumulated_iter <= lr_warmup_scheduler.T_max
        _, terms = T.train_one_iter(model, optimizer, lr_warmup_scheduler if warm else lr_scheduler, sync, batch,
                                    accumulated_iter)
        accumulated_iter += 1
        window.append(terms)
        if (i + 1) % log_interval == 0:
            if rank == 0 and logger is not None:
                mean = {k: float(torch.stack([w[k] for w in window]).mean()) for k in window[0]}
                logger.info('epoch[%d][%d/%d]: lr: %f, ' % (train_epoch, i + 1, len(train_loader), float(optimizer.lr))
                            + ', '.join('%s: %f' % kv for kv in mean.items()))
            window = []
    return accumulated_iter


def train_model(model, optimizer, train_loader, lr_scheduler, sync, start_epoch, total_epochs, start_iter, rank=0,
                logger=None, ckpt_save_dir=None, lr_warmup_scheduler=None, ckpt_save_interval=1, max_ckpt_save_num=50,
                log_interval=20):
    """Epoch loop with `checkpoint_epoch_%d.pth` files, oldest removed beyond max_ckpt_save_num (rank 0 only)."""
    it = start_iter
    for cur_epoch in range(start_epoch, total_epochs):
        trained = cur_epoch + 1
        it = train_one_epoch(model, optimizer, train_loader, lr_scheduler, sync, it, trained, rank, logger, log_interval,
                             lr_warmup_scheduler)
        if ckpt_save_dir is not None and trained % ckpt_save_interval == 0 and rank == 0:
            os.makedirs(ckpt_save_dir, exist_ok=True)
            old = sorted(glob.glob(os.path.join(ckpt_save_dir, 'checkpoint_epoch_*.pth')), key=os.path.getmtime)
            for f in old[:max(0, len(old) - max_ckpt_save_num + 1)]:
                os.remove(f)
            T.save_checkpoint(T.checkpoint_state(model, optimizer, trained, it),
                              os.path.join(ckpt_save_dir, 'checkpoint_epoch_%d' % trained))
    return it


def single_test(model, dataset, saveto=None, class_names=None, workers=2, rank=None, world=None, inflight=0,
                points_cap=None, raw_prefix=None, device_annos=False, ndim=4, tta=None, fuse_iou=None):
    """Run the detector over `dataset` (test mode) -> list of KITTI result annotations in dataset order on every rank
    (this rank's frames are computed here, the others' gathered from their ranks).  `saveto`: also write result files.
    inflight > 0: the frames' raw points go through model.frame_stream(...) with that many frames in flight (1..4) instead of
    collate + model(...): same annotations, the voxelizer and the anchor mask inside the captured frame.  `points_cap`: the
    largest cloud of the stream (default: from the sizes of this rank's point files).
    `raw_prefix` (with inflight > 0): a directory of RAW sweeps (%06d.bin, [N,4] f32 -- KITTI's velodyne/) read instead of
    dataset.lidar_prefix; the stream is built with raw_cap (the largest file, rounded up to 1024 points) and crops every
    sweep to the camera frustum of its own calib and img_shape inside the captured frame, so the annotations are those of
    the velodyne_reduced/ files.  points_cap (the most points a frustum may keep) then defaults to raw_cap: always enough,
    but the voxelizer's tables are sized for a whole sweep -- pass the real bound (KITTI: about a fifth of the sweep) to
    keep the frame's memory and its fill kernels at the size of the reduced path.
    `device_annos` (with inflight > 0): the stream is built with annos=True and every frame is submitted with its calib and
    img_shape, so the camera-frame annotation (location, alpha, the clipped 2-D box, the keep test) is computed inside the
    captured frame and only assembled on the host (kitti_common.result_anno_from_cam); False keeps kitti_bbox2results.
    `ndim` (with inflight > 0): float32 columns per point of the clouds the dataset loads (4: KITTI; a detector built with
    num_input_features = 5..8 needs at least that many).
    `tta` (with inflight > 0): a test-time augmentation spec (sassd.tta: a list of (flip, angle, scale) views, the first the
    identity) -- the stream detects on every view inside the captured frame and suppresses the views' candidates together.
    None leaves it to the model's test_cfg['tta'].
    `fuse_iou` (with inflight > 0): box fusion behind the stream's NMS (sassd.fuse: a number inside (0, 1)) -- every detection's
    box becomes the score-weighted mean of the candidates it suppressed, of all views under tta.  None leaves it to the
    model's test_cfg['fuse_iou']."""
    if rank is None or world is None:
        rank, _, world = D.env_world() if D.dist.is_initialized() else (0, 0, 1)
    if class_names is not None:
        setattr(model, 'class_names', class_names)
    model.eval()
    mine = D.frame_shard(len(dataset), rank, world)
    annos = []
    with torch.no_grad():
        if inflight:
            annos = _stream_test(model, dataset, mine, workers, inflight, points_cap, raw_prefix, device_annos, ndim, tta,
                                 fuse_iou)
        elif fuse_iou is not None:
            raise ValueError("fuse_iou needs inflight > 0 (the fusion is a node of the captured frame of a FrameStream)")
        elif tta is not None:
            raise ValueError("tta needs inflight > 0 (the views are made inside the captured frame of a FrameStream)")
        elif device_annos:
            raise ValueError("device_annos needs inflight > 0 (the annotations are written by the captured frame of a FrameStream)")
        elif raw_prefix is not None:
            raise ValueError("raw_prefix needs inflight > 0 (the crop lives in the captured frame of a FrameStream)")
        else:
            for batch in FrameLoader(dataset, 1, sampler=mine, num_workers=workers):
                annos += model(**batch)
    merged = [None] * len(dataset)
    for part_rank, part in enumerate(D.gather_results(annos) if world > 1 else [annos]):
        for idx, anno in zip(D.frame_shard(len(dataset), part_rank, world), part):
            merged[idx] = anno
    if saveto is not None and rank == 0:
        kitti.write_label_annos(merged, saveto)
    return merged


def _stream_test(model, dataset, indices, workers, inflight, points_cap=None, raw_prefix=None, device_annos=False, ndim=4,
                 tta=None, fuse_iou=None):
    """single_test's frames through a FrameStream: the point files are read ahead on `workers` threads, submitted as host
    clouds, and every result becomes the annotation forward_test builds for the frame's img_meta.  `ndim`: float32 columns
    per point of the files and of the clouds load_frame returns (4: KITTI)."""
    from concurrent.futures import ThreadPoolExecutor
    if not dataset.with_point:
        raise ValueError("single_test(inflight > 0) feeds raw points: the dataset needs with_point=True")
    indices = [int(i) for i in indices]
    if not indices:
        return []
    prefix = dataset.lidar_prefix if raw_prefix is None else raw_prefix
    raw_cap = None
    ndim = int(ndim)
    if points_cap is None or raw_prefix is not None:    # the files read below: [N, ndim] float32
        sizes = [os.path.getsize(os.path.join(prefix, '%06d.bin' % dataset.sample_ids[i])) for i in indices]
        if any(n % (4 * ndim) for n in sizes):
            raise ValueError("a point file under %s is not a whole number of %d-byte points%s"
                             % (prefix, 4 * ndim, "" if raw_prefix is not None else ": pass points_cap"))
        file_cap = (max(sizes) // (4 * ndim) + 1023) // 1024 * 1024 or 1024        # rounded up to 1024 points
        if raw_prefix is not None:
            raw_cap = file_cap
        if points_cap is None:
            points_cap = file_cap
    load = (dataset.load_frame, False) if raw_prefix is None else (dataset.load_frame, False, raw_prefix)
    gen = dataset.generator
    fs = model.frame_stream(dataset.anchors, inflight=inflight, points_cap=points_cap, batch_size=1, device=dataset._dev(),
                            **({} if ndim == 4 else dict(ndim=ndim)),
                            **({} if raw_cap is None else dict(raw_cap=raw_cap)),
                            **(dict(annos=True) if device_annos else {}),
                            **({} if tta is None else dict(tta=tta)),
                            **({} if fuse_iou is None else dict(fuse_iou=fuse_iou)),
                            anchors_bv=dataset.anchors_bv, voxel_size=tuple(gen.voxel_size),
                            point_cloud_range=tuple(gen.point_cloud_range), max_num_points=gen.max_num_points_per_voxel,
                            max_voxels=gen._max_voxels, anchor_area_threshold=dataset.anchor_area_threshold)
    metas, annos = deque(), []
    try:
        with ThreadPoolExecutor(max(1, int(workers))) as pool:
            def batches():
                ahead = max(1, int(workers)) + inflight
                pending = deque(pool.submit(load[0], i, *load[1:]) for i in indices[:ahead])
                nxt = len(pending)
                while pending:
                    fr = pending.popleft().result()
                    if nxt < len(indices):
                        pending.append(pool.submit(load[0], indices[nxt], *load[1:]))
                        nxt += 1
                    metas.append(dict(img_shape=fr['img_shape'], sample_idx=fr['sample_idx'], calib=fr['calib']))
                    view = [dict(calib=fr['calib'], img_shape=fr['img_shape'])]
                    if raw_prefix is not None:          # a raw stream's dict frustums serve as its calibs too
                        yield [fr['points']], view
                    elif device_annos:
                        yield [fr['points']], None, view
                    else:
                        yield [fr['points']]
            for _, dets in fs.map(batches()):
                annos += model.result_annos(dets, [metas.popleft()])
    finally:
        fs.close()
    return annos


def evaluate(dataset, outputs, class_names=None):
    """tools/test.py:155-158: the official KITTI report of `outputs` against the dataset's label files."""
    from .kitti_eval import get_official_eval_result
    gt_annos = kitti.get_label_annos(dataset.label_prefix, dataset.sample_ids)
    return get_official_eval_result(gt_annos, outputs, current_classes=class_names or dataset.class_names)
