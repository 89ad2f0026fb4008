#!/usr/bin/env python
"""Kernel-level times of the part-sensitive head: the two dense launches (sassd_conv2d_fwd 3x3 256 -> 28 + sassd_conv1x1_narrow_fwd
28 -> 28) against the sampled path (sassd_ps_pixel_list + sassd_ps_head_sampled) for candidate sets of growing size on the
car grid (200 x 176), up to a set that tiles the map -- every pixel listed, the worst case the sampled launch is sized for.
Candidates are car-sized boxes (1.6 x 3.9 m on the 0.4 m grid) at random positions and angles; `--boxes 0` lists every pixel by
hand.  Prints one line per case: candidates, listed pixels, us per call (hipEvents around `--iters` back-to-back calls).
usage: python tools/bench_ps_sampled.py [--iters 200] [--boxes 200 600 2000 0]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sassd  # noqa: E402,F401
from sassd import kernels as K  # noqa: E402


def timed(fn, iters):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--boxes", type=int, nargs="*", default=[200, 600, 2000, 0])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h, w, cin, parts, cap_k = 200, 176, 256, 28, 4096
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, cin, h, w, generator=g).to(dev)
    wp = K.conv2d_pack_weight((torch.randn(parts, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5).to(dev))
    w1t = K.conv1x1_narrow_pack_weight((torch.randn(parts, parts, 1, 1, generator=g) * (1.0 / parts) ** 0.5).to(dev))
    scale, shift = (torch.rand(parts, generator=g) + 0.5).to(dev), (torch.randn(parts, generator=g) * 0.1).to(dev)
    t0, dense = torch.empty(1, parts, h, w, device=dev), torch.empty(1, parts, h, w, device=dev)

    def dense_pair():
        K.conv2d_fwd(x, wp, parts, 3, scale, shift, True, t0)
        K.conv1x1_narrow_fwd(t0, w1t, parts, None, None, False, dense)
    print("dense 3x3 + 1x1: %.1f us (3x3 alone %.1f us)" %
          (timed(dense_pair, a.iters), timed(lambda: K.conv2d_fwd(x, wp, parts, 3, scale, shift, True, t0), a.iters)))
    buf = K.ps_pixel_list_buffer(1, h, w, dev)
    y = torch.zeros(1, parts, h, w, device=dev)
    rng = np.random.default_rng(0)
    for nb in a.boxes:
        guided = np.zeros((1, cap_k, 7), np.float32)
        nb = min(nb, cap_k)
        guided[0, :nb] = np.stack([rng.uniform(0, 70.4, nb), rng.uniform(-40, 40, nb), np.zeros(nb), np.full(nb, 1.6),
                                   np.full(nb, 3.9), np.full(nb, 1.56), rng.uniform(-3.14, 3.14, nb)], 1)
        gd = torch.from_numpy(guided).to(dev)
        cnt = torch.tensor([nb], dtype=torch.int32, device=dev)

        def make_list():
            K.ps_pixel_list(gd, cnt, cap_k, 1, h, w, (0.0, 40.0), 2.5, out=buf)
        t_list = timed(make_list, a.iters)
        counts, pixels, _ = K.ps_pixel_list_views(buf, 1, h, w)
        if nb == 0:                                 # the worst case: every pixel listed
            counts[0] = h * w
            pixels[0] = torch.arange(h * w, dtype=torch.int32, device=dev)
        t_head = timed(lambda: K.ps_head_sampled(x, wp, scale, shift, True, w1t, None, None, False, buf, y), a.iters)
        n = int(counts[0].item())
        px = pixels[0, :n].long()
        dense_pair()
        same = torch.equal(y[0].reshape(parts, -1)[:, px], dense[0].reshape(parts, -1)[:, px])
        print("%5s candidates: %6d of %d pixels listed; list (fill + mark + compact) %.1f us, sampled head %.1f us; "
              "bit-identical to the dense kernels at the listed pixels: %s" % (nb if nb else "all", n, h * w, t_list, t_head, same))


if __name__ == "__main__":
    main()
