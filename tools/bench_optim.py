"""The three update kernels (sassd_adam_step, sassd_adam_l2_step, sassd_sgd_step) on the car_cfg parameter count, in one
process.

Flat fp32 buffers of the size FlatParams gives the car_cfg detector (5.34 M elements), random contents, the clip on
(max_norm 10, the square sum computed once outside the timed window: the update kernels alone are timed).  The kernels and
two device copies are run in alternating blocks, `--repeats` blocks each, after `--warmup` untimed launches; a block is
`--iters` back-to-back launches between two HIP events, its figure the mean per launch.  Per kernel: the median and
min..max over the blocks in microseconds, the bytes of its byte model (28 B per element for both Adam kernels, 20 B for
SGD) over that time, and that rate as a fraction of the measured copy peak -- the rate (read + written bytes) of a
device-to-device copy of `--copy-mib` MiB, far beyond the 256 MB Infinity Cache.  The optimizer's working set (64 .. 85 MB)
fits that cache, so a copy of the parameter buffer's own size is reported beside it.  One JSON record; no target.

    python tools/bench_optim.py [--iters 200] [--warmup 20] [--repeats 5] [--out profiles/optim_family.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sassd import _C, kernels as K, synth, train  # noqa: E402


def car_cfg_numel():
    model, _ = synth.build_detector_for(synth.workload("car"), 0, train=True, cls_bias=-3.0)
    return train.FlatParams(model).numel


def _spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=0, help="elements (default: the car_cfg detector's flat parameter count)")
    ap.add_argument("--copy-mib", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.n or car_cfg_numel()
    g = torch.Generator(device="cpu").manual_seed(0)
    p, grad, s0 = (torch.randn(n, generator=g).to(dev) for _ in range(3))
    s1 = torch.rand(n, generator=g).to(dev)
    sumsq = K.grad_sumsq(grad)
    big = torch.empty(2, a.copy_mib * (1 << 20) // 4, dtype=torch.float32, device=dev).normal_()
    small = torch.empty_like(p)
    step = [0]

    def adam_onecycle():
        step[0] += 1
        K.adam_step(p, grad, s0, s1, sumsq, 1e-3, 0.9, 0.99, 1e-8, 0.01, step[0], 10.0, 1.0)

    def adam_l2():
        step[0] += 1
        K.adam_l2_step(p, grad, s0, s1, sumsq, 1e-3, 0.9, 0.999, 1e-8, 0.01, step[0], 10.0, 1.0)

    work = {                                                   # name -> (launch, bytes moved per launch)
        "sassd_adam_step": (adam_onecycle, 28 * n),
        "sassd_adam_l2_step": (adam_l2, 28 * n),
        "sassd_sgd_step": (lambda: K.sgd_step(p, grad, s0, sumsq, 1e-3, 0.9, 0.01, 10.0, 1.0), 20 * n),
        "copy_large": (lambda: big[1].copy_(big[0]), 2 * big[0].numel() * 4),
        "copy_parameter_size": (lambda: small.copy_(p), 8 * n),
    }
    for fn, _ in work.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in work}
    for _ in range(a.repeats):
        for name, (fn, _) in work.items():
            iters = a.iters if not name.startswith("copy_large") else max(4, a.iters // 20)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    assert bool(torch.isfinite(p).all())
    rate = {k: work[k][1] / (statistics.median(v) * 1e-6) / 1e9 for k, v in us.items()}       # GB/s at the median
    peak = rate["copy_large"]
    rec = dict(workload="update kernels on flat fp32 buffers of the car_cfg parameter count, clip on, random contents",
               elements=n, iters=a.iters, warmup=a.warmup, repeats=a.repeats, copy_mib=a.copy_mib,
               csrc_hash=_C.csrc_hash(), device=torch.cuda.get_device_name(0),
               copy_peak_GBps=round(peak, 1), copy_parameter_size_GBps=round(rate["copy_parameter_size"], 1),
               note="copy_peak: read + written bytes of a %d MiB device copy over its time; the kernels' working set fits "
                    "the Infinity Cache, the large copy does not" % a.copy_mib,
               results={k: dict(us=_spread(us[k]), bytes_per_element=work[k][1] // n, GBps=round(rate[k], 1),
                                fraction_of_copy_peak=round(rate[k] / peak, 3))
                        for k in work if k.startswith("sassd_")})
    for k, r in rec["results"].items():
        print("%-20s %.2f us [%.2f..%.2f]  %.0f GB/s  %.2f of the copy peak %.0f GB/s" % (
            k, r["us"]["median"], r["us"]["min"], r["us"]["max"], r["GBps"], r["fraction_of_copy_peak"], peak), flush=True)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
