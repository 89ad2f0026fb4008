"""Generate tests/golden/head_fns_exp.npz: every torch.exp the reference's second_box_decode evaluated while
make_golden.py produced head_fns.npz -- its input and its float32 result.

The decoded boxes of head_fns.npz go through three torch.exp calls (the size columns), and torch's float32 exp is not
the same function on every host CPU: the last bit of a result may differ between machines (seen on one of these 192
values).
With these values test_head_oracle_vs_reference_functions serves the oracle's exp calls from the table and keeps its
bit-exact comparison on any host; it checks the host's own exp against them separately.

    python tests/golden/make_golden_head_exp.py        (same machine and reference tree as make_golden.py)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402


class _RecordingTorch:
    """torch for the exec'd reference function, with torch.exp recorded"""

    def __init__(self):
        self.calls = []

    def exp(self, x):
        y = torch.exp(x)
        self.calls.append((x.detach().clone(), y.detach().clone()))
        return y

    def __getattr__(self, name):
        return getattr(torch, name)


def main():
    G = np.load(os.path.join(HERE, "head_fns.npz"))
    rec = _RecordingTorch()
    g = MG.ref_functions(os.path.join(MG.REF, "mmdet/models/single_stage_heads/ssd_rotate_head.py"),
                         {"second_box_decode"}, {"torch": rec, "np": np})
    dec = g["second_box_decode"](torch.from_numpy(G["enc"]), torch.from_numpy(G["anchors"]))
    assert np.array_equal(dec.numpy(), G["dec"]), "this host does not reproduce head_fns.npz (run where it was made)"
    assert len(rec.calls) == 3, len(rec.calls)
    x = np.stack([np.ascontiguousarray(a.numpy()).reshape(-1) for a, _ in rec.calls])
    y = np.stack([np.ascontiguousarray(b.numpy()).reshape(-1) for _, b in rec.calls])
    np.savez_compressed(os.path.join(HERE, "head_fns_exp.npz"), x=x, exp_x=y)
    print("head fns exp", x.shape)


if __name__ == "__main__":
    main()
