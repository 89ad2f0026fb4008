"""Mirror of the spconv v1.0 surface the reference uses (mmdet/models/necks/cmn.py:1,109-112,138-173,208-212;
mmdet/core/bbox/transforms.py:218-223): SparseConvTensor(.features/.indices/.dense()), SubMConv3d, SparseConv3d,
SparseSequential -- same constructor arguments, same weight layout [kz,ky,kx,Cin,Cout] (checkpoint compatible),
same `indice_key` rulebook sharing.  All arithmetic runs in libsassd (hash/bitmap rulebook + MFMA gather conv).

This module-by-module facade is the drop-in/compatibility path (one host read of the output row count per strided
conv, because the reference API exposes exact-size tensors); the fused, sync-free production path is
sassd.pipeline.InferencePlan, which calls the same kernels with folded BatchNorm.
"""
import math

import numpy as np
import torch
from torch import nn

from . import kernels as K
from . import weight_images
from . import autograd as AG
from .autograd import BnReluFn, DensifyFn, SparseConvFn, count_bn_batch, _n_ptr as _cached_n_ptr


class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size):
        self.features = features
        self.indices = indices
        self.spatial_shape = [int(s) for s in spatial_shape]
        self.batch_size = int(batch_size)
        self.indice_dict = {}          # indice_key -> (out_indices, nbr, out_shape, hash table)
        self._table = None
        # bf16 sparse training (autograd.set_sparse_precision("bf16")): `features` is then a bf16 tensor without autograd history
        # and `_carrier` the fp32 stride-0 tensor that owns its autograd edge (see autograd.py); features_f32() for everyone else
        self._carrier = None

    def features_f32(self):
        """The features as a differentiable fp32 tensor: `features` itself, or bf16 training features widened exactly."""
        if self._carrier is not None:
            return AG.WidenBf16Fn.apply(self._carrier, self.features)
        return self.features

    @property
    def spatial_size(self):
        return int(np.prod(self.spatial_shape))

    def _n_ptr(self):
        return _cached_n_ptr(self.indices.shape[0], self.indices.device)        # read-only [1] int32, cached per value

    def table(self):
        if self._table is None:
            idx = self.indices.int().contiguous()
            cap = max(idx.shape[0], 1)
            self._table = K.HashTable(cap, idx.device).build(idx, self._n_ptr(), self.spatial_shape, self.batch_size)
        return self._table

    def dense(self, channels_first=True):
        """[B, C, D, H, W] like spconv (scatter_nd + permute)."""
        d, h, w = self.spatial_shape
        c = self.features.shape[1]
        n = self.indices.shape[0]
        feats = self.features_f32()
        if torch.is_grad_enabled() and feats.requires_grad:
            out = DensifyFn.apply(feats.float(), self.indices.int().contiguous(), (d, h, w), self.batch_size)
            return out if channels_first else out.permute(0, 2, 3, 4, 1).contiguous()
        out = K.densify(feats.contiguous(), self.indices.int().contiguous(), self._n_ptr(), max(n, 1),
                        (d, h, w), self.batch_size, 0)
        out = out.view(self.batch_size, c, d, h, w)
        return out if channels_first else out.permute(0, 2, 3, 4, 1).contiguous()


def _triple(v):
    return tuple(v) if isinstance(v, (list, tuple)) else (v, v, v)


class SparseConvolution(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=False, subm=False,
                 indice_key=None):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = _triple(kernel_size), _triple(stride), _triple(padding)
        self.subm, self.indice_key = subm, indice_key
        self.conv1x1 = int(np.prod(self.kernel_size)) == 1
        self.weight = nn.Parameter(torch.empty(*self.kernel_size, in_channels, out_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)      # .to() / .cuda() on this layer alone: its packed image is stale
        K.bump_weights_generation()
        return out

    def reset_parameters(self):
        n = self.in_channels * int(np.prod(self.kernel_size))
        stdv = 1.0 / math.sqrt(n)
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.uniform_(-stdv, stdv)

    def packed_weight(self):
        def build():
            k = int(np.prod(self.kernel_size))
            w = self.weight.detach().reshape(k, self.in_channels, self.out_channels).contiguous().float()
            return K.spconv_pack_weight(w)
        return weight_images.image(self.weight, "spconv", build)

    def _conv(self, feats, nbr, n_out, k, grad):
        """Raw conv (+bias) over a gather table: autograd-recording HIP path when gradients are wanted."""
        cin, cout = self.in_channels, self.out_channels
        if grad:
            y = SparseConvFn.apply(feats, self.weight.view(k, cin, cout), nbr, n_out, self.packed_weight(),
                                   isinstance(self, SubMConv3d))
            return y + self.bias if self.bias is not None else y
        bias = self.bias.detach() if self.bias is not None else None
        n_ptr = _cached_n_ptr(n_out, feats.device)
        return K.spconv_fwd(feats, nbr, n_ptr, max(n_out, 1), self.packed_weight(), k, cin, cout, None, bias)[:n_out]

    def book(self, inp):
        """Rulebook of this layer for `inp`'s coordinates: (out_indices, nbr, out_shape, out_table).  Coordinate-only
        work (hash / bitmap kernels + ONE host read of the output row count for strided layers); cached per
        `indice_key` in `inp.indice_dict`, so it can be built ahead of the forward pass (VxNet.precompute_rulebooks)."""
        idx = inp.indices.int().contiguous()
        n = idx.shape[0]
        if self.kernel_size != (3, 3, 3):
            raise NotImplementedError("only k=3 and k=1 sparse convs exist on the SA-SSD path")
        book = inp.indice_dict.get(self.indice_key) if self.indice_key is not None else None
        if book is not None:
            return book
        if self.subm:
            nbr = K.rulebook_subm(idx, inp._n_ptr(), max(n, 1), inp.spatial_shape, inp.batch_size, inp.table())
            book = (idx, nbr, inp.spatial_shape, inp._table)
        else:
            if self.stride != (2, 2, 2) or self.padding != (1, 1, 1):
                raise NotImplementedError("strided sparse conv is k=3,s=2,p=1 on the SA-SSD path (cmn.py:170)")
            cap_out = max(8 * n, 1)
            oi, on, nbr = K.rulebook_conv(idx, inp._n_ptr(), max(n, 1), inp.spatial_shape, inp.batch_size,
                                          inp.table(), cap_out)
            n_out = int(on.item())            # compatibility path: exact-size tensors need the count
            book = (oi[:n_out].contiguous(), nbr[:max(n_out, 1)].contiguous(),
                    list(K.conv_out_shape(inp.spatial_shape)), None)
        if self.indice_key is not None:
            inp.indice_dict[self.indice_key] = book
        return book

    def _bf16_train(self, inp):
        """Does this call run on the bf16 training kernels?  bf16 sparse mode, gradients wanted, device features, and not the
        narrow first layer (Cin < 16: voxel means in metres stay fp32)."""
        f = inp.features
        return (AG.sparse_precision() == "bf16" and torch.is_grad_enabled() and f.is_cuda and self.in_channels >= 16
                and (inp._carrier is not None or f.requires_grad or self.weight.requires_grad))

    def _forward_bf16(self, inp, bn):
        """bf16 training path: conv (+ the BatchNorm1d + ReLU that follow, `bn`, as one autograd node).  A layer shape without
        bf16 kernels is an error, never a silent fp32 layer."""
        cin, cout = self.in_channels, self.out_channels
        n = inp.indices.shape[0]
        if self.conv1x1:
            k, nbr, out_idx, oshape, otable, n_out = 1, None, inp.indices, inp.spatial_shape, inp._table, n
        else:
            out_idx, nbr, oshape, otable = self.book(inp)
            k, n_out = 27, out_idx.shape[0]
            if self.subm:
                otable = inp._table
        cap = max(n_out, n, 1) if nbr is None else max(nbr.shape[0], n, 1)
        if not AG.sparse_bf16_layer_supported(k, cin, cout, cap):
            raise ValueError("sparse_precision='bf16': no bf16 training kernels for sparse conv %s (%d -> %d, kernel %s, %d rows)"
                             % (self.indice_key or type(self).__name__, cin, cout, "x".join(map(str, self.kernel_size)), cap))
        if inp._carrier is not None:
            carrier, xb = inp._carrier, inp.features
        else:                                         # fp32 features enter the bf16 trunk: rounded once (nearest even)
            carrier = inp.features.contiguous().float()
            xb = carrier.detach().to(torch.bfloat16)
        w = self.weight.view(k, cin, cout)
        subm = isinstance(self, SubMConv3d)
        out = SparseConvTensor(None, out_idx, oshape, inp.batch_size)
        out.indice_dict, out._table = inp.indice_dict, otable
        if bn is not None and self.bias is None and n_out > 0:
            out._carrier, out.features = AG.SparseConvBnReluBf16Fn.apply(carrier, xb, w, nbr, n_out, subm, bn.weight, bn.bias,
                                                                        bn.running_mean, bn.running_var, bn.momentum, bn.eps)
            count_bn_batch(bn)
            out._bn_fused = True
        else:
            y = AG.SparseConvBf16Fn.apply(carrier, xb, w, nbr, n_out, subm)
            out.features = y + self.bias if self.bias is not None else y
        return out

    def forward(self, inp, bn=None):
        """bn: the training-mode BatchNorm1d (+ ReLU) that follows this layer in a SparseSequential; only the bf16 training path
        fuses it (the result then carries `_bn_fused`)."""
        assert isinstance(inp, SparseConvTensor)
        if self.in_channels < 16 and self.in_channels != 4 and not (
                self.subm and self.kernel_size == (3, 3, 3) and K.spconv_in_routed(27, self.in_channels, self.out_channels)):
            # the input-layer kernels cover SubMConv3d(3..8, 16, 3) only: no 1x1x1 or strided form of a narrow layer
            raise NotImplementedError("sparse conv %s (%s, %d -> %d, kernel %s): a layer of fewer than 16 input channels runs "
                                      "as SubMConv3d(Cin, 16, 3) with Cin in 3..8 only"
                                      % (self.indice_key or "<no indice_key>", type(self).__name__, self.in_channels,
                                         self.out_channels, "x".join(map(str, self.kernel_size))))
        if self._bf16_train(inp):
            return self._forward_bf16(inp, bn)
        feats = inp.features_f32().contiguous().float()
        n = inp.indices.shape[0]
        grad = torch.is_grad_enabled() and (feats.requires_grad or self.weight.requires_grad)
        if self.conv1x1:
            # spconv shortcut: features @ weight.view(Cin, Cout), indices unchanged
            y = self._conv(feats, None, n, 1, grad)
            out = SparseConvTensor(y, inp.indices, inp.spatial_shape, inp.batch_size)
            out.indice_dict, out._table = inp.indice_dict, inp._table
            return out
        out_idx, nbr, oshape, otable = self.book(inp)
        n_out = out_idx.shape[0]
        y = self._conv(feats, nbr, n_out, 27, grad)
        out = SparseConvTensor(y, out_idx, oshape, inp.batch_size)
        out.indice_dict = inp.indice_dict
        out._table = otable if not self.subm else inp._table
        return out


class SubMConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, bias, True, indice_key)


class SparseConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, bias, False, indice_key)


class SparseSequential(nn.Sequential):
    """Sparse modules consume/produce SparseConvTensor; plain nn.Modules are applied to `.features`."""

    # Training-mode BatchNorm1d -> ReLU pairs run as one fused HIP forward / backward pair (sassd_bn_relu_*, 2 launches
    # each way instead of torch's 6: collect / transform / clamp, threshold / reduce / elementwise).  Statistics are
    # accumulated in double and rounded once, i.e. within fp32 rounding of the exact batch statistics (torch's fp32
    # Welford and the CPU oracle's fp32 two-pass mean / variance are too; the unit test holds the kernels to torch at
    # 2e-5 / 1e-4).  Set to False for torch's own BatchNorm1d + ReLU (A/B, bench.py --torch-bn).
    fuse_bn_relu = True

    def _fusable_bn(self, m, nxt, channels):
        return (self.fuse_bn_relu and isinstance(m, nn.BatchNorm1d) and isinstance(nxt, nn.ReLU) and m.training
                and m.affine and m.track_running_stats and m.momentum is not None and torch.is_grad_enabled()
                and K.bn_relu_supported(1, channels))

    def forward(self, inp):
        mods = list(self)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, SparseConvolution):
                if AG.sparse_precision() == "bf16" and m._bf16_train(inp):
                    # bf16 sparse training: conv + BatchNorm1d + ReLU are one autograd node (SparseConvBnReluBf16Fn)
                    bn = mods[i + 1] if i + 2 < len(mods) and self._fusable_bn(mods[i + 1], mods[i + 2], m.out_channels) else None
                    inp = m(inp, bn)
                    if getattr(inp, "_bn_fused", False):
                        i += 3
                        continue
                else:
                    inp = m(inp)
            elif isinstance(inp, SparseConvTensor):
                if inp.indices.shape[0] != 0:
                    f = inp.features
                    nxt = mods[i + 1] if i + 1 < len(mods) else None
                    if (self.fuse_bn_relu and isinstance(m, nn.BatchNorm1d) and isinstance(nxt, nn.ReLU) and m.training
                            and m.affine and m.track_running_stats and m.momentum is not None and f.is_cuda
                            and f.dtype == torch.float32 and torch.is_grad_enabled()
                            and K.bn_relu_supported(f.shape[0], f.shape[1])):
                        if AG.sparse_precision() == "bf16":
                            # behind an fp32 conv (the first layer): the same BatchNorm + ReLU, stored bf16 for the next conv
                            inp._carrier, inp.features = AG.BnReluBf16OutFn.apply(f, m.weight, m.bias, m.running_mean,
                                                                                  m.running_var, m.momentum, m.eps)
                        else:
                            inp.features = BnReluFn.apply(f, m.weight, m.bias, m.running_mean, m.running_var, m.momentum,
                                                          m.eps)
                        count_bn_batch(m)
                        i += 2
                        continue
                    if inp._carrier is not None:              # a plain module on bf16 training features: widened exactly
                        f, inp._carrier = inp.features_f32(), None
                    inp.features = m(f)
            else:
                inp = m(inp)
            i += 1
        return inp
