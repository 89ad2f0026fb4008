"""The one store of cached weight images on the training / facade path.  A weight image is a kernel-layout copy of a conv
weight: MFMA-fragment packs, Winograd G g G^T, bf16 packs and the transposed / tap-mirrored twins the data gradients read.

    image(weight, kind, build, extra=())    the image; build() runs on a miss
    install(weight, kind, image, extra=())  an image made elsewhere (sassd.train.PackPlan after its gather launch)
    peek(weight, kind, extra=())            the valid cached image or None
    pinned(weight, kind, extra=())          the tensor a valid entry keeps alive, or None

One rule for every kind:

  * key (address, numel, kind) + extra.  `kind` names the layout ("spconv", "spconv_t", "spconv_t_rev", "spconv16", "spconv16_t",
    "spconv16_t_rev", "direct", "wino2",
    "wino4", "dgrad", "bf16_3x3", "bf16_3x3_t", "bf16_1x1", "bf16_1x1_t"); `extra` carries (h, w) where the FORM of the image
    depends on the map size (the fp32 data-gradient image of a 3x3 layer).
  * an entry is valid while kernels.weight_key(weight) -- version counter, address, device, global generation -- equals the
    value stored with it.  Raw-pointer writers (the fused optimizer, a broadcast, a checkpoint load) bump the generation.
  * an entry PINS the storage it was packed from.  A fresh tensor can land on the address of a dead one with the same size,
    version 0 and the same generation, and would then be handed the dead tensor's image (round 5: the sparse data gradient
    of the third 64 -> 64 layer a test created ran on the first one's transposed weights); while the entry lives that
    storage cannot be freed.  It never pins an autograd graph: a weight with a grad_fn (SparseConvolution hands
    weight.view(k, cin, cout) to SparseConvFn) is pinned through its detached alias.
  * a tensor that is neither a leaf nor a view of one is never cached.  The fused RPN head's torch.cat of three conv
    weights is fresh storage every step with `_version` 0 on an address the caching allocator hands back: it has no
    generation of its own, and after an optimizer step on its sources a cached image would be silently stale.
    A view of a parameter shares the parameter's version counter and address and is cached.
  * bounded, least recently USED first (insertion order dropped the long-lived parameter images a PackPlan
    installs first once 256 transient keys had piled up).  A dropped entry only costs a re-pack."""
from collections import OrderedDict

from . import kernels as K


class ImageStore:
    MAX = 256            # one car_cfg detector in bf16 mode with its PackPlan holds fewer than half (tests/test_gpu_train_fused.py)

    def __init__(self):
        self._entries = OrderedDict()              # key -> (weight_key, image, pinned source); the front is the oldest

    def __len__(self):
        return len(self._entries)

    def clear(self):
        self._entries.clear()

    def _valid(self, weight, kind, extra):
        """-> (key, weight_key, the valid entry or None); a hit moves to the young end."""
        gen = K.weight_key(weight)
        key = (gen[1], weight.numel(), kind) + extra
        hit = self._entries.get(key)
        if hit is not None and hit[0] == gen:
            self._entries.move_to_end(key)
            return key, gen, hit
        return key, gen, None

    def _put(self, key, gen, image, weight):
        self._entries[key] = (gen, image, weight.detach() if weight.grad_fn is not None else weight)
        self._entries.move_to_end(key)
        while len(self._entries) > self.MAX:
            self._entries.popitem(last=False)

    def image(self, weight, kind, build, extra=()):
        key, gen, hit = self._valid(weight, kind, extra)
        if hit is not None:
            return hit[1]
        image = build()
        if weight.grad_fn is None or (weight._is_view() and weight._base.grad_fn is None):
            self._put(key, gen, image, weight)
        return image

    def install(self, weight, kind, image, extra=()):
        self._put((weight.data_ptr(), weight.numel(), kind) + extra, K.weight_key(weight), image, weight)

    def peek(self, weight, kind, extra=()):
        hit = self._valid(weight, kind, extra)[2]
        return None if hit is None else hit[1]

    def pinned(self, weight, kind, extra=()):
        hit = self._valid(weight, kind, extra)[2]
        return None if hit is None else hit[2]


store = ImageStore()
image, install, peek, pinned = store.image, store.install, store.peek, store.pinned
