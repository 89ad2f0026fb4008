"""CPU: the one validity rule of sassd.weight_images (key, generation, pin, derived tensors, install) on CPU tensors with a
counting builder -- no kernel runs."""
import torch

from sassd import kernels as K
from sassd import weight_images as WI


class _Builder:
    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return torch.full((3,), float(self.calls))


def test_hit_does_not_build_and_each_invalidation_builds_once():
    s, b = WI.ImageStore(), _Builder()
    w = torch.nn.Parameter(torch.randn(8, 4))
    first = s.image(w, "direct", b)
    assert b.calls == 1 and s.image(w, "direct", b) is first and s.peek(w, "direct") is first and b.calls == 1
    K.bump_weights_generation()                            # a raw-pointer writer (fused optimizer, broadcast, checkpoint load)
    assert s.peek(w, "direct") is None
    second = s.image(w, "direct", b)
    assert b.calls == 2 and second is not first and s.image(w, "direct", b) is second and b.calls == 2
    with torch.no_grad():
        w.mul_(2.0)                                        # an in-place edit moves `_version`
    assert s.peek(w, "direct") is None
    third = s.image(w, "direct", b)
    assert b.calls == 3 and s.image(w, "direct", b) is third and b.calls == 3 and len(s) == 1
    # kinds and extras are separate images of the same weight
    s.image(w, "dgrad", b, (200, 176))
    s.image(w, "dgrad", b, (100, 88))
    assert b.calls == 5 and len(s) == 3 and s.peek(w, "dgrad") is None and s.peek(w, "dgrad", (200, 176)) is not None


def test_views_of_a_parameter_share_one_entry_and_pin_no_graph():
    s, b = WI.ImageStore(), _Builder()
    w = torch.nn.Parameter(torch.randn(3, 3, 3, 4, 8))
    v1, v2 = w.view(27, 4, 8), w.view(27, 4, 8)
    assert v1.grad_fn is not None and not v1.is_leaf
    img = s.image(v1, "spconv_t", b)
    assert s.image(v2, "spconv_t", b) is img and s.image(w, "spconv_t", b) is img and b.calls == 1
    src = s.pinned(v2, "spconv_t")
    assert src.grad_fn is None and src.data_ptr() == w.data_ptr()          # the storage, never the autograd graph
    # the weight as SparseConvFn.backward sees it: unpacked from the saved tensors of a custom Function
    seen = []

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, weight):
            ctx.save_for_backward(weight)
            return weight.sum()

        @staticmethod
        def backward(ctx, g):
            (weight,) = ctx.saved_tensors
            seen.append(s.image(weight, "spconv_t", b))
            return g.expand_as(weight)
    Fn.apply(w.view(27, 4, 8)).backward()
    assert seen[0] is img and b.calls == 1


def test_derived_weight_is_rebuilt_every_call_and_leaves_no_entry():
    s, b = WI.ImageStore(), _Builder()
    parts = [torch.nn.Parameter(torch.randn(2, 4, 1, 1)) for _ in range(3)]
    for n in (1, 2, 3):
        s.image(torch.cat(parts, 0), "bf16_1x1", b)        # the fused head's weight: fresh storage, `_version` 0, every step
        assert b.calls == n and len(s) == 0


def test_install_then_image_returns_the_installed_object():
    s, b = WI.ImageStore(), _Builder()
    w = torch.nn.Parameter(torch.randn(4, 4, 1, 1))
    mine = dict(packed=torch.zeros(2))
    s.install(w, "dgrad", mine)
    assert s.image(w, "dgrad", b) is mine and s.peek(w, "dgrad") is mine and s.pinned(w, "dgrad") is w and b.calls == 0
    K.bump_weights_generation()
    assert s.image(w, "dgrad", b) is not mine and b.calls == 1
    s.install(w, "dgrad", mine)                            # (PackPlan.run after the next optimizer step)
    assert s.image(w, "dgrad", b) is mine and b.calls == 1 and len(s) == 1


def test_a_fresh_tensor_cannot_take_a_cached_tensors_address():
    """Round 5: a tensor created after a cached one died landed on its address with the same size, version 0 and the same
    generation, and was handed the dead tensor's image.  The entry keeps the storage alive, so the address stays taken."""
    s, b = WI.ImageStore(), _Builder()
    t = torch.zeros(27 * 64 * 64)
    ptr = t.data_ptr()
    s.image(t, "spconv_t", b)
    del t                                                  # the last reference outside the store
    fresh = [torch.zeros(27 * 64 * 64) for _ in range(64)]  # (without the entry the allocator hands `ptr` straight back)
    assert ptr not in {f.data_ptr() for f in fresh}
    for f in fresh:
        assert s.peek(f, "spconv_t") is None
    assert s.image(fresh[0], "spconv_t", b) is not None and b.calls == 2
