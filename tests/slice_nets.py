"""Test helper: the pbtxt of the sliced nets that tests/test_slices_cpu.py and tests/test_slices_net_gpu.py share.

 * ``verification_net`` (nets A and B): 3 x 9 x 9 input; ``h1`` = slices a, b (no channels of its own) written by a 3 x 3 pad-1 conv into
   ``a`` and a 5 x 5 pad-2 conv into ``b`` (channel concatenation); ``h2`` = slices a:5, b:3 written by the 3 x 3 pad-1 convs h1.a -> h2.a
   and h1.b -> h2.b (a grouped convolution); 3 x 3 stride-2 pool, FC, 10-way softmax.  At batch 5 slice ``b`` of h2 starts 5 * 81 * 5 =
   2025 floats into the layer — a view whose base is 4-byte aligned only; with h1 = a:3, b:7 so does h1.b (1215 floats).
 * ``wide_net`` (net C): the same pattern with slice widths that are multiples of 16 and one group of 128 -> 192 filters on 13 x 13
   pixels, the smallest sizes at which that group's three GEMMs meet the conditions of the wide kernels at batch 64
   (csrc/patch_gemm.hip patch_shape_ok / wide_plan, csrc/wgrad_wide.hip wgw_try; the reasoning is at WIDE below).
 * the planner's variants of the verification net: a second writer into one slice, one slice left unread.
"""
from convnet_amd import models
from convnet_amd.models import _conv, _fc, _header, _layer, _on, _pool, _slices

RELU, LINEAR = ("RECTIFIED_LINEAR", "MAXPOOL"), ("LINEAR", "AVERAGE_POOL")


def verification_net(h1=(("a", 4), ("b", 6)), h2=(("a", 5), ("b", 3)), kinds=RELU, dropprob=0.0, grad_check=False, size=9,
                     extra_edges="", read=("a", "b"), init_wt=1.0, pool_window=(3, 2)):
    """``h1`` / ``h2``: (name, channels) of the slices IN DECLARATION ORDER.  ``read``: the slices of h1 that a group of h2 reads."""
    act, pool = kinds
    gc = models._gc(grad_check, 6)
    s = _header("slices_net")
    s += _layer("input", 3, size=size)
    s += _layer("h1", 0, act, dropprob, extra=_slices(**dict(h1))) + _layer("h2", 0, act, dropprob, extra=_slices(**dict(h2)))
    s += _layer("pool", sum(c for _, c in h2)) + _layer("output", 10, "SOFTMAX")
    s += _on(_conv("input", "h1", 3, 1, 1, init_wt=init_wt, grad_check=gc), "", "a")
    s += _on(_conv("input", "h1", 5, 1, 2, init_wt=init_wt, grad_check=gc), "", "b")
    for g in read:
        s += _on(_conv("h1", "h2", 3, 1, 1, init_wt=init_wt, grad_check=gc), g, g)
    s += extra_edges
    s += _pool("h2", "pool", *pool_window, kind=pool) + _fc("pool", "output", init_wt=init_wt, grad_check=gc)
    return s


def net_a(kinds=RELU, **kw):
    return verification_net(kinds=kinds, **kw)


def net_b(kinds=RELU, **kw):
    return verification_net(h1=(("a", 3), ("b", 7)), kinds=kinds, **kw)


def second_writer():
    """Net A with a second edge into slice ``a`` of h2 (from h1.b): legal, accumulates — and h2 leaves the fused epilogue as a whole."""
    return net_a(extra_edges=_on(_conv("h1", "h2", 3, 1, 1), "b", "a"))


def unread_slice():
    """Net A whose slice ``b`` of h1 nobody reads (h2.b is written from h1.a instead): h1 leaves the fused ComputeDown epilogue as a whole."""
    return net_a(read=("a",), extra_edges=_on(_conv("h1", "h2", 3, 1, 1), "a", "b"))


# Net C.  The group b: C = 128 channels -> F = 192 filters, 3 x 3 stride 1 pad 1 on 13 x 13 pixels at 64 images.
#  * patch_shape_ok: N % 64 == 0, C % 16 == 0 and F % 16 == 0 (the reduction of fprop / dgrad), rows of 13 >= 8 pixels, R > 64 rows
#    (R = F = 192 forward, R = C = 128 backward: one group of three taps on 128-row tiles, i.e. gpw_kernel and not its variant);
#  * wide_plan: tiles = ceil(R / 128) * ceil(169 pixels / 8) = 44 forward and 22 backward, cut into K-ranges until they fill at least
#    60 % of one round of 256 resident blocks;
#  * wgw_try: N % 32 == 0, K = 9 * 128 >= 256, F >= 192, 2 * 169 chunks >= 64.
# Group a (32 -> 64) stays on the narrow kernels beside it.
# Measured on the MI355X with sizes 8, 10, 12, 13, 16: the weight gradient takes wgw_kernel from 8 x 8 on, the forward pass gpw_kernel
# from 10 x 10 on, the input gradient from 13 x 13 on (at 12 x 12 its 18 tiles fill too little of one round): 13 it is.
# Net C pools every map WHOLE (64 x 256 windows per pass in place of 590 000 windows of 3 x 3): a max pool's gradient is discontinuous
# where the two largest inputs of a window tie, and two correct fp32 implementations that sum a unit's 1152 products in different orders
# then route the derivative to different inputs.  tests/test_slices_net_gpu.py asserts the gap of every pass it compares as the
# premise of the comparison (pool_tie_margin); nets A and B (5 x 16 x 8 windows) keep the 3 x 3 stride-2 pool.
WIDE = dict(size=13, c1=(("a", 32), ("b", 128)), c2=(("a", 64), ("b", 192)), batch=64)


def wide_net(kinds=RELU, dropprob=0.0):
    return verification_net(h1=WIDE["c1"], h2=WIDE["c2"], kinds=kinds, dropprob=dropprob, size=WIDE["size"], init_wt=0.5,
                            pool_window=(WIDE["size"], WIDE["size"]))


def inception(kinds=RELU, **kw):
    return models.inception_small(relu=kinds is RELU, **kw)


# ---- the planner's tables of the models that have no slices: tests/golden/layer_plans.json holds them as the commit before layer slices
# planned them (all_plan_tables(), run against that commit's package, wrote the file) ------------------------------------------------
UNSLICED = {
    "alexnet": lambda: models.alexnet(), "alexnet67": lambda: models.alexnet(image_size=67, dropprob=0.0), "alexnet_nin": lambda: models.alexnet_nin(),
    "alexnet_nin_no_dropout": lambda: models.alexnet_nin(image_size=67, dropout=False), "mnist_conv": lambda: models.mnist_conv(),
    "lenet5": lambda: models.lenet5(), "cifar_local": lambda: models.cifar_local(), "vgg": lambda: models.vgg(), "vgg_bn": lambda: models.vgg_bn(),
    "small_bn": lambda: models.small_bn(), "small_bn_linear": lambda: models.small_bn(relu=False), "video_small": lambda: models.video_small(),
    "multilabel_small": lambda: models.multilabel_small(), "multilabel_small_dropout": lambda: models.multilabel_small(dropprob=0.3),
    "softdist_small": lambda: models.softdist_small(), "softdist_small_dropout": lambda: models.softdist_small(dropprob=0.3),
}


def plan_table(text, fused):
    """ConvNet.plan_ as plain data: per layer in topological order [name, the LayerPlan's fields (the output entry by name)], then the
    verdict on the mask pair of every max-pool edge."""
    from convnet_amd.convnet import ConvNet
    from convnet_amd.edge import MaxPoolEdge
    net = ConvNet(text, fused=fused)
    rows = []
    for l in net.layers_:
        p = net.plan_[l]._asdict()
        p["output_entry"] = None if p["output_entry"] is None else p["output_entry"].__name__
        rows.append([l.GetName(), p])
    return {"layers": rows, "pool_masks": [[e.GetName(), bool(e.mask_legal_), bool(e.MaskEligible())] for e in net.edges_ if isinstance(e, MaxPoolEdge)],
            "metric_on_device": bool(net.metric_on_device_)}


def all_plan_tables():
    return {f"{name} {'fused' if fused else 'unfused'}": plan_table(gen(), fused) for name, gen in UNSLICED.items() for fused in (False, True)}


if __name__ == "__main__":
    import json
    import sys
    if "--golden" in sys.argv:
        print(json.dumps(all_plan_tables(), indent=0, sort_keys=True))
