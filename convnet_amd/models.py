"""Model definitions in the reference's pbtxt schema (proto/convnet_config.proto), generated as
text so they can also be written to disk and fed to the reference's own binaries.

* ``alexnet()``    — the AlexNet-class ILSVRC model of examples/imagenet/CLS_net_20140621074703.pbtxt
                     (BASELINE configs[2]/[3]): 224x224x3 -> conv7s2p1/96 -> max3s2p1 -> rnorm ->
                     conv5s2/256 -> max -> rnorm -> conv3p1/384 -> conv3p1/384 -> conv3/256 -> max ->
                     fc4096(drop .4) -> fc4096(drop .4) -> softmax1000; 62,357,608 parameters.
* ``mnist_conv()`` — examples/mnist-conv/net.pbtxt (configs[0]/[1]).
* ``cifar_local()`` — CIFAR-10 "conv + local" (two locally connected layers, LocalEdge).
* ``vgg()``        — a VGG-style stack of 3x3 s1 p1 convs (configs[4]; no such pbtxt exists in the
                     reference).
* ``vgg_bn()``     — the same with batch normalisation on every conv layer.
* ``small_bn()``   — a small batch-normalised net for tests: conv-BN-ReLU, avgpool, conv-BN-ReLU + dropout, FC-BN-ReLU,
                     softmax.
* ``video_small()`` — a small spatio-temporal (3-D) net: 3-D convs, max pooling without and with a time extent, response norm,
                     average pooling over all remaining frames.
* ``multilabel_small()`` — a small multi-label net: conv -> LOGISTIC -> average pool -> FC LOGISTIC -> FC LOGISTIC output of independent
                     yes/no units (CROSS_ENTROPY_BINARY / CLASSIFICATION_BINARY; a negative target means "don't care").
* ``softdist_small()`` — the same trunk with ReLU and a SOFTMAX_DIST output trained on a target distribution per case.
* ``alexnet_grouped()`` — ``alexnet()`` with conv2, conv4 and conv5 as two groups each (the two-tower net of the AlexNet paper), written
                     with layer slices: grouped convolutions.
* ``inception_small()`` — a small net with one module of three branches (1x1, 3x3, 5x5; as a stride-2 reduction module also a pooled
                     fourth) concatenated into one layer through ``dest_slice``.
* ``conv_autoencoder()`` — a convolutional autoencoder: conv / max-pool encoder, conv / ``UPSAMPLE`` decoder, LINEAR output trained with
                     SQUARED_ERROR against a target stream.
* ``skip_sum_small()`` — a small net whose input goes through an ``RGBTOYUV`` edge and in which a coarse branch upsampled by 4 and a
                     1x1 branch sum into one layer.
* ``gaussian_dropout_small()`` — a small net with Gaussian dropout (``gaussian_dropout``, ``max_act_gaussian_dropout``) on a ReLU conv
                     layer, a ReLU FC layer and a LOGISTIC FC layer.
tests/test_models.py checks the first two against the reference's files when they are mounted.
"""

_OPT_W = """  weight_optimizer {{
    epsilon: {eps}
    initial_momentum : 0.5
    final_momentum : {mom}
    momentum_transition_timescale : {tau}
    l2_decay: {l2}{extra}
  }}
  bias_optimizer {{
    epsilon: {eps}
    initial_momentum : 0.5
    final_momentum : {mom}
    momentum_transition_timescale : {tau}
  }}
"""


def _layer(name, channels, activation=None, dropprob=0.0, size=None, extra="", frames=None):
    s = f'layer {{\n  name: "{name}"\n  num_channels: {channels}\n'
    if size:
        s += f"  image_size_y: {size}\n  image_size_x: {size}\n"
    if frames:
        s += f"  image_size_t: {frames}\n"
    if activation:
        s += f"  activation: {activation}\n"
    if dropprob:
        s += f"  dropprob: {dropprob}\n"
    return s + extra + "}\n\n"


def _conv(src, dst, k, stride=1, pad=0, eps=0.01, mom=0.9, tau=2000, l2=0.0005, init_wt=1.0, init_bias=0.0, grad_check=""):
    return (f'edge {{\n  source: "{src}"\n  dest: "{dst}"\n  edge_type: CONVOLUTIONAL\n  kernel_size: {k}\n  stride : {stride}\n'
            f"  padding: {pad}\n  shared_bias: true\n  initialization: DENSE_UNIFORM_SQRT_FAN_IN\n  init_wt: {init_wt}\n"
            f"  init_bias: {init_bias}\n" + _OPT_W.format(eps=eps, mom=mom, tau=tau, l2=l2, extra="") + grad_check + "}\n\n")


def _fc(src, dst, eps=0.01, mom=0.9, tau=2000, l2=0.0005, init_wt=1.0, init_bias=0.0, norm_limit=0.0, grad_check=""):
    extra = f"\n    weight_norm_limit: {norm_limit}" if norm_limit else ""
    return (f'edge {{\n  source: "{src}"\n  dest: "{dst}"\n  edge_type: FC\n  initialization: DENSE_UNIFORM_SQRT_FAN_IN\n'
            f"  init_wt: {init_wt}\n  init_bias: {init_bias}\n" + _OPT_W.format(eps=eps, mom=mom, tau=tau, l2=l2, extra=extra) + grad_check + "}\n\n")


def _nin(src, dst, eps=0.01, mom=0.9, tau=2000, init_wt=1.0, grad_check=""):
    """CONV_ONETOONE (1x1 conv) with the unit-norm row constraint the reference's NIN model uses."""
    return (f'edge {{\n  source: "{src}"\n  dest: "{dst}"\n  edge_type: CONV_ONETOONE\n  initialization: DENSE_UNIFORM_SQRT_FAN_IN\n'
            f"  init_wt: {init_wt}\n" + _OPT_W.format(eps=eps, mom=mom, tau=tau, l2=0.0, extra="\n    weight_norm_constraint: 1") + grad_check + "}\n\n")


def _pool(src, dst, k, stride, pad=0, kind="MAXPOOL"):
    return (f'edge {{\n  source: "{src}"\n  dest: "{dst}"\n  edge_type: {kind}\n  kernel_size: {k}\n  stride : {stride}\n'
            f"  padding: {pad}\n}}\n\n")


def _rnorm(src, dst, add_scale=0.0005, pow_scale=0.75, frac=0.25):
    return (f'edge {{\n  source: "{src}"\n  dest: "{dst}"\n  edge_type: RESPONSE_NORM\n  add_scale: {add_scale}\n'
            f"  pow_scale: {pow_scale}\n  frac_of_filters_response_norm: {frac}\n}}\n\n")


def _header(name, seed=42):
    return f'name: "{name}"\nseed: {seed}\nmax_iter: 10000000\nprint_after: 100\n\n'


def _gc(grad_check, num_params=10):
    if not grad_check:
        return ""
    # several step sizes, largest first: fp32 loss round-off (~ulp(L)/(2 eps batch)) favours large steps, ReLU /
    # max-pool kinks favour small ones; the checker passes an edge if ANY epsilon passes (src/grad_check.cc:60-64)
    return (f"  grad_check: true\n  grad_check_num_params: {num_params}\n  grad_check_epsilon: 0.03\n  grad_check_epsilon: 0.01\n"
            "  grad_check_epsilon: 0.003\n  grad_check_epsilon: 0.001\n")


def alexnet(image_size=224, num_classes=1000, dropprob=0.4, grad_check=False):
    gc = _gc(grad_check)
    s = _header("CLS_net")
    s += _layer("input", 3, size=image_size)
    s += _layer("hidden1_conv", 96, "RECTIFIED_LINEAR") + _layer("hidden1_maxpool", 96) + _layer("hidden1_rnorm", 96, "RECTIFIED_LINEAR")
    s += _layer("hidden2_conv", 256, "RECTIFIED_LINEAR") + _layer("hidden2_maxpool", 256) + _layer("hidden2_rnorm", 256, "RECTIFIED_LINEAR")
    s += _layer("hidden3_conv", 384, "RECTIFIED_LINEAR") + _layer("hidden4_conv", 384, "RECTIFIED_LINEAR")
    s += _layer("hidden5_conv", 256, "RECTIFIED_LINEAR") + _layer("hidden5_maxpool", 256)
    s += _layer("hidden6", 4096, "RECTIFIED_LINEAR", dropprob) + _layer("hidden7", 4096, "RECTIFIED_LINEAR", dropprob)
    s += _layer("output", num_classes, "SOFTMAX")
    s += _conv("input", "hidden1_conv", 7, 2, 1, grad_check=gc)
    s += _pool("hidden1_conv", "hidden1_maxpool", 3, 2, 1) + _rnorm("hidden1_maxpool", "hidden1_rnorm")
    s += _conv("hidden1_rnorm", "hidden2_conv", 5, 2, 0, init_bias=1.0, grad_check=gc)
    s += _pool("hidden2_conv", "hidden2_maxpool", 3, 2, 1) + _rnorm("hidden2_maxpool", "hidden2_rnorm")
    s += _conv("hidden2_rnorm", "hidden3_conv", 3, 1, 1, grad_check=gc)
    s += _conv("hidden3_conv", "hidden4_conv", 3, 1, 1, init_bias=1.0, grad_check=gc)
    s += _conv("hidden4_conv", "hidden5_conv", 3, 1, 0, init_bias=1.0, grad_check=gc)
    s += _pool("hidden5_conv", "hidden5_maxpool", 3, 2, 1)
    s += _fc("hidden5_maxpool", "hidden6", norm_limit=4, grad_check=gc) + _fc("hidden6", "hidden7", norm_limit=4, grad_check=gc)
    s += _fc("hidden7", "output", norm_limit=4, grad_check=gc)
    return s


def alexnet_nin(image_size=224, num_classes=1000, grad_check=False, dropout=True):
    """examples/imagenet/CLS_net_20140801232522.pbtxt: the network-in-network variant — 1x1
    CONV_ONETOONE layers after conv2..conv5, 512-channel conv5, dropout 0.1/0.3/0.5."""
    gc = _gc(grad_check)
    R = "RECTIFIED_LINEAR"
    d = (lambda p: p) if dropout else (lambda p: 0.0)
    s = _header("CLS_net", seed=80638)
    s += _layer("input", 3, size=image_size)
    s += _layer("hidden1_conv", 96, R) + _layer("hidden1_maxpool", 96) + _layer("hidden1_rnorm", 96, R)
    s += _layer("hidden2_conv", 256, R) + _layer("hidden2_conv_nin1", 256, R) + _layer("hidden2_maxpool", 256) + _layer("hidden2_rnorm", 256, R)
    s += _layer("hidden3_conv", 384, R) + _layer("hidden3_conv_nin1", 768, R)
    s += _layer("hidden4_conv", 384, R) + _layer("hidden4_conv_nin1", 768, R, d(0.1)) + _layer("hidden4_conv_nin2", 384, R)
    s += _layer("hidden5_conv", 512, R) + _layer("hidden5_conv_nin1", 1024, R, d(0.3)) + _layer("hidden5_conv_nin2", 512, R)
    s += _layer("hidden5_maxpool", 512)
    s += _layer("hidden6", 4096, R, d(0.5)) + _layer("hidden7", 4096, R, d(0.5)) + _layer("output", num_classes, "SOFTMAX")
    s += _conv("input", "hidden1_conv", 7, 2, 1, l2=0.0, grad_check=gc)
    s += _pool("hidden1_conv", "hidden1_maxpool", 3, 2, 1) + _rnorm("hidden1_maxpool", "hidden1_rnorm")
    s += _conv("hidden1_rnorm", "hidden2_conv", 5, 2, 1, l2=0.0, init_bias=1.0, grad_check=gc) + _nin("hidden2_conv", "hidden2_conv_nin1", grad_check=gc)
    s += _pool("hidden2_conv_nin1", "hidden2_maxpool", 3, 2, 1) + _rnorm("hidden2_maxpool", "hidden2_rnorm")
    s += _conv("hidden2_rnorm", "hidden3_conv", 3, 1, 1, grad_check=gc) + _nin("hidden3_conv", "hidden3_conv_nin1", grad_check=gc)
    s += _conv("hidden3_conv_nin1", "hidden4_conv", 3, 1, 1, init_bias=1.0, grad_check=gc)
    s += _nin("hidden4_conv", "hidden4_conv_nin1", grad_check=gc) + _nin("hidden4_conv_nin1", "hidden4_conv_nin2", grad_check=gc)
    s += _conv("hidden4_conv_nin2", "hidden5_conv", 3, 1, 0, init_bias=1.0, grad_check=gc)
    s += _nin("hidden5_conv", "hidden5_conv_nin1", grad_check=gc) + _nin("hidden5_conv_nin1", "hidden5_conv_nin2", grad_check=gc)
    s += _pool("hidden5_conv_nin2", "hidden5_maxpool", 3, 2, 1)
    s += _fc("hidden5_maxpool", "hidden6", norm_limit=4, grad_check=gc) + _fc("hidden6", "hidden7", norm_limit=4, grad_check=gc)
    s += _fc("hidden7", "output", init_wt=0.1, norm_limit=4, grad_check=gc)
    return s


def mnist_conv(grad_check=False, image_size=28):
    gc = _gc(grad_check)
    s = _header("mnist_conv")
    s += _layer("input", 1, size=image_size)
    s += _layer("hidden1_conv", 48, "RECTIFIED_LINEAR") + _layer("hidden1_maxpool", 48)
    s += _layer("hidden2_conv", 128, "RECTIFIED_LINEAR") + _layer("hidden2_maxpool", 128)
    s += _layer("output", 10, "SOFTMAX")
    s += _conv("input", "hidden1_conv", 4, mom=0.95, tau=0, grad_check=gc) + _pool("hidden1_conv", "hidden1_maxpool", 4, 2)
    s += _conv("hidden1_maxpool", "hidden2_conv", 4, mom=0.95, tau=0, init_bias=1.0, grad_check=gc) + _pool("hidden2_conv", "hidden2_maxpool", 4, 2)
    s += _fc("hidden2_maxpool", "output", mom=0.95, tau=0, norm_limit=4, grad_check=gc)
    return s


def lenet5(grad_check=False):
    """LeNet-5-class net in the same schema (BASELINE configs[1]); average pooling exercises AvgPoolEdge."""
    gc = _gc(grad_check)
    s = _header("lenet5")
    s += _layer("input", 1, size=28)
    s += _layer("c1", 6, "RECTIFIED_LINEAR") + _layer("s2", 6) + _layer("c3", 16, "RECTIFIED_LINEAR") + _layer("s4", 16)
    s += _layer("f5", 120, "RECTIFIED_LINEAR") + _layer("f6", 84, "RECTIFIED_LINEAR") + _layer("output", 10, "SOFTMAX")
    s += _conv("input", "c1", 5, 1, 2, grad_check=gc) + _pool("c1", "s2", 2, 2, kind="AVERAGE_POOL")
    s += _conv("s2", "c3", 5, grad_check=gc) + _pool("c3", "s4", 2, 2, kind="MAXPOOL")
    s += _fc("s4", "f5", grad_check=gc) + _fc("f5", "f6", grad_check=gc) + _fc("f6", "output", grad_check=gc)
    return s


def _local(src, dst, k, stride=1, pad=0, eps=0.01, mom=0.9, tau=2000, l2=0.0005, init_wt=1.0, init_bias=0.0, grad_check=""):
    """LOCAL (locally connected) edge: a conv geometry with one filter bank per module and one bias per (filter, module)."""
    return (f'edge {{\n  source: "{src}"\n  dest: "{dst}"\n  edge_type: LOCAL\n  kernel_size: {k}\n  stride : {stride}\n'
            f"  padding: {pad}\n  initialization: DENSE_UNIFORM_SQRT_FAN_IN\n  init_wt: {init_wt}\n"
            f"  init_bias: {init_bias}\n" + _OPT_W.format(eps=eps, mom=mom, tau=tau, l2=l2, extra="") + grad_check + "}\n\n")


def cifar_local(num_classes=10, grad_check=False):
    """CIFAR-10 after cuda-convnet's "conv + local" model (layers-conv-local): 24x24x3 crops -> conv5p2/64 -> max3s2 -> rnorm ->
    conv5p2/64 -> rnorm -> max3s2 -> local3p1/64 -> local3p1/32 -> fc10 -> softmax.  With this code base's pooling arithmetic
    ((size - 3) // 2 + 1) the images are 24 -> 11 -> 5, so both local layers run on 5x5 modules: 64 and 32 filters of 3x3x64."""
    gc = _gc(grad_check)
    R = "RECTIFIED_LINEAR"
    s = _header("cifar_local")
    s += _layer("input", 3, size=24)
    s += _layer("conv1", 64, R) + _layer("pool1", 64) + _layer("rnorm1", 64)
    s += _layer("conv2", 64, R) + _layer("rnorm2", 64) + _layer("pool2", 64)
    s += _layer("local3", 64, R) + _layer("local4", 32, R) + _layer("output", num_classes, "SOFTMAX")
    s += _conv("input", "conv1", 5, 1, 2, grad_check=gc) + _pool("conv1", "pool1", 3, 2) + _rnorm("pool1", "rnorm1")
    s += _conv("rnorm1", "conv2", 5, 1, 2, init_bias=1.0, grad_check=gc) + _rnorm("conv2", "rnorm2") + _pool("rnorm2", "pool2", 3, 2)
    s += _local("pool2", "local3", 3, 1, 1, grad_check=gc) + _local("local3", "local4", 3, 1, 1, grad_check=gc)
    s += _fc("local4", "output", grad_check=gc)
    return s


def vgg(image_size=224, num_classes=1000, widths=(64, 128, 256, 512, 512), depths=(2, 2, 3, 3, 3), dropprob=0.5):
    s = _header("vgg_style")
    s += _layer("input", 3, size=image_size)
    edges, prev = "", "input"
    for b, (w, d) in enumerate(zip(widths, depths), 1):
        for i in range(1, d + 1):
            name = f"conv{b}_{i}"
            s += _layer(name, w, "RECTIFIED_LINEAR")
            edges += _conv(prev, name, 3, 1, 1)
            prev = name
        s += _layer(f"pool{b}", w)
        edges += _pool(prev, f"pool{b}", 2, 2)
        prev = f"pool{b}"
    s += _layer("fc6", 4096, "RECTIFIED_LINEAR", dropprob) + _layer("fc7", 4096, "RECTIFIED_LINEAR", dropprob)
    s += _layer("output", num_classes, "SOFTMAX")
    edges += _fc(prev, "fc6") + _fc("fc6", "fc7") + _fc("fc7", "output")
    return s + edges


_BN = "  batch_normalize: true\n"
# gamma runs the default WEIGHT optimizer, beta the default BIAS optimizer (src/convnet.cc:56-64)
_BN_DEFAULTS = "".join(f"""{kind} {{
  epsilon: 0.01
  initial_momentum : 0.5
  final_momentum : 0.9
  momentum_transition_timescale : 2000
}}
""" for kind in ("default_weight_optimizer", "default_bias_optimizer")) + "\n"


def vgg_bn(image_size=224, num_classes=1000, widths=(64, 128, 256, 512, 512), depths=(2, 2, 3, 3, 3), dropprob=0.5):
    """vgg() with batch normalisation (batch_normalize: true) on all 13 conv layers, the standard way to train VGG-16."""
    s = _header("vgg_bn") + _BN_DEFAULTS
    s += _layer("input", 3, size=image_size)
    edges, prev = "", "input"
    for b, (w, d) in enumerate(zip(widths, depths), 1):
        for i in range(1, d + 1):
            name = f"conv{b}_{i}"
            s += _layer(name, w, "RECTIFIED_LINEAR", extra=_BN)
            edges += _conv(prev, name, 3, 1, 1)
            prev = name
        s += _layer(f"pool{b}", w)
        edges += _pool(prev, f"pool{b}", 2, 2)
        prev = f"pool{b}"
    s += _layer("fc6", 4096, "RECTIFIED_LINEAR", dropprob) + _layer("fc7", 4096, "RECTIFIED_LINEAR", dropprob)
    s += _layer("output", num_classes, "SOFTMAX")
    edges += _fc(prev, "fc6") + _fc("fc6", "fc7") + _fc("fc7", "output")
    return s + edges


def small_bn(image_size=12, num_classes=10, dropprob=0.25, bn_f=0.9, relu=True):
    """A small batch-normalised net for tests: conv-BN-ReLU, avgpool, conv-BN-ReLU + dropout, FC-BN-ReLU, softmax.  relu=False makes
    the three BN layers LINEAR."""
    act = "RECTIFIED_LINEAR" if relu else "LINEAR"
    bn = _BN + f"  bn_f: {bn_f}\n"
    s = _header("small_bn") + _BN_DEFAULTS
    s += _layer("input", 3, size=image_size)
    s += _layer("conv1", 16, act, extra=bn) + _layer("pool1", 16)
    s += _layer("conv2", 24, act, dropprob, extra=bn) + _layer("fc3", 32, act, extra=bn)
    s += _layer("output", num_classes, "SOFTMAX")
    s += _conv("input", "conv1", 3, 1, 1, init_wt=0.3) + _pool("conv1", "pool1", 2, 2, kind="AVERAGE_POOL")
    s += _conv("pool1", "conv2", 3, 1, 1, init_wt=0.3) + _fc("conv2", "fc3", init_wt=0.3) + _fc("fc3", "output", init_wt=0.3)
    return s


def _time(edge, kt=None, st=None):
    """The same edge with kernel_size_t / stride_t added (a 3-D convolution, or pooling boxes over time)."""
    extra = (f"  kernel_size_t: {kt}\n" if kt is not None else "") + (f"  stride_t: {st}\n" if st is not None else "")
    head, sep, tail = edge.rpartition("}")
    return head + extra + sep + tail


def video_small(image_size=32, frames=16, num_classes=10, grad_check=False, init_wt=1.0):
    """A small video net with every edge type that takes clips: 3 x 32 x 32 x T16 -> conv 3x3x3/64 -> max-pool 3x3x1 s2 (frames are
    channels) -> conv 3x3x3/128 -> max-pool 3x3x2 s2, over time too -> rnorm -> conv 3x3x3/128 -> avg-pool over all remaining frames ->
    FC -> softmax.  Sizes: 32x32xT16 -> 32x32xT14 -> 15x15xT14 -> 15x15xT12 -> 7x7xT6 -> 7x7xT4 -> 1x1xT1."""
    gc = _gc(grad_check)
    R = "RECTIFIED_LINEAR"
    s = _header("video_small")
    s += _layer("input", 3, size=image_size, frames=frames)
    s += _layer("conv1", 64, R) + _layer("pool1", 64) + _layer("conv2", 128, R) + _layer("pool2", 128) + _layer("rnorm2", 128)
    s += _layer("conv3", 128, R) + _layer("pool3", 128) + _layer("output", num_classes, "SOFTMAX")
    s += _time(_conv("input", "conv1", 3, 1, 1, init_wt=init_wt, grad_check=gc), kt=3) + _pool("conv1", "pool1", 3, 2)
    s += _time(_conv("pool1", "conv2", 3, 1, 1, init_wt=init_wt, init_bias=1.0, grad_check=gc), kt=3)
    s += _time(_pool("conv2", "pool2", 3, 2), kt=2, st=2) + _rnorm("pool2", "rnorm2")
    s += _time(_conv("rnorm2", "conv3", 3, 1, 1, init_wt=init_wt, grad_check=gc), kt=3)
    s += _time(_pool("conv3", "pool3", 0, 1, kind="AVERAGE_POOL"), kt=0)   # kernel sizes <= 0: the whole map, all frames (maxpool_edge.cc:13-25)
    s += _fc("pool3", "output", init_wt=init_wt, grad_check=gc)
    return s


def _small_head_trunk(name, act, dropprob, image_size, output, init_wt, gc):
    s = _header(name)
    s += _layer("input", 3, size=image_size)
    s += _layer("conv1", 16, act, dropprob) + _layer("pool1", 16) + _layer("fc2", 32, act, dropprob) + output
    s += _conv("input", "conv1", 3, 1, 1, init_wt=init_wt, grad_check=gc) + _pool("conv1", "pool1", 3, 2, kind="AVERAGE_POOL")
    s += _fc("pool1", "fc2", init_wt=init_wt, grad_check=gc) + _fc("fc2", "output", init_wt=init_wt, grad_check=gc)
    return s


def multilabel_small(image_size=12, num_labels=2, dropprob=0.0, grad_check=False):
    """A small multi-label net: conv3p1/16 LOGISTIC -> avg3s2 -> fc32 LOGISTIC -> fc LOGISTIC output with ``num_labels`` independent
    yes/no units, trained with CROSS_ENTROPY_BINARY and scored with CLASSIFICATION_BINARY (the share of a case's counted labels that
    are right; a negative target is not counted).  ``dropprob``: dropout on the two logistic hidden layers.
    Sigmoid units with average pooling (the LeNet pairing) make the whole net smooth, and init_wt = 3 keeps the two y (1 - y) <= 1/4
    factors of the backward pass from shrinking conv1's gradients to the fp32 difference-quotient quantum ulp(loss) / (2 eps batch)
    ~ 1e-6: a grad_check of this net measures the gradients, not the rounding of the loss."""
    out = _layer("output", num_labels, "LOGISTIC", extra="  loss_function: CROSS_ENTROPY_BINARY\n  performance_metric: CLASSIFICATION_BINARY\n")
    return _small_head_trunk("multilabel_small", "LOGISTIC", dropprob, image_size, out, 3.0, _gc(grad_check, 6))


def softdist_small(image_size=12, num_classes=10, dropprob=0.0, grad_check=False):
    """multilabel_small's trunk with ReLU layers and a SOFTMAX_DIST output: the target is a distribution over ``num_classes`` per case
    (soft labels, distillation); CROSS_ENTROPY_MULTINOMIAL_DISTRIBUTED is both the loss and the reported metric."""
    out = _layer("output", num_classes, "SOFTMAX_DIST", extra="  loss_function: CROSS_ENTROPY_MULTINOMIAL_DISTRIBUTED\n"
                 "  performance_metric: CROSS_ENTROPY_MULTINOMIAL_DISTRIBUTED\n")
    return _small_head_trunk("softdist_small", "RECTIFIED_LINEAR", dropprob, image_size, out, 1.0, _gc(grad_check, 6))


def _gaussian(stddev, max_act=None):
    """``extra`` of _layer for Gaussian dropout; the standard deviation itself is the layer's ``dropprob``."""
    return "  gaussian_dropout: true\n" + (f"  max_act_gaussian_dropout: {max_act}\n" if max_act is not None else "")


def gaussian_dropout_small(image_size=12, num_classes=10, relu=True, pool="MAXPOOL", batch_normalize=False):
    """A small net with multiplicative Gaussian noise N(1, dropprob^2) on three hidden layers: conv3p1/16 ReLU (0.3) -> max3s2 ->
    fc32 ReLU (0.5, clipped to |x| <= 10 by ``max_act_gaussian_dropout``) -> fc24 LOGISTIC (0.2) -> softmax.  Every noised layer has
    one conv or FC edge in with a shared bias, so the fused host's bias / ReLU epilogues apply in front of the noise.  ``relu=False``
    makes the first two LINEAR, ``pool`` can be AVERAGE_POOL, ``batch_normalize`` batch-normalises conv1."""
    act = "RECTIFIED_LINEAR" if relu else "LINEAR"
    s = _header("gaussian_dropout_small") + (_BN_DEFAULTS if batch_normalize else "")
    s += _layer("input", 3, size=image_size)
    s += _layer("conv1", 16, act, 0.3, extra=_gaussian(0.3) + (_BN if batch_normalize else "")) + _layer("pool1", 16)
    s += _layer("fc2", 32, act, 0.5, extra=_gaussian(0.5, 10)) + _layer("fc3", 24, "LOGISTIC", 0.2, extra=_gaussian(0.2))
    s += _layer("output", num_classes, "SOFTMAX")
    s += _conv("input", "conv1", 3, 1, 1) + _pool("conv1", "pool1", 3, 2, kind=pool)
    s += _fc("pool1", "fc2") + _fc("fc2", "fc3") + _fc("fc3", "output")
    return s


def _slices(**channels):
    """The layer_slice blocks of a layer (``extra`` of _layer; the layer's own num_channels is then 0): name=channels."""
    return "".join(f'  layer_slice {{\n    name: "{n}"\n    num_channels: {c}\n  }}\n' for n, c in channels.items())


def _on(edge, source_slice="", dest_slice=""):
    """The same edge reading ``source_slice`` of its source layer and / or writing ``dest_slice`` of its destination."""
    extra = (f'  source_slice: "{source_slice}"\n' if source_slice else "") + (f'  dest_slice: "{dest_slice}"\n' if dest_slice else "")
    head, sep, tail = edge.rpartition("}")
    return head + extra + sep + tail


def alexnet_grouped(image_size=224, num_classes=1000, dropprob=0.4, grad_check=False):
    """alexnet() with conv2, conv4 and conv5 in two groups each, as the two GPUs of the AlexNet paper had them: each half of the filters
    sees half of the input channels (48 -> 128, 192 -> 192, 192 -> 128 per group).  A layer that feeds a grouped convolution is written
    whole and read by slice ``a`` / ``b`` (hidden1_rnorm, hidden3_conv); a grouped layer is written by slice and read whole by its pool
    or, by slice again, by the next group (hidden4_conv).  60,944,488 parameters (alexnet(): 62,357,608)."""
    gc = _gc(grad_check)
    R = "RECTIFIED_LINEAR"
    s = _header("CLS_net_grouped")
    s += _layer("input", 3, size=image_size)
    s += _layer("hidden1_conv", 96, R) + _layer("hidden1_maxpool", 96) + _layer("hidden1_rnorm", 0, R, extra=_slices(a=48, b=48))
    s += _layer("hidden2_conv", 0, R, extra=_slices(a=128, b=128)) + _layer("hidden2_maxpool", 256) + _layer("hidden2_rnorm", 256, R)
    s += _layer("hidden3_conv", 0, R, extra=_slices(a=192, b=192)) + _layer("hidden4_conv", 0, R, extra=_slices(a=192, b=192))
    s += _layer("hidden5_conv", 0, R, extra=_slices(a=128, b=128)) + _layer("hidden5_maxpool", 256)
    s += _layer("hidden6", 4096, R, dropprob) + _layer("hidden7", 4096, R, dropprob)
    s += _layer("output", num_classes, "SOFTMAX")
    s += _conv("input", "hidden1_conv", 7, 2, 1, grad_check=gc)
    s += _pool("hidden1_conv", "hidden1_maxpool", 3, 2, 1) + _rnorm("hidden1_maxpool", "hidden1_rnorm")
    for g in "ab":
        s += _on(_conv("hidden1_rnorm", "hidden2_conv", 5, 2, 0, init_bias=1.0, grad_check=gc), g, g)
    s += _pool("hidden2_conv", "hidden2_maxpool", 3, 2, 1) + _rnorm("hidden2_maxpool", "hidden2_rnorm")
    for g in "ab":   # conv3 sees every channel: one edge per half of ITS filters, so that conv4's groups read slices
        s += _on(_conv("hidden2_rnorm", "hidden3_conv", 3, 1, 1, grad_check=gc), "", g)
    for g in "ab":
        s += _on(_conv("hidden3_conv", "hidden4_conv", 3, 1, 1, init_bias=1.0, grad_check=gc), g, g)
    for g in "ab":
        s += _on(_conv("hidden4_conv", "hidden5_conv", 3, 1, 0, init_bias=1.0, grad_check=gc), g, g)
    s += _pool("hidden5_conv", "hidden5_maxpool", 3, 2, 1)
    s += _fc("hidden5_maxpool", "hidden6", norm_limit=4, grad_check=gc) + _fc("hidden6", "hidden7", norm_limit=4, grad_check=gc)
    s += _fc("hidden7", "output", norm_limit=4, grad_check=gc)
    return s


def inception_small(image_size=12, num_classes=10, relu=True, pooled_branch=False, dropprob=0.0, grad_check=False, init_wt=1.0):
    """A small net with one inception-style module: conv3p1/8 ``stem`` -> {1x1 CONV_ONETOONE / 6, 3x3 p1 / 10, 5x5 p2 / 5} concatenated
    into one layer ``mix`` (slices ``b1x1``, ``b3x3``, ``b5x5``: every branch writes its own) -> 3x3 s2 pool -> FC softmax.
    pooled_branch=True makes it a reduction module: the 3x3 and 5x5 branches run at stride 2, a 3x3 s2 p1 pooling edge writes the
    stem's 8 channels straight into a fourth slice ``pool``, and the 1x1 branch reads a pooled copy of the stem (``stem_pool``).
    relu=False: LINEAR layers and average pooling (a smooth net, for grad checks)."""
    gc = _gc(grad_check, 6)
    act, kind = ("RECTIFIED_LINEAR", "MAXPOOL") if relu else ("LINEAR", "AVERAGE_POOL")
    widths = dict(b1x1=6, b3x3=10, b5x5=5)
    stride = 1
    if pooled_branch:
        widths["pool"] = 8
        stride = 2
    s = _header("inception_small")
    s += _layer("input", 3, size=image_size)
    s += _layer("stem", 8, act) + (_layer("stem_pool", 8) if pooled_branch else "")
    s += _layer("mix", 0, act, dropprob, extra=_slices(**widths)) + _layer("pool", sum(widths.values()))
    s += _layer("output", num_classes, "SOFTMAX")
    s += _conv("input", "stem", 3, 1, 1, init_wt=init_wt, grad_check=gc)
    if pooled_branch:
        s += _pool("stem", "stem_pool", 3, 2, 1, kind=kind)
    s += _on(_nin("stem_pool" if pooled_branch else "stem", "mix", init_wt=init_wt, grad_check=gc), "", "b1x1")
    s += _on(_conv("stem", "mix", 3, stride, 1, init_wt=init_wt, grad_check=gc), "", "b3x3")
    s += _on(_conv("stem", "mix", 5, stride, 2, init_wt=init_wt, grad_check=gc), "", "b5x5")
    if pooled_branch:
        s += _on(_pool("stem", "mix", 3, 2, 1, kind=kind), "", "pool")
    s += _pool("mix", "pool", 3, 2, kind=kind) + _fc("pool", "output", init_wt=init_wt, grad_check=gc)
    return s


def _upsample(src, dst, factor):
    return f'edge {{\n  source: "{src}"\n  dest: "{dst}"\n  edge_type: UPSAMPLE\n  sample_factor: {factor}\n}}\n\n'


_SQUARED_ERROR = "  loss_function: SQUARED_ERROR\n  performance_metric: SQUARED_ERROR\n"


def conv_autoencoder(image_size=32, grad_check=False, init_wt=1.0, relu=True, eps=0.0001):
    """A convolutional autoencoder: 3 x S x S -> conv3p1/16 ReLU -> max2s2 -> conv3p1/32 ReLU -> max2s2 (S/4) -> conv3p1/32 -> UPSAMPLE 2
    -> conv3p1/16 ReLU -> UPSAMPLE 2 -> conv3p1 into a LINEAR output of 3 x S x S trained with SQUARED_ERROR against a target stream of
    its own (the image, for an autoencoder).  The loss is summed over the 3 x S x S outputs, hence the small learning rate ``eps`` (at 0.01
    the net diverges within three steps).  ``image_size`` must be a multiple of 4.  relu=False: LINEAR layers and average pooling (a
    smooth net, for grad checks)."""
    gc = _gc(grad_check, 6)
    R, kind = ("RECTIFIED_LINEAR", "MAXPOOL") if relu else ("LINEAR", "AVERAGE_POOL")
    s = _header("conv_autoencoder")
    s += _layer("input", 3, size=image_size)
    s += _layer("enc1", 16, R) + _layer("pool1", 16) + _layer("enc2", 32, R) + _layer("pool2", 32)
    s += _layer("dec1", 32) + _layer("up1", 32) + _layer("dec2", 16, R) + _layer("up2", 16)
    s += _layer("output", 3, "LINEAR", extra=_SQUARED_ERROR)
    s += _conv("input", "enc1", 3, 1, 1, init_wt=init_wt, eps=eps, grad_check=gc) + _pool("enc1", "pool1", 2, 2, kind=kind)
    s += _conv("pool1", "enc2", 3, 1, 1, init_wt=init_wt, eps=eps, grad_check=gc) + _pool("enc2", "pool2", 2, 2, kind=kind)
    s += _conv("pool2", "dec1", 3, 1, 1, init_wt=init_wt, eps=eps, grad_check=gc) + _upsample("dec1", "up1", 2)
    s += _conv("up1", "dec2", 3, 1, 1, init_wt=init_wt, eps=eps, grad_check=gc) + _upsample("dec2", "up2", 2)
    s += _conv("up2", "output", 3, 1, 1, init_wt=init_wt, eps=eps, grad_check=gc)
    return s


def skip_sum_small(image_size=16, num_classes=10, colour=True, grad_check=False, init_wt=1.0, relu=True):
    """A small net with a skip sum: the input goes through an RGBTOYUV edge (``colour``; False feeds the stem from the input directly),
    conv3p1/8 ReLU ``stem``; a coarse branch (avg4s4 -> conv3p1/6 -> UPSAMPLE 4) and a fine 1x1 branch (CONV_ONETOONE / 6) both write the
    ReLU layer ``sum`` — the 1x1 edge first, so the upsampled map is ADDED to it — then avg4s4 -> FC softmax.  ``image_size`` must be
    a multiple of 4.  relu=False: LINEAR layers (a smooth net, for grad checks)."""
    gc = _gc(grad_check, 6)
    R = "RECTIFIED_LINEAR" if relu else "LINEAR"
    s = _header("skip_sum_small")
    s += _layer("input", 3, size=image_size) + (_layer("yuv", 3) if colour else "")
    s += _layer("stem", 8, R) + _layer("pool", 8) + _layer("coarse", 6) + _layer("sum", 6, R)
    s += _layer("pool2", 6) + _layer("output", num_classes, "SOFTMAX")
    if colour:
        s += 'edge {\n  source: "input"\n  dest: "yuv"\n  edge_type: RGBTOYUV\n}\n\n'
    s += _conv("yuv" if colour else "input", "stem", 3, 1, 1, init_wt=init_wt, grad_check=gc)
    s += _pool("stem", "pool", 4, 4, kind="AVERAGE_POOL") + _conv("pool", "coarse", 3, 1, 1, init_wt=init_wt, grad_check=gc)
    s += _nin("stem", "sum", init_wt=init_wt, grad_check=gc) + _upsample("coarse", "sum", 4)
    s += _pool("sum", "pool2", 4, 4, kind="AVERAGE_POOL") + _fc("pool2", "output", init_wt=init_wt, grad_check=gc)
    return s


# forward MACs per image of a built net (for roofline accounting): see bench.py
def count_macs(net):
    """(fwd_macs, train_macs) per image following BASELINE.md §2: train = fwd + wgrad (all weighted
    edges) + dgrad (all but edges whose source is an input layer, src/convnet.cc:370)."""
    from .edge import ConvEdge, ConvOneToOneEdge, FCEdge, LocalEdge
    fwd = train = 0
    for e in net.edges_:
        if isinstance(e, (ConvEdge, LocalEdge)):
            d = e.conv_desc_
            macs = e.num_modules_y_ * e.num_modules_x_ * d.num_output_channels * d.kernel_size_y * d.kernel_size_x * d.num_input_channels
            if isinstance(e, ConvEdge):   # a 3-D convolution: Kt taps in each of Mt output frames
                macs *= max(1, d.kernel_size_t) * e.num_modules_t_
        elif isinstance(e, ConvOneToOneEdge):     # 1x1 conv: C x F per pixel
            macs = e.num_modules_y_ * e.num_modules_x_ * e.num_input_channels_ * e.num_output_channels_
        elif isinstance(e, FCEdge):
            macs = e._input_size() * e.num_output_channels_
        else:
            continue
        fwd += macs
        train += 2 * macs + (0 if e.GetSource().IsInput() or e.IsBackPropBlocked() else macs)
    return fwd, train
