"""Small nets that reach each per-layer choice of ConvNet(fused=True)'s host (the rows of ``convnet.LayerPlan``, the max-pool
mask path of MaxPoolEdge): dropout on pool, conv, 1x1 and rnorm-fed layers, linear layers, refused pool geometries, layers with two
outgoing or two incoming edges.  Inputs <= 35 x 35, channels <= 48.  Used by tests/test_fused_host_configs_{cpu,gpu}.py."""
from convnet_amd import models

L, C, P, R, F, NIN = models._layer, models._conv, models._pool, models._rnorm, models._fc, models._nin
RELU = "RECTIFIED_LINEAR"


def _net(name, body, size=15):
    return models._header(name, seed=7) + L("input", 3, size=size) + body + L("output", 10, "SOFTMAX")


def pool_dropout(dropprob, relu=False):
    """(a)/(b): a max-pool layer (linear, or ReLU) with dropout between two ReLU convs."""
    return _net("pool_dropout", L("c1", 16, RELU) + L("p1", 16, RELU if relu else None, dropprob) + L("c2", 24, RELU)
                + C("input", "c1", 3, 1, 1) + P("c1", "p1", 3, 2) + C("p1", "c2", 3, 1, 1) + F("c2", "output"), size=19)


def conv_dropout_into(kind, dropprob=0.3):
    """(c): a ReLU conv layer with dropout feeding a conv, a 1x1 conv, an FC, a max-pool or an rnorm layer."""
    body = L("c1", 16, RELU, dropprob)
    if kind == "conv":
        body += L("n2", 24, RELU) + C("c1", "n2", 3, 2)
    elif kind == "nin":
        body += L("n2", 24, RELU) + NIN("c1", "n2")
    elif kind == "fc":
        body += L("n2", 32, RELU) + F("c1", "n2")
    elif kind == "maxpool":
        body += L("n2", 16) + P("c1", "n2", 3, 2)
    elif kind == "rnorm":
        body += L("n2", 16, RELU) + R("c1", "n2", 0.05, 0.75, 0.5)
    return _net(f"conv_dropout_{kind}", body + C("input", "c1", 3, 1, 1) + F("n2", "output"))


def rnorm_relu_dropout():
    """(d): ResponseNormCrossMapRelu into a ReLU layer with dropout, whose only outgoing edge is a conv (ConvDownMask at 1/(1-p))."""
    return _net("rnorm_relu_dropout", L("c1", 16, RELU) + L("r1", 16, RELU, 0.5) + L("c2", 24, RELU)
                + C("input", "c1", 3, 1, 1) + R("c1", "r1", 0.05, 0.75, 0.5) + C("r1", "c2", 3, 2) + F("c2", "output"))


def linear_conv_into(kind):
    """(e): a conv layer without activation (ConvUpBiasAct(relu=False), no ReLU' in the epilogue) feeding a max-pool or a conv."""
    body = L("c1", 16)
    if kind == "maxpool":
        body += L("n2", 16) + P("c1", "n2", 3, 2)
    else:
        body += L("n2", 24, RELU) + C("c1", "n2", 3, 2)
    return _net(f"linear_conv_{kind}", body + C("input", "c1", 3, 1, 1) + F("n2", "output"))


def pool_in_net(k, stride, kind="MAXPOOL"):
    """(f): a pool of the given geometry between two ReLU convs."""
    return _net(f"pool_{kind}_{k}s{stride}", L("c1", 16, RELU) + L("p1", 16) + L("c2", 24, RELU)
                + C("input", "c1", 3, 1, 1) + P("c1", "p1", k, stride, kind=kind) + C("p1", "c2", 3, 1, 1) + F("c2", "output"), size=17)


def branches(pool_first=True):
    """(g): c1 (ReLU) has two outgoing edges, a max-pool and a conv (in either order: the second accumulates into c1's derivative,
    ComputeDown(overwrite=False)); both branches end in m, which has two incoming conv edges (ComputeUp accumulates)."""
    pool, conv = P("c1", "p1", 3, 2), C("c1", "c2", 3, 2)
    return _net("branches", L("c1", 16, RELU) + L("p1", 16) + L("c2", 24, RELU) + L("c3", 24, RELU) + L("m", 24, RELU)
                + C("input", "c1", 3, 1, 1) + (pool + conv if pool_first else conv + pool) + C("p1", "c3", 3, 1, 1)
                + C("c2", "m", 1) + C("c3", "m", 1) + F("m", "output"))


def nin_dropout():
    """(h): the reference's network-in-network ImageNet model with its real dropout layers and FC norm limits."""
    return models.alexnet_nin(image_size=67, num_classes=10, dropout=True)


# id -> (model text, batch size)
CONFIGS = {
    "a_linear_pool_dropout": (pool_dropout(0.5), 8),
    "a_linear_pool_control": (pool_dropout(0.0), 8),
    "b_relu_pool_dropout": (pool_dropout(0.5, relu=True), 8),
    "c_into_conv": (conv_dropout_into("conv"), 8),
    "c_into_nin": (conv_dropout_into("nin"), 8),
    "c_into_fc": (conv_dropout_into("fc"), 8),
    "c_into_maxpool": (conv_dropout_into("maxpool"), 8),
    "c_into_rnorm": (conv_dropout_into("rnorm"), 8),
    "d_rnorm_relu_dropout": (rnorm_relu_dropout(), 8),
    "e_linear_into_maxpool": (linear_conv_into("maxpool"), 8),
    "e_linear_into_conv": (linear_conv_into("conv"), 8),
    "f_max3s2_N6": (pool_in_net(3, 2), 6),
    "f_max3s2_N10": (pool_in_net(3, 2), 10),
    "f_max3s2_N8": (pool_in_net(3, 2), 8),
    "f_max2s2": (pool_in_net(2, 2), 8),
    "f_max3s1": (pool_in_net(3, 1), 8),
    "f_avg3s2": (pool_in_net(3, 2, "AVERAGE_POOL"), 8),
    "g_pool_then_conv": (branches(True), 8),
    "g_conv_then_pool": (branches(False), 8),
    "h_alexnet_nin67": (nin_dropout(), 8),
}
