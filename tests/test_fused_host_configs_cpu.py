"""CPU: the host's choice of the max-pool mask path, and the whole-net oracle's DAG extension pinned to float64 torch autograd.
 * The mask pair (MaxPoolMask / MaxPoolUndoMask) is legal only where backprop sees the raw window maxima: the pool layer has no
   dropout and a linear or ReLU activation.  AlexNet, VGG and the NIN model keep it (the benchmark's path); a pool layer with dropout
   does not.
 * tests/oracle_net.forward_backward on a net with a two-outgoing-edge layer and a two-incoming-edge layer gives the same parameter
   gradients as float64 autograd from the same parameters and input."""
import numpy as np
import pytest

from convnet_amd import models
from convnet_amd.convnet import ConvNet
from convnet_amd.edge import ConvEdge, FCEdge, MaxPoolEdge

import fused_host_nets as nets
from golden_cases import rel_err


def _pools(text):
    return [e for e in ConvNet(text, fused=True).edges_ if isinstance(e, MaxPoolEdge)]


@pytest.mark.parametrize("gen", [models.alexnet, models.vgg, models.alexnet_nin])
def test_reference_models_keep_the_pool_mask_path(gen):
    pools = _pools(gen())
    assert pools and all(e.MaskEligible() for e in pools), [e.GetName() for e in pools if not e.MaskEligible()]


def test_pool_layer_with_dropout_takes_the_reference_undo():
    assert not any(e.MaskEligible() for e in _pools(nets.pool_dropout(0.5)))                # row (a): linear pool layer, dropout
    assert not any(e.MaskEligible() for e in _pools(nets.pool_dropout(0.5, relu=True)))     # row (b): ReLU pool layer, dropout
    assert all(e.MaskEligible() for e in _pools(nets.pool_dropout(0.0)))                    # the control keeps the mask
    assert all(e.MaskEligible() for e in _pools(nets.pool_dropout(0.0, relu=True)))
    assert not any(e.MaskEligible() for e in ConvNet(nets.pool_dropout(0.0), fused=False).edges_ if isinstance(e, MaxPoolEdge))


class _Host:
    def __init__(self, a):
        self.a = np.ascontiguousarray(a, np.float32)

    def ToNumpy(self):
        return self.a


def test_oracle_net_dag_gradients_match_float64_autograd():
    """Branching net, dropout off: c1 feeds a max-pool and a conv; m sums two conv edges.  Continuous random data, so pool ties and
    ReLU kinks at exactly 0 do not occur."""
    import torch
    import torch.nn.functional as tf
    from oracle_net import forward_backward
    net = ConvNet(nets.branches(pool_first=True))
    N = 4
    rng = np.random.default_rng(3)
    params = {}
    for e in net.edges_:
        if isinstance(e, ConvEdge):
            d, C = e.conv_desc_, e.GetSource().GetNumChannels()
            w = rng.standard_normal((C, d.kernel_size_y, d.kernel_size_x, d.num_output_channels)) / np.sqrt(C * d.kernel_size_y * d.kernel_size_x)
            b = 0.1 * rng.standard_normal(d.num_output_channels)
        elif isinstance(e, FCEdge):
            src = e.GetSource()
            D = src.GetNumChannels() * src.GetSizeY() * src.GetSizeX()
            w, b = rng.standard_normal((D, e.GetDest().GetNumChannels())) / np.sqrt(D), 0.1 * rng.standard_normal(e.GetDest().GetNumChannels())
        else:
            continue
        w, b = w.astype(np.float32), b.astype(np.float32)
        params[e.GetName()] = (w, b)
        e.GetWeight = (lambda a: lambda: _Host(a))(w.reshape(-1) if isinstance(e, ConvEdge) else w)
        e.GetBias = (lambda a: lambda: _Host(a))(b)
    inp = net.input_layers_[0]
    x = rng.standard_normal((3, inp.GetSizeY(), inp.GetSizeX(), N)).astype(np.float32)
    labels = rng.integers(0, 10, N).astype(np.float32)
    _, _, grads = forward_backward(net, x, labels)

    # the same net in float64 autograd (NCHW; reference layouts: activations (C, H, W, N), filters (C, Ky, Kx, F))
    T = {k: (torch.tensor(w, dtype=torch.float64, requires_grad=True), torch.tensor(b, dtype=torch.float64, requires_grad=True))
         for k, (w, b) in params.items()}

    def conv(name, a):
        e = net.GetEdgeByName(name)
        d = e.conv_desc_
        w, b = T[name]
        return tf.conv2d(a, w.permute(3, 0, 1, 2), b, stride=(d.stride_y, d.stride_x), padding=(-d.padding_y, -d.padding_x))

    X = torch.tensor(x, dtype=torch.float64).permute(3, 0, 1, 2)
    c1 = torch.relu(conv("input:c1", X))
    pe = net.GetEdgeByName("c1:p1").conv_desc_
    p1 = tf.max_pool2d(c1, (pe.kernel_size_y, pe.kernel_size_x), (pe.stride_y, pe.stride_x))
    c2 = torch.relu(conv("c1:c2", c1))
    c3 = torch.relu(conv("p1:c3", p1))
    m = torch.relu(conv("c2:m", c2) + conv("c3:m", c3))
    w, b = T["m:output"]
    logits = m.reshape(N, -1) @ w + b
    loss = tf.cross_entropy(logits, torch.tensor(labels, dtype=torch.long), reduction="sum") / N
    loss.backward()
    assert set(grads) == set(T)
    for name, (w, b) in T.items():
        dw = w.grad.numpy()
        assert rel_err(grads[name][0], dw.reshape(-1)) < 1e-5, ("dW", name, rel_err(grads[name][0], dw.reshape(-1)))
        assert rel_err(grads[name][1], b.grad.numpy()) < 1e-5, ("db", name, rel_err(grads[name][1], b.grad.numpy()))
