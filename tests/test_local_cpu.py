"""Locally connected layers without a GPU: the host's LocalEdge (graph building, parameter slices after src/local_edge.cc) and the
float64 oracle of tests/local_ref.py, pinned against an independent torch-CPU unfold / fold formulation and against its own
adjointness."""
import numpy as np
import pytest

from convnet_amd import models
from convnet_amd.convnet import ConvNet
from convnet_amd.edge import LocalEdge

import local_ref as L
from local_ref import LocalGeom

GEOMS = [
    LocalGeom(N=1, C=3, H=7, W=7, F=7, Ky=3, Kx=3),
    LocalGeom(N=6, C=3, H=9, W=8, F=16, Ky=3, Kx=2, sy=2, sx=1, pady=1, padx=0),
    LocalGeom(N=5, C=4, H=6, W=10, F=5, Ky=2, Kx=4, sy=1, sx=3, pady=0, padx=2),
    LocalGeom(N=4, C=2, H=11, W=11, F=3, Ky=2, Kx=2, sy=3, sx=3),              # stride > kernel
    LocalGeom(N=3, C=5, H=5, W=5, F=4, Ky=5, Kx=5, pady=2, padx=2),
    LocalGeom(N=7, C=16, H=5, W=5, F=9, Ky=3, Kx=3, pady=1, padx=1),
    LocalGeom(N=2, C=1, H=12, W=7, F=2, Ky=4, Kx=1, sy=2, sx=2, pady=1, padx=0),
    LocalGeom(N=9, C=3, H=8, W=8, F=6, Ky=1, Kx=1),
    LocalGeom(N=3, C=6, H=10, W=9, F=8, Ky=3, Kx=5, sy=2, sx=2, pady=2, padx=1),
    LocalGeom(N=1, C=2, H=4, W=4, F=1, Ky=4, Kx=4),                            # one module
]


def _data(g, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(g.in_shape()), rng.standard_normal(g.bank_shape()), rng.standard_normal(g.out_shape()))


@pytest.mark.parametrize("g", GEOMS, ids=str)
def test_oracle_matches_torch_unfold(g):
    x, w, dy = _data(g)
    np.testing.assert_allclose(L.up(g, x, w), L.torch_up(g, x, w), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(L.down(g, dy, w), L.torch_down(g, dy, w), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(L.outp(g, x, dy), L.torch_outp(g, x, dy), rtol=1e-12, atol=1e-12)
    # the element-wise forms the large-layer GPU test samples with
    rng = np.random.default_rng(1)
    up, down, outp = L.up(g, x, w), L.down(g, dy, w), L.outp(g, x, dy)
    for _ in range(8):
        f, my, mx, n = (int(rng.integers(s)) for s in g.out_shape())
        assert abs(L.up_at(g, x, w, f, my, mx, n) - up[f, my, mx, n]) < 1e-12
        c, iy, ix, n = (int(rng.integers(s)) for s in g.in_shape())
        assert abs(L.down_at(g, dy, w, c, iy, ix, n) - down[c, iy, ix, n]) < 1e-12
        m, c, ky, kx, f = (int(rng.integers(s)) for s in g.bank_shape())
        assert abs(L.outp_at(g, x, dy, m, c, ky, kx, f) - outp[m, c, ky, kx, f]) < 1e-12


@pytest.mark.parametrize("g", GEOMS, ids=str)
def test_oracle_is_adjoint(g):
    x, w, dy = _data(g, seed=3)
    a = float((L.up(g, x, w) * dy).sum())
    b = float((x * L.down(g, dy, w)).sum())
    c = float((w * L.outp(g, x, dy)).sum())
    assert abs(a - b) <= 1e-10 * max(1.0, abs(a)) and abs(a - c) <= 1e-10 * max(1.0, abs(a))


def test_oracle_scale_targets_and_output():
    g = GEOMS[1]
    x, w, dy = _data(g)
    t = np.random.default_rng(5).standard_normal(g.out_shape())
    np.testing.assert_allclose(L.up(g, x, w, t, 1.0), t + L.up(g, x, w))
    tw = np.random.default_rng(6).standard_normal(g.bank_shape())
    np.testing.assert_allclose(L.outp(g, x, dy, tw, 1.0, 0.25), tw + 0.25 * L.outp(g, x, dy))


def _local_net(pad=1, stride=1, k=3, size=9, tie=False, bias=True):
    s = models._header("local_test") + models._layer("input", 3, size=size)
    s += models._layer("h1", 7, "RECTIFIED_LINEAR") + models._layer("h2", 7, "RECTIFIED_LINEAR") + models._layer("output", 4, "SOFTMAX")
    e1 = models._local("input", "h1", k, stride, pad)
    e2 = models._local("input", "h2", k, stride, pad)
    if tie:
        e2 = e2.replace('  edge_type: LOCAL\n', '  edge_type: LOCAL\n  tied_to: "input:h1"\n')
    if not bias:
        e1 = e1.replace('  edge_type: LOCAL\n', '  edge_type: LOCAL\n  has_no_bias: true\n')
    return s + e1 + e2 + models._fc("h1", "output") + models._fc("h2", "output")


@pytest.mark.parametrize("k,stride,pad,size", [(3, 1, 1, 9), (5, 2, 0, 13), (2, 3, 1, 10), (4, 1, 2, 6)])
def test_local_edge_builds_and_slices_like_local_edge_cc(k, stride, pad, size):
    net = ConvNet(_local_net(pad, stride, k, size))
    e = net.GetEdgeByName("input:h1")
    assert isinstance(e, LocalEdge)
    g = LocalGeom(N=1, C=3, H=size, W=size, F=7, Ky=k, Kx=k, sy=stride, sx=stride, pady=pad, padx=pad)
    n, wshape, bshape, s4 = L.local_edge_sizes(g)
    assert (e.num_modules_y_, e.num_modules_x_) == (g.My, g.Mx)
    assert net.GetLayerByName("h1").GetSizeY() == g.My
    assert e.GetParameterMemoryRequirement() == n == 7 * (k * k * 3 * g.M + g.M)
    assert (e.conv_desc_.padding_y, e.conv_desc_.stride_x, e.conv_desc_.num_input_channels) == (-pad, stride, 3)
    assert "Local Kernel" in e.GetDescription()
    nb = ConvNet(_local_net(pad, stride, k, size, bias=False)).GetEdgeByName("input:h1")
    assert nb.GetParameterMemoryRequirement() == L.local_edge_sizes(g, has_bias=False)[0] == 7 * k * k * 3 * g.M
    # the slices themselves need device memory: tests/test_local_gpu.py checks (rows, cols) and Shape4D after SetMemory
    assert wshape == (7, k * k * 3 * g.M) and bshape == (1, 7 * g.M) and s4 == (7, k, k, 3 * g.M)


def test_tied_local_edge_has_no_parameters_and_shares_the_geometry():
    net = ConvNet(_local_net(tie=True))
    a, b = net.GetEdgeByName("input:h1"), net.GetEdgeByName("input:h2")
    assert b.is_tied_ and b.tied_edge_ is a and b.GetParameterMemoryRequirement() == 0
    assert a.num_shares_ == 2 and (b.num_modules_y_, b.num_modules_x_) == (a.num_modules_y_, a.num_modules_x_)
    assert sum(e.GetParameterMemoryRequirement() for e in net.edges_) == a.GetParameterMemoryRequirement() + 2 * (4 * 7 * 81 + 4)


def test_cifar_local_graph():
    net = ConvNet(models.cifar_local())
    sizes = {l.GetName(): (l.GetSizeY(), l.GetNumChannels()) for l in net.layers_}
    assert sizes["conv1"] == (24, 64) and sizes["pool1"] == (11, 64) and sizes["conv2"] == (11, 64) and sizes["pool2"] == (5, 64)
    assert sizes["local3"] == (5, 64) and sizes["local4"] == (5, 32) and sizes["output"] == (1, 10)
    l3, l4 = net.GetEdgeByName("pool2:local3"), net.GetEdgeByName("local3:local4")
    assert isinstance(l3, LocalEdge) and isinstance(l4, LocalEdge)
    assert l3.GetParameterMemoryRequirement() == 64 * (9 * 64 * 25 + 25) and l4.GetParameterMemoryRequirement() == 32 * (9 * 64 * 25 + 25)
    fwd, _ = models.count_macs(net)
    assert fwd == 24 * 24 * 64 * 75 + 11 * 11 * 64 * 1600 + 25 * 64 * 576 + 25 * 32 * 576 + 800 * 10


def test_three_d_local_layer_raises():
    s = _local_net().replace("  image_size_x: 9\n", "  image_size_x: 9\n  image_size_t: 3\n", 1)
    with pytest.raises(SystemExit):
        ConvNet(s)
