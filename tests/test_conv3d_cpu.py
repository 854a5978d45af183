"""Spatio-temporal (3-D) layers without a GPU: the float64 statement of tests/conv3d_ref.py pinned against the composition the
reference defines the operations by (a loop of the pinned 2-D oracle over frame slices, cudamat_conv3d_gemm.cu) and against its own
adjointness, and the host's graph building for nets with image_size_t > 1 (sizes, parameter slices, refusals)."""
import numpy as np
import pytest

import oracle
from oracle import Geom

from convnet_amd import models
from convnet_amd.convnet import ConvNet
from convnet_amd.edge import AvgPoolEdge, ConvEdge, MaxPoolEdge, ResponseNormEdge

import conv3d_ref as R
from conv3d_ref import Geom3D
from golden_cases import rel_err

PORT_PIN = 2e-6   # the port's own pin against the reference's CPU path (DESIGN.md §0 row c), relative

GEOMS = [
    Geom3D(N=2, C=3, H=7, W=6, T=5, F=4, Ky=3, Kx=2, Kt=3, sy=2, sx=1, st=1, pady=1, padx=0),
    Geom3D(N=3, C=2, H=5, W=5, T=7, F=5, Ky=3, Kx=3, Kt=2, st=2, pady=1, padx=1),           # ragged T: frame 6 is never read
    Geom3D(N=1, C=4, H=6, W=6, T=8, F=3, Ky=2, Kx=2, Kt=2, sy=2, sx=2, st=3),               # st > Kt: frames 2, 5 uncovered
    Geom3D(N=4, C=3, H=4, W=5, T=9, F=2, Ky=1, Kx=1, Kt=5, st=2),
    Geom3D(N=2, C=2, H=5, W=4, T=6, F=3, Ky=3, Kx=3, Kt=1, st=1, pady=1, padx=1),           # Kt = 1: frames independent
    Geom3D(N=2, C=1, H=6, W=6, T=10, F=2, Ky=5, Kx=5, Kt=3, sy=2, sx=2, st=3, pady=2, padx=2),
    Geom3D(N=5, C=2, H=4, W=4, T=5, F=3, Ky=2, Kx=3, Kt=5, st=1, padx=1),                   # Kt = T: one output frame
    Geom3D(N=2, C=2, H=4, W=4, T=11, F=2, Ky=3, Kx=3, Kt=3, st=2, pady=1, padx=1),
]


def _data(g, seed=0, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(s).astype(dtype) for s in (g.in_shape(), g.filt_shape(), g.out_shape()))


def _frame_geom(g):
    return Geom(g.N, g.C * g.Kt, g.H, g.W, g.F, g.Ky, g.Kx, g.sy, g.sx, g.pady, g.padx)


def _loop_of_2d(g, x, w, dy):
    """The reference's definition: 2-D operations on C*Kt contiguous channels of a frame slice, frame by frame."""
    g2, P = _frame_geom(g), oracle.port
    w2 = np.ascontiguousarray(w.reshape(g.Kt * g.C, g.Ky, g.Kx, g.F))
    up = np.zeros(g.out_shape(), np.float32)
    down = np.zeros(g.in_shape(), np.float32)
    outp = np.zeros(g2.filt_shape(), np.float32)
    for m in range(g.Mt):
        xs = np.ascontiguousarray(x[m * g.st:m * g.st + g.Kt].reshape(g2.in_shape()))
        up[m] = P.conv_up(g2, xs, w2)
        down[m * g.st:m * g.st + g.Kt] += P.conv_down(g2, np.ascontiguousarray(dy[m]), w2).reshape(g.Kt, g.C, g.H, g.W, g.N)
        outp = P.conv_outp(g2, xs, np.ascontiguousarray(dy[m]), outp, 1.0, 0.5)
    return up, down, outp.reshape(g.filt_shape())


@pytest.mark.parametrize("g", GEOMS, ids=str)
def test_ref_conv_equals_the_loop_of_pinned_2d_ops(g):
    x, w, dy = _data(g)
    up, down, outp = _loop_of_2d(g, x, w, dy)
    for name, got, want in (("up", R.conv_up(g, x, w), up), ("down", R.conv_down(g, dy, w), down),
                            ("outp", R.conv_outp(g, x, dy, None, 0.0, 0.5), outp)):
        err = rel_err(got, want)
        print(f"{g} {name}: {err:.2e}")
        assert err <= PORT_PIN, (name, err)


@pytest.mark.parametrize("g", GEOMS, ids=str)
def test_ref_conv_is_adjoint(g):
    x, w, dy = _data(g, seed=3, dtype=np.float64)
    a = float((R.conv_up(g, x, w) * dy).sum())
    b = float((x * R.conv_down(g, dy, w)).sum())
    c = float((w * R.conv_outp(g, x, dy)).sum())
    assert abs(a - b) <= 1e-10 * max(1.0, abs(a)) and abs(a - c) <= 1e-10 * max(1.0, abs(a))


def test_ref_conv_uncovered_frames_and_scale_targets():
    g = GEOMS[2]
    x, w, dy = _data(g)
    t = np.random.default_rng(5).standard_normal(g.in_shape())
    dx = R.conv_down(g, dy, w, t, 1.0)
    for ti in (2, 5):
        np.testing.assert_array_equal(dx[ti], t[ti])
    np.testing.assert_array_equal(R.conv_down(g, dy, w)[2], 0.0)
    tw = np.random.default_rng(6).standard_normal(g.filt_shape())
    np.testing.assert_allclose(R.conv_outp(g, x, dy, tw, 1.0, 0.25), tw + 0.25 * R.conv_outp(g, x, dy))


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("C,size_f", [(8, 3), (16, 5), (7, 4)])
def test_ref_rnorm_equals_the_pinned_2d_op_per_frame(C, size_f, blocked):
    rng = np.random.default_rng(C)
    x, dy = (rng.standard_normal((3, C, 4, 5, 2)).astype(np.float32) for _ in range(2))
    P = oracle.port
    for t in range(3):
        f, b = P.rnorm(np.ascontiguousarray(x[t]), size_f, 0.01, 0.75, blocked), P.rnorm_undo(np.ascontiguousarray(dy[t]), np.ascontiguousarray(x[t]), size_f, 0.01, 0.75, blocked)
        assert rel_err(R.rnorm(x, size_f, 0.01, 0.75, blocked)[t], f) <= PORT_PIN
        assert rel_err(R.rnorm_undo(dy, x, size_f, 0.01, 0.75, blocked)[t], b) <= PORT_PIN


POOLS_2D = [Geom(N=3, C=4, H=7, W=6, F=4, Ky=3, Kx=3, sy=2, sx=2, pady=1, padx=1), Geom(N=2, C=3, H=8, W=8, F=3, Ky=2, Kx=2, sy=2, sx=2),
            Geom(N=5, C=2, H=9, W=7, F=2, Ky=4, Kx=3, sy=3, sx=2, pady=1, padx=0)]


@pytest.mark.parametrize("g2", POOLS_2D, ids=str)
def test_ref_pooling_with_one_frame_equals_the_pinned_2d_ops(g2):
    g = Geom3D(g2.N, g2.C, g2.H, g2.W, 1, g2.C, g2.Ky, g2.Kx, 1, g2.sy, g2.sx, 1, g2.pady, g2.padx, 0)
    rng = np.random.default_rng(1)
    x = rng.integers(-4, 5, g2.in_shape()).astype(np.float32)          # small integers: ties, and every sum exact in fp32
    dy = rng.integers(-4, 5, g2.pooled_shape()).astype(np.float32)
    P = oracle.port
    y = P.max_pool(g2, x)
    np.testing.assert_array_equal(R.max_pool(g, x[None])[0], y)
    np.testing.assert_array_equal(R.max_pool_undo(g, x[None], dy[None], y[None])[0], P.max_pool_undo(g2, x, dy, y))
    # averages divide: exact only where the window size is a power of two, so compare at fp32 resolution
    np.testing.assert_allclose(R.avg_pool(g, x[None])[0], P.avg_pool(g2, x), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(R.avg_pool_undo(g, dy[None])[0], P.avg_pool_undo(g2, dy), rtol=1e-6, atol=1e-6)


def test_ref_pooling_over_time_is_adjoint_and_clips():
    g = Geom3D(N=2, C=3, H=6, W=5, T=7, F=3, Ky=3, Kx=2, Kt=3, sy=2, sx=1, st=2, pady=1, padx=0, padt=1)
    rng = np.random.default_rng(2)
    x, dy = rng.standard_normal(g.in_shape()), rng.standard_normal(g.pooled_shape())
    assert g.Mt == 4
    a, b = float((R.avg_pool(g, x) * dy).sum()), float((x * R.avg_pool_undo(g, dy)).sum())
    assert abs(a - b) <= 1e-12 * max(1.0, abs(a))
    # the first box is clipped in time (frames -1..1 -> 0..1) and in y (rows -1..1 -> 0..1): the average divides by 2*2*2
    np.testing.assert_allclose(R.avg_pool(g, x)[0, :, 0, 0, :], x[0:2, :, 0:2, 0:2, :].sum(axis=(0, 2, 3)) / 8)
    y = R.max_pool(g, x)
    np.testing.assert_array_equal(y[1, :, 1, 2, :], x[1:4, :, 1:4, 2:4, :].max(axis=(0, 2, 3)))
    # without ties every box routes its derivative to exactly one input
    np.testing.assert_allclose(R.max_pool_undo(g, x, dy, y).sum(axis=(0, 2, 3)), dy.sum(axis=(0, 2, 3)))


# ---- host graph -----------------------------------------------------------------------------------------------------------------------
def test_video_small_graph():
    net = ConvNet(models.video_small())
    sizes = {l.GetName(): (l.GetSizeY(), l.GetSizeX(), l.GetSizeT(), l.GetNumChannels()) for l in net.layers_}
    assert sizes == {"input": (32, 32, 16, 3), "conv1": (32, 32, 14, 64), "pool1": (15, 15, 14, 64), "conv2": (15, 15, 12, 128),
                     "pool2": (7, 7, 6, 128), "rnorm2": (7, 7, 6, 128), "conv3": (7, 7, 4, 128), "pool3": (1, 1, 1, 128),
                     "output": (1, 1, 1, 10)}
    kinds = {e.GetName(): type(e) for e in net.edges_}
    assert kinds["input:conv1"] is ConvEdge and kinds["conv1:pool1"] is MaxPoolEdge and kinds["pool2:rnorm2"] is ResponseNormEdge
    assert kinds["conv3:pool3"] is AvgPoolEdge
    mt = {e.GetName(): e.GetNumModulesT() for e in net.edges_}
    assert mt == {"input:conv1": 14, "conv1:pool1": 14, "pool1:conv2": 12, "conv2:pool2": 6, "pool2:rnorm2": 6, "rnorm2:conv3": 4,
                  "conv3:pool3": 1, "pool3:output": 1}
    params = {e.GetName(): e.GetParameterMemoryRequirement() for e in net.edges_}
    assert params["input:conv1"] == 64 * (3 * 3 * 3 * 3 + 1) and params["pool1:conv2"] == 128 * (3 * 3 * 3 * 64 + 1)
    assert params["rnorm2:conv3"] == 128 * (3 * 3 * 3 * 128 + 1) and params["pool3:output"] == 10 * (128 + 1)
    assert sum(params.values()) == 64 * 82 + 128 * 1729 + 128 * 3457 + 1290
    p1, p2, p3 = (net.GetEdgeByName(n) for n in ("conv1:pool1", "conv2:pool2", "conv3:pool3"))
    assert not p1.HasTimeWindow() and p2.HasTimeWindow() and p3.HasTimeWindow()
    assert (p3.conv_desc_.kernel_size_y, p3.conv_desc_.kernel_size_x, p3.conv_desc_.kernel_size_t) == (7, 7, 4)
    fwd, train = models.count_macs(net)
    c1, c2, c3 = 32 * 32 * 14 * 64 * 81, 15 * 15 * 12 * 128 * 27 * 64, 7 * 7 * 4 * 128 * 27 * 128
    assert fwd == c1 + c2 + c3 + 1280 and train == 2 * c1 + 3 * (c2 + c3 + 1280)
    d = net.GetEdgeByName("pool1:conv2").GetDescription()
    assert "Convolutional Kernel: 3-3-64-3 : 128 Layer: 15-15-14 : 15-15-12" in d
    assert net.GetEdgeByName("pool1:conv2").conv_desc_.kernel_size_t == 3


def test_non_shared_bias_counts_every_output_frame():
    s = models.video_small().replace("  shared_bias: true\n", "  shared_bias: false\n", 1)
    e = ConvNet(s).GetEdgeByName("input:conv1")
    assert e.GetParameterMemoryRequirement() == 64 * (81 + 32 * 32 * 14)


def _clip_net(edge, act="RECTIFIED_LINEAR", extra=""):
    s = models._header("clip") + models._layer("input", 3, size=8, frames=4) + models._layer("h", 6, act, extra=extra)
    return s + models._layer("output", 4, "SOFTMAX") + edge + models._fc("h", "output")


@pytest.mark.parametrize("make,what", [
    (lambda: _clip_net(models._local("input", "h", 3, 1, 1)), "locally connected"),
    (lambda: _clip_net(models._nin("input", "h")), "CONV_ONETOONE"),
    (lambda: models._BN_DEFAULTS + _clip_net(models._time(models._conv("input", "h", 3, 1, 1), kt=2), extra=models._BN), "batch_normalize"),
    (lambda: _clip_net(models._time(models._conv("input", "h", 3, 1, 1), kt=2).replace("  padding: 1\n", "  padding: 1\n  padding_t: 1\n")), "padding_t"),
    (lambda: _clip_net(models._time(models._conv("input", "h", 3, 1, 1), kt=5)), "kernel_size_t"),
], ids=["local", "onetoone", "batchnorm", "padding_t", "kt_gt_T"])
def test_refusals_name_what_is_refused(make, what):
    with pytest.raises(SystemExit) as ei:
        ConvNet(make())
    msg = str(ei.value)
    # (the LOCAL refusal predates this feature and keeps its text, which names no edge)
    assert what in msg and ("input:h" in msg or "layer h" in msg or what == "locally connected"), msg


def test_a_supported_clip_net_builds():
    net = ConvNet(_clip_net(models._time(models._conv("input", "h", 3, 1, 1), kt=2, st=2)))
    assert net.GetLayerByName("h").GetSizeT() == 2 and net.GetEdgeByName("h:output")._input_size() == 8 * 8 * 2 * 6
