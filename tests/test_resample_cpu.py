"""CPU: UPSAMPLE and RGBTOYUV on the host — the restatement of tests/resample_ref.py against the reference's compiled CPU Matrix, the edge
classes' sizing and descriptions, the graphs of the two models against the reference's compiled host, every refusal with its message, and
the new prototypes in include/convnet_hip.h (tests/test_abi_exports.py then demands their export)."""
import os

import numpy as np
import pytest

import ref_host
import resample_ref as ref
from convnet_amd import _lib, models
from convnet_amd.convnet import ConvNet
from convnet_amd.edge import Edge, RGBToYUVEdge, UpSampleEdge


@pytest.fixture(scope="module")
def cpu_host():
    if not os.path.exists(ref_host.CPU_SO):
        pytest.skip("oracle/_ref/libref_host_cpu.so not built (needs the reference tree at build time)")
    return ref_host.RefHost(ref_host.CPU_SO)


# ---- the restatement against the reference's CPU Matrix -------------------------------------------------------------------------------
def _probe_net(channels, size, factor):
    """input -> UPSAMPLE -> up -> FC -> one LINEAR unit with LINEAR_ERROR.  At batch 1 the loss derivative is exactly 1 and
    scale_gradients / batch is 1, so the FC weight gradient 0 * dW + 1 * (1 * up) IS the upsampled state, bit for bit."""
    s = models._header("upsample_probe")
    s += models._layer("input", channels, size=size) + models._layer("up", channels)
    s += models._layer("output", 1, "LINEAR", extra="  loss_function: LINEAR_ERROR\n  performance_metric: LINEAR_ERROR\n")
    return s + models._upsample("input", "up", factor) + models._fc("up", "output", l2=0.0)


@pytest.mark.parametrize("factor", [1, 2, 3, 4])
@pytest.mark.parametrize("channels,size", [(1, 1), (2, 3), (3, 4)])
def test_restated_upsample_equals_the_reference_cpu_matrix(cpu_host, tmp_path, factor, channels, size):
    """Square images only: src/CPUMatrix.cc:869-899 takes inp_height = inp_width.  Factors 1, 2, 4 bit for bit; factor 3 within 2^-22
    relative (the CPU build leaves f*f * (x * (1 / (f*f))), three roundings of 2^-24)."""
    seed = 5
    m, d = ref_host.write_configs(tmp_path, _probe_net(channels, size, factor), 1, 1, seed, "probe")
    p0 = cpu_host.init_params(m, d)
    big = size * factor
    D = channels * big * big
    assert p0.size == (D + 1 + 127) // 128 * 128      # one edge with parameters: D weights, then the bias, padded to 128 floats
    g = cpu_host.gradient(m, d, p0)[:D].reshape(channels, big, big, 1)
    x = ref_host.hash_batch(seed, 0, channels * size * size, True).reshape(channels, size, size, 1)
    mine = ref.upsample(x, factor)
    assert np.any(x != 0)
    if factor in (1, 2, 4):
        assert np.array_equal(g.view(np.uint32), mine.view(np.uint32))
    else:
        rel = np.abs(g.astype(np.float64) - mine) / np.abs(mine)
        print("factor", factor, "worst relative difference in units of 2^-24:", rel.max() * 2.0 ** 24)
        assert rel.max() <= 2.0 ** -22
        # and the restated CPU form is what the CPU build left
        assert np.array_equal(g.view(np.uint32), ref.upsample_reference_forms(x, factor)[1].view(np.uint32))


def test_both_reference_forms_are_within_the_bound_of_the_definition_and_exact_for_powers_of_two():
    x = ref_host.hash_batch(3, 1, 2 * 5 * 7 * 4, True).reshape(2, 5, 7, 4)
    for f in (1, 2, 3, 4, 5, 6, 7, 8):
        mine = ref.upsample(x, f)
        for form in ref.upsample_reference_forms(x, f):
            if f in (1, 2, 4, 8):
                assert np.array_equal(form, mine)
            else:
                assert (np.abs(form.astype(np.float64) - mine) / np.abs(mine)).max() <= 2.0 ** -22


def test_restated_accumulation_rounds_the_product_and_the_sum():
    x = np.float32([[[[1.0]]]])
    t = np.full((1, 2, 2, 1), np.float32(1 + 2.0 ** -23))
    out = ref.upsample(x, 2, t, np.float32(1 + 2.0 ** -23))
    # (1 + u)^2 = 1 + 2u + u^2 rounds to 1 + 2u; + 1 = 2 + 2u, exactly representable
    assert np.all(out == np.float32(2 + 2.0 ** -22))
    assert np.array_equal(ref.upsample(x, 2, t, 1.0), t + 1)


# ---- edge classes ---------------------------------------------------------------------------------------------------------------------
def test_upsample_edge_sizes_and_describes_itself_like_the_reference():
    net = ConvNet(models.conv_autoencoder(image_size=16))
    e = net.GetEdgeByName("dec1:up1")
    assert type(e) is UpSampleEdge and e.sample_factor_ == 2
    assert (e.image_size_y_, e.image_size_x_, e.GetNumModulesY(), e.GetNumModulesX(), e.GetNumModulesT()) == (4, 4, 8, 8, 1)
    assert e.GetDescription() == "dec1:up1  Upsample factor 2 Layer: 4-4-32 : 8-8-32\n"      # src/upsample_edge.cc:8-16
    assert e.HasNoParameters() and e.GetParameterMemoryRequirement() == 0
    assert not e.CanFuseUp(e.GetDest()) and not e.can_fuse_mask
    up2 = net.GetLayerByName("up2")
    assert (up2.GetSizeY(), up2.GetSizeX(), up2.GetNumChannels()) == (16, 16, 16)
    out = net.GetLayerByName("output")
    assert (out.GetSizeY(), out.GetSizeX(), out.GetNumChannels()) == (16, 16, 3) and out.loss_function_ == "SQUARED_ERROR"


def test_upsample_edge_keeps_a_rectangular_image():
    text = models._header("rect") + models._layer("input", 2, extra="  image_size_y: 3\n  image_size_x: 5\n") + models._layer("up", 2)
    text += models._layer("output", 4, "SOFTMAX") + models._upsample("input", "up", 3) + models._fc("up", "output")
    net = ConvNet(text)
    e = net.GetEdgeByName("input:up")
    assert (e.GetNumModulesY(), e.GetNumModulesX()) == (9, 15)
    up = net.GetLayerByName("up")
    assert (up.GetSizeY(), up.GetSizeX()) == (9, 15)


def test_rgb_to_yuv_edge_keeps_the_image_size():
    net = ConvNet(models.skip_sum_small())
    e = net.GetEdgeByName("input:yuv")
    assert type(e) is RGBToYUVEdge
    assert (e.GetNumModulesY(), e.GetNumModulesX(), e.GetNumModulesT()) == (16, 16, 1)
    assert e.GetDescription() == "input:yuv RGB to YUV 16-16"                                 # src/rgb_to_yuv_edge.cc:7-11
    assert not e.CanFuseUp(e.GetDest()) and not e.can_fuse_mask
    yuv = net.GetLayerByName("yuv")
    assert (yuv.GetSizeY(), yuv.GetSizeX(), yuv.GetNumChannels()) == (16, 16, 3)
    with pytest.raises(SystemExit) as err:
        e.ComputeDown(None, None, None, None, True)
    assert str(err.value) == "RGBtoYUV backprop Not implemented."
    up = net.GetEdgeByName("coarse:sum")
    assert type(up) is UpSampleEdge and (up.GetNumModulesY(), up.GetNumModulesX()) == (16, 16)
    # the 1x1 edge writes `sum` first, the upsampled map is added
    assert [f.GetName() for f in net.GetLayerByName("sum").incoming_edge_] == ["stem:sum", "coarse:sum"]


def _graph(net):
    layers = [(l.GetName(), l.GetSizeY(), l.GetSizeX(), l.GetNumChannels(), bool(l.IsInput()), bool(l.IsOutput())) for l in net.layers_]
    edges = [(e.GetSource().GetName(), e.GetDest().GetName(), e.GetParameterMemoryRequirement()) for e in net.edges_]
    return layers, edges, sum(((n + 127) // 128) * 128 for _, _, n in edges)


@pytest.mark.parametrize("which", ["conv_autoencoder", "conv_autoencoder_16", "skip_sum_no_colour"])
def test_models_build_the_same_graph_as_the_reference(cpu_host, tmp_path, which):
    text = {"conv_autoencoder": models.conv_autoencoder, "conv_autoencoder_16": lambda: models.conv_autoencoder(image_size=16),
            "skip_sum_no_colour": lambda: models.skip_sum_small(colour=False)}[which]()
    m, d = ref_host.write_configs(tmp_path, text, 2, 1, 1, which)
    assert _graph(ConvNet(text)) == cpu_host.describe(m, d)


def test_skip_sum_small_builds_the_reference_graph_below_its_colour_edge(cpu_host, tmp_path):
    """The reference's RGBToYUVEdge never sets num_modules (src/rgb_to_yuv_edge.cc has no SetImageSize), so its destination and, through
    it, every layer above the edge come out 1 x 1 there: their sizes, and the parameter count of the FC edge that depends on them, are
    excluded.  What does not depend on the size is compared: the input layer, every layer's name, channels and role, the edge list, and
    the parameter counts of the convolutions."""
    text = models.skip_sum_small()
    m, d = ref_host.write_configs(tmp_path, text, 2, 1, 1, "skip_sum")
    layers, edges, _ = cpu_host.describe(m, d)
    mine_layers, mine_edges, _ = _graph(ConvNet(text))
    assert mine_layers[0] == layers[0] == ("input", 16, 16, 3, True, False)
    strip = lambda ls: [(n, c, i, o) for n, _, _, c, i, o in ls]  # noqa: E731
    assert strip(mine_layers) == strip(layers)
    assert dict((l[0], l[1:3]) for l in layers)["yuv"] == (1, 1), "the reference sizes the edge's destination after all: compare it"
    assert [e[:2] for e in mine_edges] == [e[:2] for e in edges]
    sized = {("pool2", "output")}
    assert [e for e in mine_edges if e[:2] not in sized] == [e for e in edges if e[:2] not in sized]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _exits(text, *words):
    with pytest.raises(SystemExit) as e:
        ConvNet(text, fused=True)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    return str(e.value)


def _edge(kind, src, dst, extra=""):
    return f'edge {{\n  source: "{src}"\n  dest: "{dst}"\n  edge_type: {kind}\n{extra}}}\n\n'


def _small(edges, mid_channels=3, frames=None, mid="mid"):
    s = models._header("refusals") + models._layer("input", 3, size=8, frames=frames) + models._layer(mid, mid_channels)
    return s + models._layer("output", 4, "SOFTMAX") + edges


def test_downsample_is_refused_and_points_to_average_pooling():
    msg = _exits(_small(_edge("DOWNSAMPLE", "input", "mid", "  sample_factor: 2\n") + models._fc("mid", "output")),
                 "input:mid", "DOWNSAMPLE", "AVERAGE_POOL", "kernel_size = stride = sample_factor (2)", "backward")
    assert "out of hot-path scope" not in msg


@pytest.mark.parametrize("factor", [0, -2])
def test_a_sample_factor_below_one_is_refused(factor):
    _exits(_small(_edge("UPSAMPLE", "input", "mid", f"  sample_factor: {factor}\n") + models._fc("mid", "output")),
           "input:mid", f"sample_factor {factor}", "UPSAMPLE", "at least 1")


@pytest.mark.parametrize("kind", ["UPSAMPLE", "RGBTOYUV"])
def test_clips_are_refused(kind):
    _exits(_small(_edge(kind, "input", "mid") + models._fc("mid", "output"), frames=4), "input:mid", kind, "image_size_t > 1", "4 frames")


def test_rgb_to_yuv_needs_three_channels():
    text = models._header("refusals") + models._layer("input", 4, size=8) + models._layer("mid", 4) + models._layer("output", 4, "SOFTMAX")
    _exits(text + _edge("RGBTOYUV", "input", "mid") + models._fc("mid", "output"), "input:mid", "RGBTOYUV", "3 channels", "num_channels is 4")
    _exits(_small(_edge("RGBTOYUV", "input", "mid") + models._fc("mid", "output"), mid_channels=5), "input:mid", "3 channels", "5 on its destination")


def test_rgb_to_yuv_on_a_source_that_needs_a_derivative_is_refused():
    head = models._header("refusals") + models._layer("input", 3, size=8) + models._layer("h", 3) + models._layer("yuv", 3)
    head += models._layer("output", 4, "SOFTMAX")
    tail = models._fc("yuv", "output")
    _exits(head + models._conv("input", "h", 3, 1, 1) + _edge("RGBTOYUV", "h", "yuv") + tail,
           "h:yuv", "RGBTOYUV", "RGBtoYUV backprop Not implemented.", "layer h needs a derivative", "block_backprop")
    # behind block_backprop nothing is asked of it
    net = ConvNet(head + models._conv("input", "h", 3, 1, 1) + _edge("RGBTOYUV", "h", "yuv", "  block_backprop: true\n") + tail)
    assert type(net.GetEdgeByName("h:yuv")) is RGBToYUVEdge


def test_an_upsample_edge_beside_another_back_propagated_edge_is_refused():
    head = models._header("refusals") + models._layer("input", 3, size=8) + models._layer("h", 4) + models._layer("up", 4)
    head += models._layer("side", 4) + models._layer("output", 4, "SOFTMAX")
    edges = models._conv("input", "h", 3, 1, 1) + _edge("UPSAMPLE", "h", "up", "  sample_factor: 2\n") + models._conv("h", "side", 3, 1, 1)
    tail = models._fc("up", "output") + models._fc("side", "output")
    _exits(head + edges + tail, "h:up", "UPSAMPLE", "overwrites the derivative", "layer h", "edge h:side", "block_backprop")
    # either edge blocked, or an input layer as the source (no derivative at all), is fine
    blocked = edges.replace("sample_factor: 2\n", "sample_factor: 2\n  block_backprop: true\n")
    assert type(ConvNet(head + blocked + tail).GetEdgeByName("h:up")) is UpSampleEdge
    two = (models._header("refusals") + models._layer("input", 3, size=8) + models._layer("up", 3) + models._layer("side", 4)
           + models._layer("output", 4, "SOFTMAX") + _edge("UPSAMPLE", "input", "up", "  sample_factor: 2\n")
           + models._conv("input", "side", 3, 1, 1) + models._fc("up", "output") + models._fc("side", "output"))
    assert type(ConvNet(two).GetEdgeByName("input:up")) is UpSampleEdge


def test_an_unknown_edge_type_keeps_its_message():
    with pytest.raises(SystemExit) as e:
        Edge.ChooseEdgeClass(type("C", (), {"edge_type": "WARP", "source": "a", "dest": "b", "sample_factor": 1})())
    assert "Undefined edge type WARP" in str(e.value)


# ---- fused plan -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text", [models.conv_autoencoder(image_size=16), models.skip_sum_small()], ids=["conv_autoencoder", "skip_sum_small"])
def test_the_fused_host_plans_the_unfused_path_around_the_new_edges(text):
    net = ConvNet(text, fused=True)
    for e in net.edges_:
        if isinstance(e, (UpSampleEdge, RGBToYUVEdge)):
            dest, src = net.plan_[e.GetDest()], net.plan_[e.GetSource()]
            assert dest.fuse_relu is None and dest.activate, e.GetName()       # the destination: reference sequence, activation pass
            assert src.down_scale is None, e.GetName()                         # the source: ReLU' and dropout' as passes of their own
    # the layers away from them keep their epilogues
    first = net.GetLayerByName("enc1" if net.model_.name == "conv_autoencoder" else "stem")
    assert net.plan_[first].fuse_relu is True


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_declared_with_the_references_signatures():
    import ctypes
    sigs = _lib.header_signatures(open(_lib.HEADER_PATH).read())
    M, S, I, F = ctypes.POINTER(_lib.cudamat), ctypes.POINTER(_lib.Shape4D), ctypes.c_int, ctypes.c_float
    for name in ("UpSampleGemm", "UpSample"):
        assert sigs[name] == (None, [M, M, S, S, I, F])          # cudamat_conv_gemm.cuh:94-95, cudamat_conv.cuh:72-73
    for name in ("DownSampleGemm", "DownSample"):
        assert sigs[name] == (None, [M, M, S, S, I])             # cudamat_conv_gemm.cuh:97-98, cudamat_conv.cuh:75-76
    assert sigs["RGBToYUV"] == (None, [M, M])                    # cudamat_conv.cuh:78
