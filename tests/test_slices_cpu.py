"""CPU: layer slices on the host — graph and layout against the reference's compiled host, the name-order layout, the refusals, and
the fused host's per-destination plan.  Nets: tests/slice_nets.py."""
import json
import os

import numpy as np
import pytest

import ref_host
import slice_nets as nets
from convnet_amd import models
from convnet_amd.convnet import ConvNet


@pytest.fixture(scope="module")
def cpu_host():
    if not os.path.exists(ref_host.CPU_SO):
        pytest.skip("oracle/_ref/libref_host_cpu.so not built (needs the reference tree at build time)")
    return ref_host.RefHost(ref_host.CPU_SO)


def _graph(net):
    layers = [(l.GetName(), l.GetSizeY(), l.GetSizeX(), l.GetNumChannels(), bool(l.IsInput()), bool(l.IsOutput())) for l in net.layers_]
    edges = [(e.GetSource().GetName(), e.GetDest().GetName(), e.GetParameterMemoryRequirement()) for e in net.edges_]
    return layers, edges, sum(((n + 127) // 128) * 128 for _, _, n in edges)


VERIFICATION_EDGES = [("input", "h1", 112), ("input", "h1", 456), ("h1", "h2", 185), ("h1", "h2", 165), ("h2", "pool", 0), ("pool", "output", 1290)]


def test_verification_net_builds_the_graph_the_issue_records():
    """The figures of the reference host's describe() on this net, as recorded when the feature was specified."""
    layers, edges, total = _graph(ConvNet(nets.net_a()))
    assert {n: c for n, _, _, c, _, _ in layers} == {"input": 3, "h1": 10, "h2": 8, "pool": 8, "output": 10}
    assert edges == VERIFICATION_EDGES and total == 2560
    names = [e.GetName() for e in ConvNet(nets.net_a()).edges_]
    assert names == ["input:h1_a", "input:h1_b", "h1_a:h2_a", "h1_b:h2_b", "h2:pool", "pool:output"]      # src/edge.cc:150-155


@pytest.mark.parametrize("which", ["net_a", "net_a_linear", "net_b", "wide_net", "inception_small", "inception_small_pooled", "alexnet_grouped"])
def test_sliced_nets_build_the_same_graph_as_the_reference(cpu_host, tmp_path, which):
    text = {"net_a": nets.net_a, "net_a_linear": lambda: nets.net_a(nets.LINEAR, grad_check=True), "net_b": nets.net_b, "wide_net": nets.wide_net,
            "inception_small": models.inception_small, "inception_small_pooled": lambda: models.inception_small(pooled_branch=True),
            "alexnet_grouped": models.alexnet_grouped}[which]()
    m, d = ref_host.write_configs(tmp_path, text, 2, 1, 1, which)
    layers, edges, total = cpu_host.describe(m, d)
    mine = _graph(ConvNet(text))
    assert mine[0] == layers
    assert mine[1] == edges
    assert mine[2] == total
    if which == "net_a":
        assert edges == VERIFICATION_EDGES and total == 2560


def test_count_macs_counts_an_edge_on_a_slice_by_the_channels_of_its_slice():
    grouped, plain = ConvNet(models.alexnet_grouped()), ConvNet(models.alexnet())
    macs = {}
    for tag, net in (("grouped", grouped), ("plain", plain)):
        for e in net.edges_:
            if hasattr(e, "conv_desc_") and hasattr(e, "weight_optimizer_"):
                d = e.conv_desc_
                macs.setdefault(tag, {}).setdefault(e.GetDest().GetName(), 0)
                macs[tag][e.GetDest().GetName()] += (e.num_modules_y_ * e.num_modules_x_ * d.num_output_channels * d.kernel_size_y * d.kernel_size_x
                                                     * d.num_input_channels)
    for layer, groups in (("hidden1_conv", 1), ("hidden2_conv", 2), ("hidden3_conv", 1), ("hidden4_conv", 2), ("hidden5_conv", 2)):
        assert macs["grouped"][layer] * groups == macs["plain"][layer], layer
    fc = sum(e._input_size() * e.num_output_channels_ for e in plain.edges_ if type(e).__name__ == "FCEdge")
    assert models.count_macs(grouped)[0] == sum(macs["grouped"].values()) + fc
    assert models.count_macs(plain)[0] == sum(macs["plain"].values()) + fc


# ---- layout -------------------------------------------------------------------------------------------------------------------------
def test_slices_lie_in_name_order_whichever_order_they_are_declared_in():
    a_first = ConvNet(nets.net_a())
    b_first = ConvNet(nets.verification_net(h1=(("b", 6), ("a", 4)), h2=(("b", 3), ("a", 5))))
    assert "name: \"b\"" in nets.verification_net(h1=(("b", 6), ("a", 4))).split("layer_slice")[1]      # b really is declared first
    for net in (a_first, b_first):
        h1, h2 = net.GetLayerByName("h1"), net.GetLayerByName("h2")
        assert (h1.GetSliceChannelRange("a"), h1.GetSliceChannelRange("b")) == ((0, 4), (4, 10))
        assert (h2.GetSliceChannelRange("a"), h2.GetSliceChannelRange("b")) == ((0, 5), (5, 8))
        assert (h1.GetNumChannels(), h1.GetNumChannels("a"), h1.GetNumChannels("b")) == (10, 4, 6)
    assert _graph(a_first) == _graph(b_first)


def test_slice_views_are_column_ranges_with_their_own_shape(monkeypatch):
    """SetupSlices on host memory (the trace helper's recorder carries out get_slice on the structs): offsets, extents, Shape4D — and a
    layer's own channels sit behind the last slice."""
    import torch
    import host_trace
    from convnet_amd import matrix
    from convnet_amd.matrix import Matrix
    rec = host_trace.Recorder()
    monkeypatch.setattr(matrix, "lib", rec)
    monkeypatch.setattr(Matrix, "_device", torch.device("cpu"))
    allocate = Matrix.AllocateGPUMemory

    def allocate_and_register(self, rows, cols, name=""):
        allocate(self, rows, cols, name)
        rec.register(self)
    monkeypatch.setattr(Matrix, "AllocateGPUMemory", allocate_and_register)
    text = nets.verification_net(h1=(("b", 6), ("a", 4)))
    head = 'name: "h2"\n  num_channels: 0\n'
    assert text.count(head) == 1
    net = ConvNet(text.replace(head, 'name: "h2"\n  num_channels: 2\n'))        # h2: slices a:5, b:3 and 2 channels of its own
    net.SetBatchsize(5)
    net.AllocateLayerMemory()
    base = lambda m: m.mat_.data_device  # noqa: E731
    h1, h2 = net.GetLayerByName("h1"), net.GetLayerByName("h2")
    assert h2.GetNumChannels() == 10 and net.GetLayerByName("pool").GetNumChannels() == 8
    for l, ranges in ((h1, {"a": (0, 4), "b": (4, 10)}), (h2, {"a": (0, 5), "b": (5, 8)})):
        for whole, get in ((l.GetState(), l.GetState), (l.GetDeriv(), l.GetDeriv)):
            assert (whole.GetRows(), whole.GetCols()) == (5, 81 * l.GetNumChannels())
            for name, (c0, c1) in ranges.items():
                v = get(name)
                assert base(v) - base(whole) == 4 * 5 * 81 * c0, (l.GetName(), name)
                assert (v.GetRows(), v.GetCols()) == (5, 81 * (c1 - c0))
                assert list(v.shape_.shape) == [5, 9, 9, c1 - c0]
    assert (base(h2.GetState("b")) - base(h2.GetState())) // 4 == 2025              # 4-byte aligned only: what the GPU tests run on
    # independent flags: one per slice beside the whole layer's, all reset together (src/layer.cc:307-332)
    assert h1.AddOrOverwriteState("a") and not h1.AddOrOverwriteState("a") and h1.AddOrOverwriteState("b") and h1.AddOrOverwriteState()
    assert h1.AddOrOverwriteDeriv("b") and not h1.AddOrOverwriteDeriv("b") and h1.AddOrOverwriteDeriv("a")
    h1.ResetAddOrOverwrite()
    assert h1.AddOrOverwriteState("a") and h1.AddOrOverwriteDeriv("b")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _exits(text, *words):
    with pytest.raises(SystemExit) as e:
        ConvNet(text, fused=True)
    msg = str(e.value)
    assert all(w in msg for w in words), msg


def test_a_layer_read_whole_and_by_slice_is_refused():
    text = nets.net_a(extra_edges=models._conv("h1", "h2", 3, 1, 1).replace('dest: "h2"', 'dest: "h2"\n  dest_slice: "a"'))
    _exits(text, "layer h1", "read both whole", "by slice", "overwrite")


def test_a_layer_written_whole_and_by_slice_is_refused():
    text = nets.net_a(extra_edges=models._on(models._conv("h1", "h2", 3, 1, 1), "a", ""))
    _exits(text, "layer h2", "written both whole", "by slice", "overwrite")


def test_slices_on_a_layer_with_frames_are_refused():
    text = nets.net_a().replace('name: "input"\n  num_channels: 3\n', 'name: "input"\n  num_channels: 3\n  image_size_t: 4\n')
    _exits(text, "layer_slice on layer h1", "image_size_t > 1", "4 frames")


def test_batch_normalize_on_or_behind_a_slice_is_refused():
    bn = "  batch_normalize: true\n"
    text = nets.net_a().replace('name: "h2"\n', 'name: "h2"\n' + bn)
    _exits(text, "batch_normalize on layer h2", "slices")
    # a whole layer fed from a slice
    text = nets.net_a(extra_edges=models._layer("side", 4, "RECTIFIED_LINEAR", extra=bn) + models._on(models._conv("h1", "side", 3, 1, 1), "a", "")
                      + models._layer("side_out", 10, "SOFTMAX") + models._fc("side", "side_out"))
    _exits(text, "batch_normalize on layer side", "fed from a slice")


def test_an_unknown_slice_name_is_refused_with_the_references_message():
    _exits(nets.net_a().replace('source_slice: "b"', 'source_slice: "c"'), "Layer h1 does not contain a slice called c")
    _exits(nets.net_a().replace('dest_slice: "b"', 'dest_slice: "x"', 1), "Layer h1 does not contain a slice called x")
    _exits(nets.net_a().replace('source: "h2"\n', 'source: "h2"\n  dest_slice: "a"\n'), "Layer pool does not contain a slice called a")
    net = ConvNet(nets.net_a())
    for call in (net.GetLayerByName("h1").GetState, net.GetLayerByName("h1").GetDeriv, net.GetLayerByName("h1").GetNumChannels,
                 net.GetLayerByName("h1").AddOrOverwriteState, net.GetLayerByName("h1").AddOrOverwriteDeriv):
        with pytest.raises(SystemExit) as e:
            call("nope")
        assert str(e.value) == "Layer h1 does not contain a slice called nope"


def test_gaussian_dropout_keeps_its_refusal_with_a_message_of_its_own():
    _exits(nets.net_a().replace('name: "h1"\n', 'name: "h1"\n  gaussian_dropout: true\n'), "gaussian_dropout", "h1")


# ---- the fused host's plan -----------------------------------------------------------------------------------------------------------
def _plans(text, fused=True):
    net = ConvNet(text, fused=fused)
    return net, {l.GetName(): net.plan_[l] for l in net.layers_}


def test_a_concatenated_layer_plans_the_fused_epilogue_on_all_its_writers():
    net, p = _plans(models.inception_small())
    mix = net.GetLayerByName("mix")
    assert [type(e).__name__ for e in mix.incoming_edge_] == ["ConvOneToOneEdge", "ConvEdge", "ConvEdge"]
    assert [e.GetDestSliceName() for e in mix.incoming_edge_] == ["b1x1", "b3x3", "b5x5"] and mix.is_relu
    assert p["mix"].fuse_relu is True and p["mix"].activate is False          # bias + ReLU in all three epilogues, no ApplyActivation
    assert p["mix"].down_scale == 1.0                                         # (one reader of the whole layer: the max pool)
    # h1 of the verification net: two single-writer slices
    _, p = _plans(nets.net_a())
    assert p["h1"].fuse_relu is True and p["h2"].fuse_relu is True and not p["h1"].activate and not p["h2"].activate
    # a pooled branch cannot apply the layer's ReLU: the reference sequence for the whole layer
    _, p = _plans(models.inception_small(pooled_branch=True))
    assert p["mix"].fuse_relu is None and p["mix"].activate is True
    # unfused: the reference sequence everywhere
    _, p = _plans(models.inception_small(), fused=False)
    assert all(v.fuse_relu is None and v.down_scale is None for v in p.values())


def test_a_grouped_layer_plans_down_scale_on_all_its_readers():
    net, p = _plans(nets.net_a(dropprob=0.25))
    h1 = net.GetLayerByName("h1")
    assert [e.GetSourceSliceName() for e in h1.outgoing_edge_] == ["a", "b"]
    assert p["h1"].down_scale == pytest.approx(1 / 0.75) and net._fused_down_scale(h1) == p["h1"].down_scale
    assert p["h2"].down_scale is None                   # the max-pool undo masks but does not scale (dropout 0.25)
    _, p = _plans(nets.net_a())
    assert p["h1"].down_scale == 1.0 and p["h2"].down_scale == 1.0


def test_a_second_writer_into_one_slice_sends_the_whole_layer_to_the_reference_sequence():
    net, p = _plans(nets.second_writer())
    assert [e.GetDestSliceName() for e in net.GetLayerByName("h2").incoming_edge_] == ["a", "b", "a"]
    assert p["h2"].fuse_relu is None and p["h2"].activate is True
    assert p["h1"].fuse_relu is True                    # its neighbour is untouched
    assert p["h1"].down_scale is None                   # ... but h1.b now has two readers: the derivative accumulates first


def test_an_unread_slice_sends_the_whole_layer_to_the_reference_sequence():
    net, p = _plans(nets.unread_slice())
    assert [e.GetSourceSliceName() for e in net.GetLayerByName("h1").outgoing_edge_] == ["a", "a"]
    assert p["h1"].down_scale is None and p["h1"].fuse_relu is True
    # one reader per slice, but channels of the layer's own beside the slices: not all of the layer is covered
    text = nets.net_a()
    head = 'name: "h1"\n  num_channels: 0\n'
    assert text.count(head) == 1
    _, p = _plans(text.replace(head, 'name: "h1"\n  num_channels: 2\n'))
    assert p["h1"].down_scale is None and p["h1"].fuse_relu is None and p["h1"].activate is True


def test_models_without_slices_plan_what_they_planned_before_slices():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_plans.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(nets.all_plan_tables()))
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


# ---- the calls a sliced net makes, recorded without a GPU (tests/host_trace.py) ---------------------------------------------------------
def _calls(lines, entry):
    return [l.split() for l in lines if l.startswith(entry + " ")]


def test_the_edges_of_a_sliced_net_hand_the_library_their_slices():
    """Net A at batch 5, one recorded training step: every conv entry gets the slice views (offsets 0 / 1620 into h1, 0 / 2025 into h2)
    with the slices' channel counts in Shape4D, fused and unfused; layer-level calls stay on the whole layer."""
    import host_trace
    for fused in (False, True):
        lines = host_trace.trace(nets.net_a(), 5, fused)
        step = lines[lines.index("# TrainOneBatch"):]
        step = step[:step[1:].index("# TrainOneBatch") + 1]
        up = _calls(step, "convUpBiasAct" if fused else "convUpGemm")
        assert len(up) == 4
        target = 3 if fused else 2         # (images, filters[, bias], targets, shapes...)
        offsets = [int(c[1 + target].split("+")[1].split(",")[0]) for c in up]
        assert offsets == [0, 1620, 0, 2025], (fused, offsets)
        sources = [int(c[1].split("+")[1].split(",")[0]) for c in up]
        assert sources == [0, 0, 0, 1620]
        shapes = [[a for a in c if a.startswith("S(")] for c in up]
        assert [s[0] for s in shapes] == ["S(5,9,9,3)", "S(5,9,9,3)", "S(5,9,9,4)", "S(5,9,9,6)"]
        assert [s[2] for s in shapes] == ["S(5,9,9,4)", "S(5,9,9,6)", "S(5,9,9,5)", "S(5,9,9,3)"]
        down = _calls(step, "convDownMask" if fused else "convDownGemm")
        assert len(down) == 2              # h2.a -> h1.a, h2.b -> h1.b; the input layer takes no derivative
        if not fused:
            relu = _calls(step, "lower_bound_scalar")
            assert {c[1] for c in relu} == {c[3] for c in relu}       # in place, on whole layers: (5, 810) and (5, 648)
            assert sorted(int(c[1].split(",")[2]) for c in relu) == [648, 810]
        else:
            assert not _calls(step, "lower_bound_scalar") and not _calls(step, "apply_rectified_linear_deriv")


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("which", ["net_b", "net_a_linear_dropout", "second_writer", "unread_slice", "inception", "inception_pooled", "wide_net"])
def test_sliced_nets_run_their_training_steps_on_the_recorder(which, fused):
    import host_trace
    text, batch = {"net_b": (nets.net_b(), 5), "net_a_linear_dropout": (nets.net_a(nets.LINEAR, dropprob=0.25), 5),
                   "second_writer": (nets.second_writer(), 5), "unread_slice": (nets.unread_slice(), 5),
                   "inception": (models.inception_small(dropprob=0.25), 8), "inception_pooled": (models.inception_small(pooled_branch=True), 8),
                   "wide_net": (nets.wide_net(), 64)}[which]
    lines = host_trace.trace(text, batch, fused)
    assert lines.count("# TrainOneBatch") == 2 and any(l.startswith("get_slice ") for l in lines)
    if which == "second_writer":
        # two writers into h2.a: the second accumulates (scaleTargets 1), exactly as two writers into one layer do
        first_step = lines[:lines.index("# TrainOneBatch", lines.index("# TrainOneBatch") + 1)]
        up = _calls(first_step, "convUpGemm")
        assert len(up) == (3 if fused else 5) and [c[-1] for c in up][-3:] == ["f0x0.0p+0", "f0x0.0p+0", "f0x1.0000000000000p+0"]
    if which == "inception_pooled" and fused:
        assert _calls(lines, "MaxPoolMask") and _calls(lines, "MaxPoolUndoMask")          # the mask pair on a slice view


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------------
class _HostMat:
    """The two Matrix methods a checkpoint uses, on a numpy array in memory order ((cols, rows): column-major)."""

    def __init__(self, a):
        self.a = np.array(a, np.float32)

    def GetNumEls(self):
        return self.a.size

    def WriteHDF5(self, file, name):
        file.WriteHDF5CPU(self.a, self.a.shape[0], self.a.shape[1], name)

    def ReadHDF5(self, file, name):
        self.a.reshape(-1)[:] = file.ReadHDF5CPU(self.a.size, name)


def _with_host_parameters(net, seed):
    rng = np.random.default_rng(seed)
    mats = {}
    for e in net.edges_:
        if hasattr(e, "weight_optimizer_"):
            rows, bias_cols, _ = e._param_layout()
            e.weights_, e.bias_ = _HostMat(rng.standard_normal((e._input_size(), rows))), _HostMat(rng.standard_normal((rows * bias_cols, 1)))
            e.weight_optimizer_.gradient_history_ = _HostMat(rng.standard_normal((e._input_size(), rows)))
            e.bias_optimizer_.gradient_history_ = _HostMat(rng.standard_normal((rows * bias_cols, 1)))
            e.weight_optimizer_.step_ = e.bias_optimizer_.step_ = 7
            mats[e.GetName()] = (e.weights_, e.bias_, e.weight_optimizer_.gradient_history_, e.bias_optimizer_.gradient_history_)
    return mats


@pytest.mark.parametrize("which", ["net_a", "alexnet_grouped_small"])
def test_a_sliced_net_saves_and_loads_every_group(tmp_path, which):
    """ConvNet.Save / Load on a net with two weighted edges between the same two layers: every edge gets its own datasets and gets its own
    parameters and optimizer state back; edges on whole layers keep the reference's dataset names."""
    text = nets.net_a() if which == "net_a" else models.alexnet_grouped(image_size=67, num_classes=10)
    saved_net, loaded_net = ConvNet(text), ConvNet(text)
    saved, loaded = _with_host_parameters(saved_net, 1), _with_host_parameters(loaded_net, 2)
    path = os.path.join(str(tmp_path), "net.h5")
    saved_net.current_iter_ = 5
    saved_net.Save(path)
    assert not os.path.exists(path + "temp")
    names, _ = ref_host.h5_listing(path)
    if which == "net_a":
        assert [n for n in names if n.endswith(":weight")] == sorted(f"{e}:weight" for e in ("input:h1_a", "input:h1_b", "h1_a:h2_a", "h1_b:h2_b",
                                                                                             "pool:output"))
        assert "pool:output:bias_gradient_history" in names and "h1_b:h2_b:bias_gradient_history" in names
    else:
        assert "input:hidden1_conv:weight" in names and "hidden3_conv_a:hidden4_conv_a:weight" in names and "hidden3_conv_b:hidden4_conv_b:weight" in names
    assert len(names) == 4 * len(saved)
    loaded_net.Load(path)
    assert loaded_net.current_iter_ == 5
    groups = [a.a for a, _, _, _ in saved.values()]
    assert all(not np.array_equal(x, y) for i, x in enumerate(groups) for y in groups[i + 1:] if x.shape == y.shape)    # the groups do differ
    for name, mats in saved.items():
        for want, got in zip(mats, loaded[name]):
            assert np.array_equal(want.a, got.a), name
    assert all(e.weight_optimizer_.step_ == 7 for e in loaded_net.edges_ if hasattr(e, "weight_optimizer_"))
