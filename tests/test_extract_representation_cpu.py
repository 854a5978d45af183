"""CPU: the pieces of ``ExtractFeatures(config)`` that need no GPU — the two config messages, the restatement of the reference's
DataWriter loop (tests/datawriter_ref.py) against the plain reading of a feature config, the refusals of ``datawriter.plan_streams``
and the create-then-write-rows pair of hdf5io."""
import os

import numpy as np
import pytest

from convnet_amd import hdf5io, pbtxt
from convnet_amd.datawriter import plan_streams
from datawriter_ref import run_extraction

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_feature_messages_parse_with_their_defaults():
    c = pbtxt.parse('output_file: "o.h5"\nfeature { layer: "a" }\nfeature { layer: "b" average_batches: 10 average_online: 3 }\n'
                    'input { batch_size: 8 multiplicity: 10 data_config { layer_name: "input" file_pattern: "x.h5" dataset_name: "d" } }',
                    pbtxt.FeatureExtractorConfig)
    assert c.output_file == "o.h5" and [f.layer for f in c.feature] == ["a", "b"]
    assert (c.feature[0].average_batches, c.feature[0].average_online) == (1, 1) and not c.feature[0].has_average_batches()
    assert (c.feature[1].average_batches, c.feature[1].average_online) == (10, 3)
    assert isinstance(c.input, pbtxt.DatasetConfig) and c.input.multiplicity == 10 and c.input.data_config[0].dataset_name == "d"
    d = pbtxt.FeatureExtractorConfig()
    assert d.output_file == "" and d.feature == [] and d.input.batch_size == 1
    assert pbtxt.parse(pbtxt.dump(c), pbtxt.FeatureExtractorConfig).feature[1].average_online == 3
    with pytest.raises(ValueError, match="no field named 'average'"):
        pbtxt.parse('feature { layer: "a" average: 2 }', pbtxt.FeatureExtractorConfig)


def test_the_mnist_example_config_parses():
    """A copy of the reference's examples/mnist-conv/feature_config.pbtxt (tests/golden)."""
    c = pbtxt.read(os.path.join(GOLDEN, "mnist_conv_feature_config.pbtxt"), pbtxt.FeatureExtractorConfig)
    assert c.output_file == "output.h5" and [f.layer for f in c.feature] == ["output", "hidden2"]
    assert all(f.average_batches == 1 and f.average_online == 1 for f in c.feature)
    s = c.input.data_config[0]
    assert (s.layer_name, s.file_pattern, s.dataset_name, s.data_type) == ("input", "../data/mnist.h5", "test", "HDF5")
    assert c.input.batch_size == 100 and c.input.multiplicity == 1


def _state(B, D):
    """State of (batch, view): row n = (id of column n, view) — columns behind the end of the dataset get ids >= D (padding)."""
    return lambda name, k, view: np.stack([k * B + np.arange(B), np.full(B, view)], axis=1).astype(np.float64)


def _plain_reading(D, B, M, P, G):
    """What a feature config says: every case (in order, batch by batch; within a batch every group of P consecutive views, then the
    batch's real cases) averaged over its P views, then every G consecutive such rows averaged."""
    items = []
    for k in range(-(-D // B)):
        n = min(B, D - k * B)
        for vg in range(M // P):
            items += [(k * B + i, np.mean(np.arange(vg * P, (vg + 1) * P))) for i in range(n)]
    items = np.array(items, np.float64)
    return items.reshape(len(items) // G, G, 2).mean(axis=1)


@pytest.mark.parametrize("D,B,M,P,G", [(21, 8, 1, 1, 1), (24, 8, 1, 1, 3), (20, 8, 10, 10, 1)])
def test_restatement_gives_the_plain_reading_where_the_config_is_supported(D, B, M, P, G):
    """A left-over batch of 5 (and of 4 under ten-view averaging), groups of 3 that straddle the batches of 8."""
    plans = plan_streams([_feature("f", P, G)], D, M, B, lambda name: 2)
    w = run_extraction(D, B, M, {"f": (P, G)}, _state(B, D))
    rows = w.Rows("f")
    assert len(rows) == D * M // (P * G) == plans[0].num_rows == w.NumRows("f")
    assert np.allclose(rows, _plain_reading(D, B, M, P, G), rtol=0, atol=1e-12)
    assert w.streams_["f"].consumed == 0 and w.streams_["f"].counter == 0


def test_restatement_of_the_left_over_batch_under_online_averaging_with_several_views():
    """(D, B, M, P, G) = (20, 8, 10, 5, 2): inside the two divisibility rules, and still not a config the reference can run.  Its loop
    ignores numcases for average_online > 1, and its stop test compares against cases x multiplicity, not divided by average_batches:
    the left-over batch's first averaged buffer walks all 8 columns (4 of them padding) into rows 16..19, its second one goes on to
    row 20 of a dataset of 20 — the reference's failing hyperslab selection.  With average_batches == 1 (stop test exact) the padding
    columns land in the file instead.  plan_streams refuses both."""
    D, B = 20, 8
    with pytest.raises(IndexError, match=r"rows 20:21 of a dataset of 20"):
        run_extraction(D, B, 10, {"f": (5, 2)}, _state(B, D))
    w = run_extraction(D, B, 2, {"f": (1, 2)}, _state(B, D))
    rows = w.Rows("f")
    assert len(rows) == 20 and np.allclose(rows[:18], _plain_reading(D, B, 2, 1, 2)[:18])
    assert rows[18:, 0].tolist() == [20.5, 22.5] and rows[18:, 1].tolist() == [0.0, 0.0]       # padding columns of view 0; view 1 never written
    for M, P in ((10, 5), (2, 1)):
        with pytest.raises(SystemExit, match=r"Feature f: average_online 2 with a partial last batch \(20 cases in batches of 8\)"):
            plan_streams([_feature("f", P, 2)], D, M, B, lambda name: 2)
    # one averaged buffer per input batch: the dataset's end stops the walk right behind the last real case
    assert plan_streams([_feature("f", 10, 2)], D, 10, B, lambda name: 2)[0].num_rows == 10
    assert np.allclose(run_extraction(D, B, 1, {"f": (1, 2)}, _state(B, D)).Rows("f"), _plain_reading(D, B, 1, 1, 2))


def _feature(layer, P=1, G=1):
    f = pbtxt.FeatureStreamConfig()
    f.layer = layer
    if P != 1:
        f.average_batches = P
    if G != 1:
        f.average_online = G
    return f


def test_refusals_name_the_feature():
    dims = {"hidden7": 64}.get
    with pytest.raises(SystemExit, match=r"Feature hidden7: average_batches 4 does not divide the input's multiplicity 10"):
        plan_streams([_feature("hidden7", 4)], 24, 10, 8, dims)
    with pytest.raises(SystemExit, match=r"Feature hidden7: 24 rows .* are not a multiple of average_online 5"):
        plan_streams([_feature("hidden7", 10, 5)], 24, 10, 8, dims)
    with pytest.raises(SystemExit, match=r"Feature conv9: the model has no layer of that name"):
        plan_streams([_feature("hidden7"), _feature("conv9")], 24, 10, 8, dims)
    with pytest.raises(SystemExit, match=r"names no feature"):
        plan_streams([], 24, 10, 8, dims)
    with pytest.raises(SystemExit, match=r"Feature hidden7: named twice"):
        plan_streams([_feature("hidden7"), _feature("hidden7", 10)], 24, 10, 8, dims)
    p = plan_streams([_feature("hidden7", 10, 3)], 24, 10, 8, dims)[0]
    assert (p.layer, p.average_batches, p.average_online, p.num_dims, p.num_rows) == ("hidden7", 10, 3, 64, 8)


def test_create_rows_and_write_rows_round_trip_through_row_reader(tmp_path):
    path = str(tmp_path / "rows.h5")
    a = np.arange(7 * 5, dtype=np.float32).reshape(7, 5) / 4
    with hdf5io.File(path, "w") as f:
        w = f.CreateRows("feat", 7, 5)
        one = f.CreateRows("one", 3, 1)
        w.WriteRows(a[3:5], 3)                                          # out of order, in pieces, one row at a time
        w.WriteRows(a[:3], 0)
        w.WriteRows(a[5:], 5)
        one.WriteRows(np.array([[1.5], [2.5], [3.5]], np.float32), 0)
        with pytest.raises(IndexError, match=r"feat: rows 6:8 are not inside its 7 rows"):
            w.WriteRows(a[:2], 6)
        with pytest.raises(ValueError, match="contiguous float32"):
            w.WriteRows(a[:, :3], 0)
        with pytest.raises(ValueError, match="contiguous float32"):
            w.WriteRows(a.astype(np.float64), 0)
        with pytest.raises(OSError, match="Could not create dataset feat"):
            f.CreateRows("feat", 2, 2)                                  # the name is taken
        w.close()
        with pytest.raises(OSError, match="feat .* is closed"):
            w.WriteRows(a[:1], 0)
        one.close()
    with hdf5io.File(path) as f:
        r = f.RowReader("feat")
        assert (r.GetDataSetSize(), r.GetDims(), r.GetStoredType()) == (7, 5, np.float32)
        out = np.zeros((7, 5), np.float32)
        r.Get(out, 0, 7)
        assert np.array_equal(out, a)
        assert f.ReadHDF5CPU(3, "one").tolist() == [1.5, 2.5, 3.5]      # (and the matrix reader sees a (1, 3) column-major matrix)
        r.close()


def test_hdf5_calls_of_two_threads_never_overlap(tmp_path):
    """The one lock of hdf5io: a reader thread (the data handler's preload) and a writer thread (the data writer's) hammer two files;
    a probe wrapped round H5Dread / H5Dwrite sees at most one thread inside the library at any time."""
    import threading
    src = str(tmp_path / "in.h5")
    data = np.arange(64 * 16, dtype=np.float32).reshape(64, 16)
    with hdf5io.File(src, "w") as f:
        f.WriteDataset("d", data)
    L = hdf5io._lib()
    inside, worst, guard = [0], [0], threading.Lock()
    real = {n: getattr(L, n) for n in ("H5Dread", "H5Dwrite")}

    def probe(fn):
        def call(*a):
            with guard:
                inside[0] += 1
                worst[0] = max(worst[0], inside[0])
            try:
                return fn(*a)
            finally:
                with guard:
                    inside[0] -= 1
        return call

    errors = []

    def reader():
        try:
            with hdf5io.File(src) as f:
                r, out = f.RowReader("d"), np.zeros((8, 16), np.float32)
                for i in range(200):
                    r.Get(out, (i * 8) % 56, (i * 8) % 56 + 8)
                    assert np.array_equal(out, data[(i * 8) % 56:(i * 8) % 56 + 8])
                r.close()
        except BaseException as e:
            errors.append(e)

    def writer():
        try:
            with hdf5io.File(str(tmp_path / "out.h5"), "w") as f:
                w = f.CreateRows("d", 64, 16)
                for i in range(200):
                    w.WriteRows(data[(i * 8) % 64:(i * 8) % 64 + 8], (i * 8) % 64)
                w.close()
        except BaseException as e:
            errors.append(e)

    try:
        for n, fn in real.items():
            setattr(L, n, probe(fn))
        threads = [threading.Thread(target=t) for t in (reader, writer)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        for n, fn in real.items():
            setattr(L, n, fn)
    assert not errors, errors
    assert worst[0] == 1
    with hdf5io.File(str(tmp_path / "out.h5")) as f:
        assert np.array_equal(f.ReadHDF5CPU(64 * 16, "d").reshape(64, 16), data)
