"""CPU: sequence streams (is_sequence) of the DataHandler — the row mapping of SequenceDataIterator, the stream's sizes and refusals, the
float form's materialised clips, the frames-once byte form's host buffer with its first-frame table, and the buffer-size rule.  No GPU
call is made: plain host buffers, DiskAccess on the calling thread."""
import threading

import numpy as np
import pytest

from convnet_amd import hdf5io, pbtxt
from convnet_amd.datahandler import DataHandler, _run_frames, _SequenceReader

FRAMES, FS, T = 14, 6, 3
BOUNDS = [5, 2, 7]
CLIPS = [0, 1, 2, 7, 8, 9, 10, 11]        # written out by hand: 5 frames hold 3 clips of 3, 2 frames none, 7 frames (from 7) hold 5


@pytest.fixture(scope="module")
def seq_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("seq")
    path = str(d / "frames.h5")
    data = ((17 * np.arange(FRAMES)[:, None] + np.arange(FS)) % 251).astype(np.uint8)     # every frame is recognisable by its first value
    with hdf5io.File(path, "w") as f:
        f.WriteDataset("x", data)
        f.WriteDataset("xf", data.astype(np.float32))
        f.WriteDataset("y", np.arange(FRAMES, dtype=np.float32))
    bounds = str(d / "bounds.txt")
    with open(bounds, "w") as f:
        f.write("5\n2\n7\n")
    return path, data, bounds, d


def _config(path, bounds, extra="", stream="", seq=T, dataset="x", labels=True):
    b = f'boundary_file: "{bounds}"' if bounds else ""
    text = (f'data_config {{ file_pattern: "{path}" layer_name: "input" dataset_name: "{dataset}" is_sequence: true seq_length: {seq} {b} {stream} }}\n')
    if labels:
        text += (f'data_config {{ file_pattern: "{path}" layer_name: "output" dataset_name: "y" is_sequence: true seq_length: {seq} {b} '
                 'pick_first: true }\n')
    return pbtxt.parse(text + f"batch_size: 2\n{extra}", pbtxt.DatasetConfig)


def _frame_ids(data, rows):
    return [int(np.flatnonzero((data == np.asarray(r).astype(np.uint8)).all(axis=1))[0]) for r in rows]


# ---- row mapping ------------------------------------------------------------------------------------------------------------------------
def test_row_mapping_by_hand_and_the_skipped_sequence_warns(seq_file, capsys):
    path, data, bounds, _ = seq_file
    dh = DataHandler(_config(path, bounds))
    out = capsys.readouterr().out
    assert "Warning: Number of frames 2 is smaller than sequence length 3 for sequence starting at 5. This sequence will be skipped." in out
    for name in ("input", "output"):
        assert dh.streams_[name].reader_.row_mapping_.tolist() == CLIPS
    assert dh.GetDataSetSize() == 8
    dh.close()
    assert _SequenceReader.SetupRowMapping([5, 2, 7], 3).tolist() == CLIPS
    assert _SequenceReader.SetupRowMapping([3, 3], 3).tolist() == [0, 3] and _SequenceReader.SetupRowMapping([4], 1).tolist() == [0, 1, 2, 3]


def test_no_boundary_file_is_one_sequence(seq_file, capsys):
    path, data, _, _ = seq_file
    dh = DataHandler(_config(path, ""))
    assert "Assuming entire dataset is one sequence" in capsys.readouterr().err
    assert dh.streams_["input"].reader_.row_mapping_.tolist() == list(range(FRAMES - T + 1)) and dh.GetDataSetSize() == 12
    dh.close()


def test_boundary_total_and_unreadable_boundary_file_stop(seq_file):
    path, data, _, d = seq_file
    bad = str(d / "bad.txt")
    with open(bad, "w") as f:
        f.write("5 2 6\n")
    with pytest.raises(SystemExit, match=r"layer input.*Dataset has 14 frames but boundary_file adds up to 13"):
        DataHandler(_config(path, bad))
    with pytest.raises(SystemExit, match=r"layer input.*Could not open boundary file : .*nowhere.txt"):
        DataHandler(_config(path, str(d / "nowhere.txt")))


# ---- stream properties ------------------------------------------------------------------------------------------------------------------
def test_dims_pick_first_and_staged_dims(seq_file):
    path, data, bounds, _ = seq_file
    dh = DataHandler(_config(path, bounds, stream="image_size_y: 1 image_size_x: 3 gpu_image_size_x: 2 num_colors: 2"))
    st, lab = dh.streams_["input"], dh.streams_["output"]
    assert (dh.GetDims("input"), dh.GetDims("output")) == (FS * T, 1)
    assert st.StagedDims() == T * 2 * 1 * 2 and lab.StagedDims() == 1            # the frame factor; none with pick_first
    row = np.zeros((2, 1), np.float32)
    lab.reader_.Get(row, 3, 5)                                                   # pick_first: the first frame of clips 3 and 4
    assert row.reshape(-1).tolist() == [7.0, 8.0]
    dh.close()
    with pytest.raises(SystemExit, match=r"layer input: frames of 6 values are not 3 colours"):
        DataHandler(_config(path, bounds, stream="image_size_y: 1 image_size_x: 3 gpu_image_size_x: 2 num_colors: 3"))


def test_max_dataset_size_goes_to_the_base_reader_only(seq_file):
    """SequenceDataIterator::SetMaxDataSetSize: the clip count stays, the frames beyond it can no longer be read."""
    path, data, bounds, _ = seq_file
    dh = DataHandler(_config(path, bounds, "max_dataset_size: 9"))
    assert dh.GetDataSetSize() == 8 and dh.streams_["input"].reader_.base_.GetDataSetSize() == 9
    out = np.zeros((1, FS * T), np.float32)
    dh.streams_["input"].reader_.Get(out, 2, 3)                                  # frames 2..4
    with pytest.raises(IndexError):
        dh.streams_["input"].reader_.Get(out, 3, 4)                              # frames 7..9: past the base's 9
    dh.close()
    dh = DataHandler(_config(path, bounds))
    assert dh.GetDataSetSize() == 8 and dh.streams_["input"].reader_.base_.GetDataSetSize() == 14
    dh.close()


def test_refusals_are_distinct_and_name_the_layer(seq_file):
    path, data, bounds, _ = seq_file
    messages = set()
    for seq, stream, word in ((0, "", "is_sequence"), (-2, "", "is_sequence"), (3, "pca_noise_stddev: 0.1", "pca_noise_stddev"),
                              (3, "data_type: VIDEO_RAW", "data_type VIDEO_RAW"), (3, 'noise_layer_name: "output"', "noise_layer_name"),
                              (3, "gpu_id: 1", "gpu_id 1"), (8, "", "no sequence holds")):
        with pytest.raises(SystemExit) as e:
            DataHandler(_config(path, bounds, stream=stream, seq=seq))
        assert word in str(e.value) and "layer input" in str(e.value), (seq, stream)
        messages.add(str(e.value).replace("-2", "0"))
    assert len(messages) == 6                                                    # (the two seq_length cases share theirs)


# ---- the float form: materialised clips -------------------------------------------------------------------------------------------------
def _clip_rows(chunk, data):
    x = np.asarray(chunk["input"]).reshape(-1, T, FS)
    firsts = []
    for clip in x:
        ids = _frame_ids(data, clip)
        assert ids == list(range(ids[0], ids[0] + T))                            # T consecutive frames
        firsts.append(ids[0])
    assert np.asarray(chunk["output"]).reshape(-1).tolist() == firsts            # pick_first labels: the first frame's
    return firsts


@pytest.mark.parametrize("dataset", ["x", "xf"])
def test_float_form_clips_are_numpy_indexed_frames_across_the_wrap(seq_file, dataset):
    path, data, bounds, _ = seq_file
    dh = DataHandler(_config(path, bounds, "chunk_size: 5", dataset=dataset), raw_chunks=False)
    dh.SetInputLayers(["input"])
    dh.AllocateHostMemory(pinned=False)
    assert dh.host_[0]["input"].shape == (5, FS * T) and dh.host_[0]["input"].dtype == np.float32
    want = [[0, 1, 2, 7, 8], [9, 10, 11, 0, 1], [2, 7, 8, 9, 10]]
    for chunk in want:
        host = dh.DiskAccess()
        assert _clip_rows(host, data) == chunk
        assert np.array_equal(host["input"], np.stack([data[f:f + T].reshape(-1) for f in chunk]).astype(np.float32))
    dh.close()


def test_float_form_under_randomize_cpu_reads_runs_of_clip_rows(seq_file):
    path, data, bounds, _ = seq_file
    dh = DataHandler(_config(path, bounds, "chunk_size: 6 randomize_cpu: true random_access_chunk_size: 4"), raw_chunks=False, seed=3)
    for _ in range(5):
        firsts = _clip_rows(dh.DiskAccess(), data)
        rows = [CLIPS.index(f) for f in firsts]
        for run in (rows[:4], rows[4:]):                                         # a run of 4 and one cut to 2, consecutive CLIP rows modulo 8
            assert run == [(run[0] + k) % 8 for k in range(len(run))]
    dh.close()


# ---- the bytes form: every frame once ---------------------------------------------------------------------------------------------------
def _once(path, bounds, extra, seed=0):
    dh = DataHandler(_config(path, bounds, extra), seed=seed)
    dh.SetInputLayers(["input"])
    dh.AllocateHostMemory(pinned=False)
    st = dh.streams_["input"]
    assert st.raw_ and st.frames_once_ and not dh.streams_["output"].raw_
    return dh


def _access(dh, data):
    host = dh.DiskAccess()
    used = dh.disk_.frames_used_[0]["input"]
    table = dh.disk_.first_frame_[0]["input"]
    assert host["input"].dtype == np.uint8 and host["input"].shape[1] == FS and used <= host["input"].shape[0]
    frames = _frame_ids(data, host["input"][:used])
    labels = np.asarray(host["output"]).reshape(-1)
    for i in range(dh.chunk_size_):                                              # buffer[table[i] : table[i] + T] is clip i's frames
        at = int(table[i])
        assert table[i] == at and frames[at:at + T] == list(range(int(labels[i]), int(labels[i]) + T)), i
    return frames, table.astype(int).tolist(), labels.astype(int).tolist()


def test_frames_once_sequential_chunks_by_hand(seq_file):
    path, data, bounds, _ = seq_file
    dh = _once(path, bounds, "chunk_size: 5")
    # worst run of 5 clip rows: rows 2..6 (2 | 7 8 9 10) or 3 rows + wrap ...: 3 + 3 + 1 + 1 + 3 = 11 at the most
    assert dh.FrameBufferSize("input") == 11 and dh.host_[0]["input"].shape == (11, FS)
    # clips 0 1 2 | 7 8: crosses the boundary and the skipped sequence (frames 5, 6 are never read)
    assert _access(dh, data) == ([0, 1, 2, 3, 4, 7, 8, 9, 10], [0, 1, 2, 5, 6], [0, 1, 2, 7, 8])
    # clips 9 10 11 | 0 1: wraps to row 0
    assert _access(dh, data) == ([9, 10, 11, 12, 13, 0, 1, 2, 3], [0, 1, 2, 5, 6], [9, 10, 11, 0, 1])
    # clips 2 | 7 8 9 10
    assert _access(dh, data) == ([2, 3, 4, 7, 8, 9, 10, 11, 12], [0, 3, 4, 5, 6], [2, 7, 8, 9, 10])
    reads = dh.streams_["input"].reader_.num_reads_
    assert reads == 6                                                            # two pieces a chunk: one hyperslab read each
    dh.close()


def test_frames_once_boundary_without_a_skipped_sequence(seq_file):
    path, data, _, d = seq_file
    bounds = str(d / "b2.txt")
    with open(bounds, "w") as f:
        f.write("4 10")
    dh = _once(path, bounds, "chunk_size: 4")
    assert dh.streams_["input"].reader_.row_mapping_.tolist() == [0, 1, 4, 5, 6, 7, 8, 9, 10, 11]
    # clips 0 1 | 4 5: a new piece at the boundary although the frames go on (0..3, then 4..7)
    assert _access(dh, data) == ([0, 1, 2, 3, 4, 5, 6, 7], [0, 1, 4, 5], [0, 1, 4, 5])
    assert dh.streams_["input"].reader_.num_reads_ == 2
    dh.close()


def test_frames_once_random_runs_by_hand(seq_file):
    path, data, bounds, _ = seq_file
    dh = _once(path, bounds, "chunk_size: 5 randomize_cpu: true random_access_chunk_size: 2", seed=1)
    # runs of 2, 2 and 1 clip rows; the worst run of 2 is 3 + 3 (rows 2, 3 or the wrap), of 1 is 3
    assert dh.FrameBufferSize("input") == 6 + 6 + 3
    dh.disk_.random_indices_ = np.array([1, 2, 7, 0, 3, 4, 5, 6])                # rows 1 2 | 2 3 | 7: clips 1 2 | 2 7 | 11
    dh.disk_.random_indices_ind_ = 0
    frames, table, labels = _access(dh, data)
    assert labels == [1, 2, 2, 7, 11]
    assert frames == [1, 2, 3, 4, 2, 3, 4, 7, 8, 9, 11, 12, 13]                  # runs follow each other: frames 2 3 4 are stored twice
    assert table == [0, 1, 4, 7, 10]
    dh.disk_.random_indices_ = np.array([7, 0, 3, 1, 2, 4, 5, 6])                # a run that wraps: rows 7 0 -> clips 11 | 0
    dh.disk_.random_indices_ind_ = 0
    frames, table, labels = _access(dh, data)
    assert labels == [11, 0, 0, 1, 7] and frames == [11, 12, 13, 0, 1, 2, 0, 1, 2, 3, 7, 8, 9] and table == [0, 3, 6, 7, 10]
    dh.close()


def test_pick_first_and_float_datasets_keep_the_float_form(seq_file):
    path, data, bounds, _ = seq_file
    dh = DataHandler(_config(path, bounds, stream="pick_first: true", labels=False))
    dh.SetInputLayers(["input"])
    assert not dh.streams_["input"].raw_ and dh.GetDims("input") == FS
    dh.close()
    for kw in (dict(dataset="xf"), dict(stream="normalize_local: true")):
        dh = DataHandler(_config(path, bounds, **kw))
        dh.SetInputLayers(["input"])
        assert not dh.streams_["input"].raw_ and not dh.streams_["input"].frames_once_
        dh.close()


# ---- the buffer-size rule ---------------------------------------------------------------------------------------------------------------
def _brute_force(mapping, seq, length):
    """The frames a run of ``length`` clip rows lays down, by the rule itself, for every start."""
    worst, D = 0, len(mapping)
    for s in range(D):
        rows = [(s + k) % D for k in range(length)]
        frames = seq
        for a, b in zip(rows, rows[1:]):
            frames += 1 if (b == a + 1 and mapping[b] == mapping[a] + 1) else seq
        worst = max(worst, frames)
    return worst


def test_buffer_size_is_the_exact_worst_case_and_is_never_exceeded(tmp_path):
    rng = np.random.default_rng(2024)
    for k in range(20):
        seq = int(rng.integers(1, 6))
        bounds = rng.integers(1, 12, int(rng.integers(1, 7))).tolist()
        if max(bounds) < seq:
            bounds[0] = seq + 2
        total = int(sum(bounds))
        path, bfile = str(tmp_path / f"f{k}.h5"), str(tmp_path / f"b{k}.txt")
        data = np.arange(total, dtype=np.uint8).reshape(total, 1)
        with hdf5io.File(path, "w") as f:
            f.WriteDataset("x", data)
        with open(bfile, "w") as f:
            f.write(" ".join(map(str, bounds)))
        mapping = _SequenceReader.SetupRowMapping(bounds, seq)
        D = len(mapping)
        chunk = int(rng.integers(1, D + 1))
        racs = int(rng.integers(1, chunk + 2))
        random = bool(k % 2)
        extra = f"chunk_size: {chunk}" + (f" randomize_cpu: true random_access_chunk_size: {racs}" if random else "")
        cfg = pbtxt.parse(f'data_config {{ file_pattern: "{path}" layer_name: "input" dataset_name: "x" is_sequence: true seq_length: {seq} '
                          f'boundary_file: "{bfile}" }}\nbatch_size: 1\n{extra}', pbtxt.DatasetConfig)
        dh = DataHandler(cfg, seed=k)
        dh.SetInputLayers(["input"])
        dh.AllocateHostMemory(pinned=False)
        chunk = dh.chunk_size_
        if random:
            whole, last = divmod(chunk, racs)
            want = whole * _brute_force(mapping, seq, min(racs, chunk)) + (_brute_force(mapping, seq, last) if last else 0)
        else:
            want = _brute_force(mapping, seq, chunk)
        for length in range(1, D + 1):
            assert _run_frames(mapping, seq, length) == _brute_force(mapping, seq, length), (k, length)
        assert dh.FrameBufferSize("input") == want == dh.host_[0]["input"].shape[0], (k, bounds, seq, extra)
        for _ in range(50):
            host = dh.DiskAccess()
            used, table = dh.disk_.frames_used_[0]["input"], dh.disk_.first_frame_[0]["input"].astype(int)
            assert used <= want
            buf = host["input"][:used, 0].astype(int)
            for i in range(chunk):                                               # every clip is seq consecutive frames, inside the used prefix
                clip = buf[table[i]:table[i] + seq]
                assert len(clip) == seq and (np.diff(clip) == 1).all() and int(clip[0]) in mapping
        dh.close()


# ---- the preload thread -----------------------------------------------------------------------------------------------------------------
def test_preload_thread_fills_the_other_frame_buffer_and_is_joined(seq_file):
    path, data, bounds, _ = seq_file
    before = threading.active_count()
    dh = DataHandler(_config(path, bounds, "chunk_size: 5 pipeline_loads: true"))
    dh.SetInputLayers(["input"])
    dh.AllocateHostMemory(pinned=False)
    assert len(dh.host_) == 2 and len(dh.disk_.first_frame_) == 2
    dh.StartPreload()
    with pytest.raises(SystemExit, match="previous one is still running"):
        dh.StartPreload()
    dh.Sync()
    buf = dh.pending_
    assert threading.active_count() == before and dh.disk_.frames_used_[buf]["input"] == 9
    assert _frame_ids(data, dh.host_[buf]["input"][:9]) == [0, 1, 2, 3, 4, 7, 8, 9, 10]
    assert dh.disk_.first_frame_[buf]["input"].tolist() == [0, 1, 2, 5, 6]
    dh.StartPreload()
    dh.close()
    assert threading.active_count() == before
