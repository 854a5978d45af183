"""CPU: what DataHandler and ChunkDataHandler do — library calls, arrays uploaded, disk reads, host buffers — for every config of
tests/datahandler_trace.py, against tests/golden/datahandler_trace.json (per config: the call count, the SHA-256 of the canonical trace
and a three-digit tag per line).

The goldens were recorded from convnet_amd/datahandler.py as it stood before each chunk form became a class (NOTES.md, "The data handler
is checked by call trace") and are regenerated only by a commit that means to change what a handler does and says so.  On a mismatch the
actual trace is written to pytest's tmp_path; `python tests/datahandler_trace.py CONFIG` on the other checkout gives the trace to diff
it with."""
import json
import os

import pytest

import datahandler_trace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datahandler_trace.json")
with open(GOLDEN) as f:
    EXPECTED = json.load(f)


@pytest.fixture(scope="module")
def configs(tmp_path_factory):
    return datahandler_trace.configs(datahandler_trace.write_files(str(tmp_path_factory.mktemp("traced"))))


def test_goldens_cover_exactly_the_traced_configs(configs):
    assert set(EXPECTED) == set(configs)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_data_handler_does_what_was_recorded(name, configs, tmp_path):
    lines = datahandler_trace.trace(configs[name])
    want = EXPECTED[name]
    got = datahandler_trace.digest(lines)
    if got != want:
        path = tmp_path / "actual_trace.txt"
        path.write_text("\n".join(lines) + "\n")
        a, b = got["lines"], want["lines"]
        first = next((i for i in range(0, min(len(a), len(b)), 3) if a[i:i + 3] != b[i:i + 3]), min(len(a), len(b))) // 3 + 1
        assert got == want, f"{name}: {got['calls']} calls, recorded {want['calls']}; first differing line: {first} of {path}"
