"""CPU: the library calls the host issues — entry, operands, scalars, order — for every net of tests/host_trace.py, fused and unfused,
against tests/golden/host_trace.json (per net and mode: the call count, the SHA-256 of the canonical trace and a three-digit tag per line).

The goldens were recorded from the host as it stood before the per-layer plan (NOTES.md, "Host refactors are checked by call trace") and
are regenerated only by a commit that means to change the call sequence and says so.  On a mismatch the actual trace is written to
pytest's tmp_path; `python tests/host_trace.py NET [--fused]` on the other checkout gives the trace to diff it with."""
import json
import os

import pytest

import host_trace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_trace.json")
NETS = host_trace.nets()
with open(GOLDEN) as f:
    EXPECTED = json.load(f)


def test_goldens_cover_exactly_the_traced_nets():
    assert set(EXPECTED) == {host_trace.key(n, f) for n in NETS for f in (True, False)}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("name", list(NETS))
def test_host_issues_the_recorded_calls(name, fused, tmp_path):
    text, batch = NETS[name]
    lines = host_trace.trace(text, batch, fused)
    want = EXPECTED[host_trace.key(name, fused)]
    got = host_trace.digest(lines)
    if got != want:
        path = tmp_path / "actual_trace.txt"
        path.write_text("\n".join(lines) + "\n")
        a, b = got["lines"], want["lines"]
        first = next((i for i in range(0, min(len(a), len(b)), 3) if a[i:i + 3] != b[i:i + 3]), min(len(a), len(b))) // 3 + 1
        mode = "fused" if fused else "unfused"
        assert got == want, f"{name} ({mode}): {got['calls']} calls, recorded {want['calls']}; first differing line: {first} of {path}"
