"""What the emulated test files share: kernel sources of convnet_amd/csrc compiled as host C++ against tests/emu/hip/hip_runtime.h, linked
with a main of tests/emu, run, and the program's lines.  A plain module (tests/ is on the path), no fixture of its own."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "convnet_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-x", "c++", "-I", EMU, "-I", CSRC, "-Wno-everything"]


def clang():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    return None


def build(out_dir, kernels, main, why, extras=None, link_args=()):
    """Compiles ``kernels`` (files of convnet_amd/csrc), the library's own state.hip (stream, arenas, deferred epilogues, kernel report:
    no program has a stand-in for it) and ``main`` (a file of tests/emu), all at once, and links them in ``out_dir``; returns the
    program's path.  ``extras``: file name -> further compile arguments; ``link_args`` go behind the objects.  Without a clang++ the
    test is skipped; ``why`` says what the kernels need it for."""
    cc = clang()
    if not cc:
        pytest.skip(f"no clang++ ({why})")
    jobs = [(os.path.join(CSRC, f), os.path.join(str(out_dir), f + ".o")) for f in ["state.hip", *kernels]]
    jobs.append((os.path.join(EMU, main), os.path.join(str(out_dir), main + ".o")))
    procs = [subprocess.Popen([cc, *FLAGS, *(extras or {}).get(os.path.basename(src), []), "-c", src, "-o", obj], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for src, obj in jobs]
    for p, (src, _) in zip(procs, jobs):
        out, _ = p.communicate()
        assert p.returncode == 0, src + "\n" + out
    exe = os.path.join(str(out_dir), os.path.splitext(main)[0])
    subprocess.run([cc, *[obj for _, obj in jobs], "-o", exe, *link_args], check=True)
    return exe


def run(exe, *args, timeout=600):
    """Runs the program and returns the lines it printed: its exit status must be 0 and its last line ALL PASSED."""
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert r.returncode == 0 and lines and lines[-1] == "ALL PASSED", r.stdout + r.stderr
    return lines
