"""The one recipe of convnet_amd/lib/libconvnet_hip.so (the C-ABI library declared in include/convnet_hip.h), built from
convnet_amd/csrc/*.hip with hipcc for gfx950, and of its variants lib/libconvnet_hip_<tag>.so for same-call A/B runs through
CONVNET_HIP_LIB (convnet_amd/_lib.py).  hipcc cross-compiles without a GPU; the libraries stay in-tree (git-ignored) so they travel
to the GPU box with the snapshot.  plan() says what would be run, run() runs it, listings() writes a plan's kernels as assembly.

  python -m convnet_amd.build [--force]                  the product
  python -m convnet_amd.build --diag                     libconvnet_hip_diag.so: the experiment knobs (-DCONVNET_DIAG) compiled in
  python -m convnet_amd.build --tag early --flags "-DCONVNET_GPV_FILT_LATE=0"     a compile-time choice
  python -m convnet_amd.build --rev 256646b [--tag r03]  that revision's sources by that revision's recipe
  python -m convnet_amd.build --listings DIR [--rev REV | --flags "..."]          no library: DIR/<source>/<symbol>.s
`diff -r` of two listing directories is the check a refactor of csrc/ has to show: same symbols, every file identical."""
import argparse
import collections
import concurrent.futures
import glob
import os
import pathlib
import re
import runpy
import shlex
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "lib")
OUT = os.path.join(LIB, "libconvnet_hip.so")
SOURCES = ["state.hip", "gather_gemm.hip", "patch_gemm.hip", "wgrad_wide.hip", "fewc_conv.hip", "local_conv.hip", "conv3d.hip", "batch_norm.hip", "pool_norm.hip", "resample.hip", "elementwise.hip", "input_staging.hip", "dataset_moments.hip", "feature_rows.hip", "comm.hip", "rccl_abi_check.hip", "probe.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment", "-Wno-inline-asm"]
# Per-file additions.  patch_gemm.hip: the SLP vectoriser packs the split's fp32 subtractions into v_pk_add_f32 (+ the v_mov / s_nop
# that feed them) — fewer instructions on paper, but beside MFMAs a packed fp32 op costs more issue time than the two plain ones
# (MI355X_MICROARCH.md), and gpw_kernel's one wave per SIMD has nobody to hide it: 177 instead of 191 VALU + 10 s_nop per chunk.
FILE_FLAGS = {"patch_gemm.hip": ["-fno-slp-vectorize"], "wgrad_wide.hip": ["-fno-slp-vectorize"], "fewc_conv.hip": ["-fno-slp-vectorize"]}
# CONVNET_BUILD_NOSLP=1: the same for gather_gemm.hip (ggp_kernel's consumers and wg_kernel run the same split) — an A/B for the next
# round with hardware, not the product build: the default kernels were measured and parity-tested as compiled without it.
if os.environ.get("CONVNET_BUILD_NOSLP"):
    FILE_FLAGS["gather_gemm.hip"] = ["-fno-slp-vectorize"]
# CONVNET_BUILD_DIAG=1: compile the experiment knobs of csrc/common.h (CHIP_DIAG_KNOB) into the library.  Never set for the product.
if os.environ.get("CONVNET_BUILD_DIAG"):
    FLAGS.append("-DCONVNET_DIAG")

# compiles: source name -> command, in link order (a command ends "-c <source> -o <object>"); link: the command that writes `out`
Plan = collections.namedtuple("Plan", "out compiles link")


def plan(tag="", flags=(), recipe=None, csrc=SRC, lib=LIB, objdir=None, cc="hipcc"):
    """The exact commands of one library: the product's, or with a ``tag`` lib/libconvnet_hip_<tag>.so with ``flags`` added to every
    compile.  ``recipe``: another (SOURCES, FLAGS, FILE_FLAGS), for the sources under ``csrc``.  Every library has its own objects."""
    sources, base, per_file = recipe or (SOURCES, FLAGS, FILE_FLAGS)
    objdir = objdir or os.path.join(lib, "obj_" + tag if tag else "obj")
    compiles = {s: [cc, *base, *flags, *per_file.get(s, []), "-c", os.path.join(csrc, s), "-o", os.path.join(objdir, s.replace(".hip", ".o"))]
                for s in sources}
    out = os.path.join(lib, f"libconvnet_hip_{tag}.so" if tag else "libconvnet_hip.so")
    return Plan(out, compiles, [cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, *(c[-1] for c in compiles.values()), "-ldl"])


def _fresh(target, cmd, deps):
    """``target`` was made by exactly ``cmd`` (recorded beside it) and no dependency is newer"""
    try:
        made_by, t = pathlib.Path(target + ".cmd").read_text(), os.path.getmtime(target)
    except OSError:
        return False
    return made_by == "\n".join(cmd) and not any(os.path.getmtime(d) > t for d in deps)


def run(p, force=False, verbose=False):
    """Runs what of the plan is not up to date, every compile at once, and returns the library's path.  An object depends on its
    command, its source, every header beside the source and include/convnet_hip.h; the library on its command and its objects.  A
    failed compile raises before anything is linked."""
    csrc = os.path.dirname(next(iter(p.compiles.values()))[-3])
    headers = glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(csrc, "..", "..", "include", "convnet_hip.h")]
    todo = [cmd for cmd in p.compiles.values() if force or not _fresh(cmd[-1], cmd, [cmd[-3]] + headers)]
    procs = []
    for cmd in todo:
        os.makedirs(os.path.dirname(cmd[-1]), exist_ok=True)
        pathlib.Path(cmd[-1] + ".cmd").unlink(missing_ok=True)   # until it has compiled, the object is nobody's
        if verbose:
            print(" ".join(cmd))
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    failed = False
    for cmd, proc in zip(todo, procs):
        out, _ = proc.communicate()
        if proc.returncode != 0:
            failed = True
            print(f"--- {os.path.basename(cmd[-3])} failed ---\n{out}", file=sys.stderr)
        else:
            pathlib.Path(cmd[-1] + ".cmd").write_text("\n".join(cmd))
            if verbose and out.strip():
                print(out)
    if failed:
        raise RuntimeError("hipcc failed")
    if force or todo or not _fresh(p.out, p.link, [c[-1] for c in p.compiles.values()]):
        os.makedirs(os.path.dirname(p.out), exist_ok=True)
        r = subprocess.run(p.link, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout, r.stderr, file=sys.stderr)
            raise RuntimeError("link failed")
        pathlib.Path(p.out + ".cmd").write_text("\n".join(p.link))
    return p.out


def build(force=False, verbose=False):
    return run(plan(), force, verbose)


def at_revision(rev, tmp, repo=os.path.dirname(HERE)):
    """Unpacks ``rev``'s recipe and sources into ``tmp``; returns that revision's (SOURCES, FLAGS, FILE_FLAGS), as the product has
    them (the environment switches unset), and its csrc directory."""
    tree = subprocess.run(["git", "-C", repo, "archive", rev, "convnet_amd/build.py", "convnet_amd/csrc", "include"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", tmp], input=tree, check=True)
    switches = {k: os.environ.pop(k) for k in ("CONVNET_BUILD_NOSLP", "CONVNET_BUILD_DIAG") if k in os.environ}
    try:
        theirs = runpy.run_path(os.path.join(tmp, "convnet_amd", "build.py"))
    finally:
        os.environ.update(switches)
    return (theirs["SOURCES"], theirs["FLAGS"], theirs.get("FILE_FLAGS", {})), os.path.join(tmp, "convnet_amd", "csrc")


def device_asm(cmd):
    """The gfx950 assembly of the compile command ``cmd``: the same flags with --cuda-device-only -S"""
    return subprocess.run([*cmd[:-4], "--cuda-device-only", "-S", cmd[-3], "-o", "-"], check=True, capture_output=True, text=True).stdout


def split_listing(asm):
    """symbol -> its lines: the function with its .amdhsa_* block and resource lines.  What differs between identical kernels is gone:
    comments, the __hip_cuid_<hash> object, the function's index in local labels (.LBB6_3 / .LBB9_3).  "_module": the rest."""
    parts, name = collections.defaultdict(list), "_module"
    for line in asm.splitlines():
        begin = re.search(r"; -- Begin function (\S+)", line)
        if begin:
            name = begin.group(1)
        elif re.match(r"\s*\.(p2alignl|amdgpu_metadata)\b", line):   # behind the last function: the code-end padding, the metadata
            name = "_module"
        if '"' not in line:
            line = line.split(";")[0].rstrip()
        if line.strip() and "__hip_cuid_" not in line:
            parts[name].append(re.sub(r"\.L(BB|func_begin|func_end|JTI|CPI)\d+", r".L\1", line))
    return parts


def listings(p, out_dir):
    """out_dir/<source>/<symbol>.s for every source of the plan, each compiled with its own flags"""
    with concurrent.futures.ThreadPoolExecutor(len(p.compiles)) as pool:   # every compile at once, as in run()
        asms = list(pool.map(device_asm, p.compiles.values()))
    for s, asm in zip(p.compiles, asms):
        d = os.path.join(out_dir, s)
        os.makedirs(d, exist_ok=True)
        for name, lines in split_listing(asm).items():
            pathlib.Path(d, name + ".s").write_text("\n".join(lines) + "\n")
    return out_dir


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--force", action="store_true", help="compile and link everything again")
    ap.add_argument("--diag", action="store_true", help='the tag "diag" with -DCONVNET_DIAG')
    ap.add_argument("--tag", default="", help="build lib/libconvnet_hip_<tag>.so")
    ap.add_argument("--flags", default="", help="further flags for every compile (with --tag)")
    ap.add_argument("--rev", help="the sources and the recipe of this revision; the tag defaults to its abbreviated name")
    ap.add_argument("--listings", metavar="DIR", help="write one assembly file per kernel symbol instead of building")
    a = ap.parse_args(argv)
    tag, flags = a.tag, shlex.split(a.flags)
    if a.diag:
        tag, flags = tag or "diag", flags + ["-DCONVNET_DIAG"]
    with tempfile.TemporaryDirectory() as tmp:
        there = {}
        if a.rev:
            recipe, csrc = at_revision(a.rev, tmp)
            tag = tag or subprocess.run(["git", "-C", HERE, "rev-parse", "--short", a.rev], check=True, capture_output=True, text=True).stdout.strip()
            there = dict(recipe=recipe, csrc=csrc, objdir=os.path.join(tmp, "obj"))
        if flags and not tag and not a.listings:
            ap.error("--flags needs --tag: the untagged library is the product")
        p = plan(tag, flags, **there)
        print(listings(p, a.listings) if a.listings else run(p, force=a.force, verbose=True))


if __name__ == "__main__":
    main()
