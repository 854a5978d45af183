"""convnet_amd/build.py is the one recipe of the library and of its variants: what its plan says and what its run reuses, with a
recording stand-in for the compiler (it logs its arguments and creates its -o file), so nothing is compiled here."""
import json
import os
import subprocess
import sys
import time

import pytest

from convnet_amd import build as B


class Tree:
    """A source tree of two files and a header under ``root``, a recipe for it, and the stand-in compiler's log"""
    recipe = (["a.hip", "b.hip"], ["-O3", "-fPIC"], {"b.hip": ["-fno-slp-vectorize"]})

    def __init__(self, root):
        self.root, self.csrc, self.lib, self.log = str(root), str(root / "convnet_amd" / "csrc"), str(root / "lib"), str(root / "cc.log")
        os.makedirs(self.csrc)
        os.makedirs(str(root / "include"))
        for f in ("a.hip", "b.hip", "common.h", "../../include/convnet_hip.h"):
            open(os.path.join(self.csrc, f), "w").close()
        self.cc = str(root / "cc")
        with open(self.cc, "w") as f:   # fails on a command that names what the file "fail" beside it holds
            f.write(f"#!{sys.executable}\nimport json, os, sys\nhere = os.path.dirname(os.path.abspath(__file__))\n"
                    "open(os.path.join(here, 'cc.log'), 'a').write(json.dumps(sys.argv) + '\\n')\n"
                    "fail = os.path.join(here, 'fail')\n"
                    "if os.path.exists(fail) and open(fail).read() in ' '.join(sys.argv): sys.exit('stand-in: told to fail')\n"
                    "open(sys.argv[sys.argv.index('-o') + 1], 'w').close()\n")
        os.chmod(self.cc, 0o755)

    def plan(self, tag="", flags=(), recipe=None):
        return B.plan(tag, flags, recipe=recipe or self.recipe, csrc=self.csrc, lib=self.lib, cc=self.cc)

    def ran(self):
        """(compile commands by object name: they run at once; link commands) since the last look"""
        cmds = [json.loads(l) for l in open(self.log)] if os.path.exists(self.log) else []
        open(self.log, "w").close()
        return sorted((c for c in cmds if "-c" in c), key=lambda c: c[-1]), [c for c in cmds if "-shared" in c]


@pytest.fixture
def tree(tmp_path):
    return Tree(tmp_path)


def test_product_plan_is_the_recipe_per_file():
    p = B.plan()
    assert list(p.compiles) == B.SOURCES and p.out == B.OUT == os.path.join(B.HERE, "lib", "libconvnet_hip.so")
    objs = [os.path.join(B.HERE, "lib", "obj", s.replace(".hip", ".o")) for s in B.SOURCES]
    for s, obj in zip(B.SOURCES, objs):
        assert p.compiles[s] == ["hipcc", *B.FLAGS, *B.FILE_FLAGS.get(s, []), "-c", os.path.join(B.SRC, s), "-o", obj]
    assert p.link == ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", B.OUT, *objs, "-ldl"]
    for s in ("patch_gemm.hip", "wgrad_wide.hip", "fewc_conv.hip"):   # the three hottest files: what a second recipe once dropped
        assert "-fno-slp-vectorize" in p.compiles[s]
    assert "-fno-slp-vectorize" not in p.compiles["state.hip"] and "--offload-arch=gfx950" in p.compiles["state.hip"]
    diag = B.plan("diag", ["-DCONVNET_DIAG"])   # what --diag builds: the product's commands with the one flag, objects of its own
    assert diag.out == os.path.join(B.HERE, "lib", "libconvnet_hip_diag.so")
    for s in B.SOURCES:
        assert [a for a in diag.compiles[s][:-1] if a != "-DCONVNET_DIAG"] == p.compiles[s][:-1] and "-DCONVNET_DIAG" in diag.compiles[s]
        assert diag.compiles[s][-1] != p.compiles[s][-1]


def test_a_variant_build_leaves_the_product_alone(tree):
    product, diag = tree.plan(), tree.plan("diag", ["-DCONVNET_DIAG"])
    assert B.run(product) == os.path.join(tree.lib, "libconvnet_hip.so") and os.path.exists(product.out)
    compiles, links = tree.ran()
    assert compiles == list(product.compiles.values()) and links == [product.link]
    assert B.run(diag) == os.path.join(tree.lib, "libconvnet_hip_diag.so")
    made_by = {c[-1]: c for c in compiles + tree.ran()[0]}   # object -> the command that last wrote it
    B.run(product)
    assert tree.ran() == ([], [])   # nothing to do ...
    assert not any("-DCONVNET_DIAG" in made_by[obj] for obj in product.link if obj.endswith(".o"))   # ... and the library's objects are its own
    assert all("-DCONVNET_DIAG" in made_by[obj] for obj in diag.link if obj.endswith(".o"))


def test_a_changed_flag_or_a_touched_header_recompiles_every_object(tree):
    B.run(tree.plan())
    tree.ran()
    sources, flags, per_file = tree.recipe
    switched = tree.plan(recipe=(sources, flags + ["-DCONVNET_DIAG"], per_file))   # an environment switch: same library, same objects
    B.run(switched)
    assert tree.ran() == (list(switched.compiles.values()), [switched.link])
    B.run(tree.plan())
    assert tree.ran() == (list(tree.plan().compiles.values()), [tree.plan().link])
    later = time.time() + 10
    os.utime(os.path.join(tree.csrc, "common.h"), (later, later))
    B.run(tree.plan())
    assert tree.ran() == (list(tree.plan().compiles.values()), [tree.plan().link])
    # one touched source: that object alone, and the link
    for p in tree.plan().compiles.values():
        os.utime(p[-1], (later, later))
    os.utime(tree.plan().out, (later, later))
    os.utime(os.path.join(tree.csrc, "b.hip"), (later + 10, later + 10))
    B.run(tree.plan())
    assert tree.ran() == ([tree.plan().compiles["b.hip"]], [tree.plan().link])
    # a source fewer: nothing compiles, the library is linked from the shorter list
    fewer = tree.plan(recipe=(["a.hip"], flags, per_file))
    B.run(fewer)
    assert tree.ran() == ([], [fewer.link])


def test_a_failed_compile_raises_and_links_nothing(tree):
    with open(os.path.join(tree.root, "fail"), "w") as f:
        f.write("b.hip")
    with pytest.raises(RuntimeError):
        B.run(tree.plan())
    compiles, links = tree.ran()
    assert len(compiles) == 2 and links == [] and not os.path.exists(tree.plan().out)
    os.remove(os.path.join(tree.root, "fail"))
    B.run(tree.plan())   # the object of the failed compile is not taken for a finished one
    assert tree.ran() == ([tree.plan().compiles["b.hip"]], [tree.plan().link])


def test_rev_takes_the_flags_of_that_revision(tree, tmp_path, monkeypatch):
    def git(*args):
        subprocess.run(["git", "-C", tree.root, "-c", "user.name=t", "-c", "user.email=t@example.org", *args], check=True, capture_output=True)
    with open(os.path.join(tree.root, "convnet_amd", "build.py"), "w") as f:
        f.write('import os\nSOURCES = ["a.hip"]\nFLAGS = ["-O1", "-DTHEIRS"]\nif os.environ.get("CONVNET_BUILD_DIAG"):\n    FLAGS.append("-DCONVNET_DIAG")\n'
                'if __name__ == "__main__":\n    raise SystemExit("a recipe is read, not run")\n')
    git("init", "-q")
    git("add", "convnet_amd", "include")
    git("commit", "-q", "-m", "theirs")
    monkeypatch.setenv("CONVNET_BUILD_DIAG", "1")   # the switch is for this tree's product, never for a revision's
    there = tmp_path / "there"
    there.mkdir()
    recipe, csrc = B.at_revision("HEAD", str(there), repo=tree.root)
    assert recipe == (["a.hip"], ["-O1", "-DTHEIRS"], {}) and os.environ["CONVNET_BUILD_DIAG"] == "1"   # (no FILE_FLAGS there: none)
    assert csrc == str(there / "convnet_amd" / "csrc") and os.path.exists(there / "include" / "convnet_hip.h")
    p = B.plan("theirs", recipe=recipe, csrc=csrc, lib=tree.lib, objdir=str(there / "obj"), cc=tree.cc)
    assert B.run(p) == os.path.join(tree.lib, "libconvnet_hip_theirs.so")
    assert tree.ran() == ([[tree.cc, "-O1", "-DTHEIRS", "-c", os.path.join(csrc, "a.hip"), "-o", str(there / "obj" / "a.o")]], [p.link])


def test_listings_of_the_same_kernel_at_another_place_are_equal():
    def asm(index, cuid, first):
        kernel = (f"\t.protected\tkern ; -- Begin function kern\nkern:\n; %bb.0:\n\ts_cbranch_scc1 .LBB{index}_2 ; a comment\n.LBB{index}_2:\n\ts_endpgm\n"
                  f"\t.amdhsa_kernel kern\n\t\t.amdhsa_next_free_vgpr 8\n\t.end_amdhsa_kernel\n.Lfunc_end{index}:\n\t.size\tkern, .Lfunc_end{index}-kern\n\t; -- End function\n")
        other = "\t.globl\tother ; -- Begin function other\nother:\n\ts_endpgm\n"
        return ("\t.text\n" + (kernel + other if first else other + kernel) + f"\t.p2alignl 6, 3212836864\n\t.type\t__hip_cuid_{cuid},@object\n\t.amdgpu_metadata\n"
                "    .name: kern\n\t.end_amdgpu_metadata\n")
    a, b = B.split_listing(asm(0, "12ab", True)), B.split_listing(asm(7, "34cd", False))
    assert a == b and set(a) == {"_module", "kern", "other"}
    assert a["kern"] == ["\t.protected\tkern", "kern:", "\ts_cbranch_scc1 .LBB_2", ".LBB_2:", "\ts_endpgm", "\t.amdhsa_kernel kern", "\t\t.amdhsa_next_free_vgpr 8",
                         "\t.end_amdhsa_kernel", ".Lfunc_end:", "\t.size\tkern, .Lfunc_end-kern"]
    assert B.split_listing(asm(0, "12ab", True).replace("next_free_vgpr 8", "next_free_vgpr 9"))["kern"] != a["kern"]
