"""stage_images_jitter_u8 of convnet_amd/csrc/input_staging.hip executed FUNCTIONALLY on the CPU through the C ABI — the real kernel
source compiled as host C++ against tests/emu/hip/hip_runtime.h (tests/emu/stage_jitter_emu_main.cc) — on the scenes of
tests/jitter_scene.py, whose expectation is the host definition (convnet_amd/image_iterators.py): exact to the bit.  Both arms, all four
(norm, jitter) builds, 5 and 130 cases, a patch wider than the tile, a rotated window that leaves the resized crop; then tables of
random numbers, which may give any pixels but must return 0; then the error codes.  No GPU; not a product path."""
import numpy as np

import emu_build
import jitter_scene as js


def _write(path, name, index, rotated, normalize, jitter, seed):
    s = js.scene(name)
    (H, W), (ph, pw) = s["image"], s["patch"]
    if not jitter:
        ph, pw = H, W
    wo, ho, flip = s["wo"][:len(index)], s["ho"][:len(index)], s["flip"][:len(index)]
    want = js.expect(name, s["crops"][index], normalize, jitter, wo, ho, flip)
    if not jitter:
        want = want.reshape(3, H, W, len(index))
    head = np.array([s["data"].size, len(s["table"]), len(s["taps"]), len(index), rotated, normalize, jitter, W, H, pw, ph, seed], np.int64)
    with open(path, "wb") as f:
        for a in (head, s["data"], s["table"], s["taps"], s["cases"][index], s["mean"], s["std"], wo, ho, flip, want):
            f.write(np.ascontiguousarray(a).tobytes())
    return path


def test_the_jitter_kernel_runs_correctly_in_emulation(tmp_path):
    exe = emu_build.build(tmp_path, ["input_staging.hip"], "stage_jitter_emu_main.cc", "the kernels use clang's vector extensions",
                          extras={"input_staging.hip": ["-include", emu_build.os.path.join(emu_build.EMU, "input_staging_emu_prelude.h")]})
    small, plain = js.scene("small"), js.unrotated_cases("small")
    assert small["border"] > 0 and small["both"] > 0 and js.scene("oblong")["border"] > 0 and plain.size >= 8
    scenes = []
    for build in range(4):
        normalize, jitter = build & 1, build >> 1
        for N in (5, 130):
            scenes.append(_write(str(tmp_path / f"small{build}_{N}.bin"), "small", np.arange(N), 1, normalize, jitter, 10 * build + N))
        scenes.append(_write(str(tmp_path / f"plain{build}.bin"), "small", plain[:70], 0, normalize, jitter, 50 + build))
    scenes.append(_write(str(tmp_path / "wide.bin"), "wide", np.arange(3), 1, 1, 1, 60))
    scenes.append(_write(str(tmp_path / "oblong.bin"), "oblong", np.arange(5), 1, 0, 1, 61))
    lines = emu_build.run(exe, *scenes, timeout=600)
    assert sum(l.startswith("PASS jitter ") for l in lines) == len(scenes) == 14
    assert sum(l == "PASS errors" for l in lines) == 1
