"""The overlay's pixel rules (simple_pose_amd/csrc/sp_render.h) under AddressSanitizer + UBSan, on the CPU: tests/render_core_main.cpp is a
stand-alone program, statically linked against the sanitizer runtimes (nothing has to be preloaded for them) and run as a subprocess in the
test's own environment.  It renders the scenes of tests/render_scenes.py - the ones the GPU tests draw - and every image is compared bit
for bit with tests/render_ref.py.  This checks the header the kernels share, bounds and bits; it never runs on a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import render_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
         "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simple_pose_amd", "csrc")]


def _compile(tmp):
    """-> path of the sanitized program, or None when no compiler here links a static ASan runtime."""
    src, exe = os.path.join(ROOT, "tests", "render_core_main.cpp"), os.path.join(tmp, "render_core_main")
    candidates = [(os.environ.get("CXX") or "g++", ["-static-libasan", "-static-libubsan"]), ("clang++", []), ("/opt/rocm/lib/llvm/bin/clang++", [])]
    for cxx, extra in candidates:
        if shutil.which(cxx) is None:
            continue
        r = subprocess.run([cxx] + FLAGS + extra + [src, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        if "asan" not in (r.stderr or "").lower() and "sanitize" not in (r.stderr or "").lower():
            raise AssertionError(f"{cxx} failed to compile tests/render_core_main.cpp:\n{r.stderr}")
    return None


def _write(path, scene, style, image, with_ids):
    rows, J = scene["kps"].shape[:2]
    h, w = scene["img"].shape[:2]
    with open(path, "wb") as f:
        f.write(np.array([h, w, rows, J, scene["keep_count"].size, image, int(with_ids)], np.int32).tobytes())
        f.write(bytes(render_scenes.style_struct(style)))
        for k, dt in (("kps", np.float64), ("box", np.float32), ("track_id", np.int32), ("keep", np.int32), ("keep_count", np.int32),
                      ("seg", np.int32), ("img", np.uint8)):
            f.write(np.ascontiguousarray(scene[k], dt).tobytes())


def test_header_renders_the_scenes_bitwise_as_the_reference_under_asan_ubsan(tmp_path):
    exe = _compile(str(tmp_path))
    if exe is None:
        pytest.skip("no compiler with a static AddressSanitizer runtime")
    st = render_scenes.styles()
    cases = [("ragged_person_ids", render_scenes.ragged(), st["person"], 0, True), ("ragged_person", render_scenes.ragged(), st["person"], 0, False),
             ("ragged_part_ids", render_scenes.ragged(), st["part"], 0, True), ("ragged_part", render_scenes.ragged(), st["part"], 0, False),
             ("crowd14", render_scenes.crowd(14), st["person"], 0, True), ("crowd24", render_scenes.crowd(24), st["part"], 0, True),
             ("two_images_1", render_scenes.two_images(), st["person"], 1, True), ("two_images_0", render_scenes.two_images(), st["part"], 0, False)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")      # the environment as it is, plus the sanitizer's options
    for name, scene, style, image, with_ids in cases:
        src, out = str(tmp_path / f"{name}.bin"), str(tmp_path / f"{name}.bgr")
        _write(src, scene, style, image, with_ids)
        r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
        assert r.stdout.startswith("OK "), r.stdout
        got = np.fromfile(out, np.uint8).reshape(scene["img"].shape)
        want = render_scenes.reference(scene, style, image, with_ids)
        assert (want != scene["img"]).any(), name                                # the scene draws something
        np.testing.assert_array_equal(got, want, err_msg=name)
