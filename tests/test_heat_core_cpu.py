"""The heat overlay's rules (simple_pose_amd/csrc/sp_heat.h) under AddressSanitizer + UBSan, on the CPU: tests/heat_core_main.cpp is a
stand-alone program, statically linked against the sanitizer runtimes (nothing has to be preloaded for them) and run as a subprocess in the
test's own environment.  It draws the scenes of tests/heat_scenes.py - the ones the GPU tests use - and every image is compared bit for
bit with tests/heat_ref.py.  This checks the header the kernels share, bounds and bits; it never runs on a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import heat_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
         "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simple_pose_amd", "csrc")]


def _compile(tmp):
    """-> path of the sanitized program, or None when no compiler here links a static ASan runtime."""
    src, exe = os.path.join(ROOT, "tests", "heat_core_main.cpp"), os.path.join(tmp, "heat_core_main")
    candidates = [(os.environ.get("CXX") or "g++", ["-static-libasan", "-static-libubsan"]), ("clang++", []), ("/opt/rocm/lib/llvm/bin/clang++", [])]
    for cxx, extra in candidates:
        if shutil.which(cxx) is None:
            continue
        r = subprocess.run([cxx] + FLAGS + extra + [src, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        if "asan" not in (r.stderr or "").lower() and "sanitize" not in (r.stderr or "").lower():
            raise AssertionError(f"{cxx} failed to compile tests/heat_core_main.cpp:\n{r.stderr}")
    return None


def _write(path, scene, style, image):
    rows, J, mh, mw = scene["hm"].shape
    h, w = scene["img"].shape[:2]
    with open(path, "wb") as f:
        f.write(np.array([h, w, rows, J, mh, mw, scene["keep_count"].size, image], np.int32).tobytes())
        f.write(bytes(heat_scenes.style_struct(style)))
        for k, dt in (("hm", np.float32), ("trans_inv", np.float32), ("keep", np.int32), ("keep_count", np.int32), ("seg", np.int32),
                      ("lut", np.uint8), ("img", np.uint8)):
            f.write(np.ascontiguousarray(scene[k], dt).tobytes())


def test_header_draws_the_scenes_bitwise_as_the_reference_under_asan_ubsan(tmp_path):
    exe = _compile(str(tmp_path))
    if exe is None:
        pytest.skip("no compiler with a static AddressSanitizer runtime")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")      # the environment as it is, plus the sanitizer's options
    for name, scene, style, image in heat_scenes.cases():
        src, out = str(tmp_path / f"{name}.bin"), str(tmp_path / f"{name}.bgr")
        _write(src, scene, style, image)
        r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
        assert r.stdout.startswith("OK "), r.stdout
        got = np.fromfile(out, np.uint8).reshape(scene["img"].shape)
        want = heat_scenes.reference(scene, style, image)
        assert (want != scene["img"]).any(), name                                # the scene draws something
        bad = np.argwhere((got != want).any(axis=2))
        assert bad.shape[0] == 0, f"{name}: {bad.shape[0]} pixels differ, first at (y, x) = {bad[0].tolist()}"
