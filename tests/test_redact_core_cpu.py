"""The redaction rules (simple_pose_amd/csrc/sp_redact.h) under AddressSanitizer + UBSan, on the CPU: tests/redact_core_main.cpp is a
stand-alone program, statically linked against the sanitizer runtimes (nothing has to be preloaded for them) and run as a subprocess in the
test's own environment.  It redacts the scenes of tests/redact_scenes.py - the ones the GPU tests use - and every image is compared bit
for bit with tests/redact_ref.py.  This checks the header the kernels share, bounds and bits; it never runs on a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import redact_ref, redact_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
         "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simple_pose_amd", "csrc")]


def _compile(tmp):
    """-> path of the sanitized program, or None when no compiler here links a static ASan runtime."""
    src, exe = os.path.join(ROOT, "tests", "redact_core_main.cpp"), os.path.join(tmp, "redact_core_main")
    candidates = [(os.environ.get("CXX") or "g++", ["-static-libasan", "-static-libubsan"]), ("clang++", []), ("/opt/rocm/lib/llvm/bin/clang++", [])]
    for cxx, extra in candidates:
        if shutil.which(cxx) is None:
            continue
        r = subprocess.run([cxx] + FLAGS + extra + [src, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        if "asan" not in (r.stderr or "").lower() and "sanitize" not in (r.stderr or "").lower():
            raise AssertionError(f"{cxx} failed to compile tests/redact_core_main.cpp:\n{r.stderr}")
    return None


def _write(path, scene, style, image):
    rows, J = scene["kps"].shape[:2]
    h, w = scene["img"].shape[:2]
    with open(path, "wb") as f:
        f.write(np.array([h, w, rows, J, scene["keep_count"].size, image], np.int32).tobytes())
        f.write(bytes(redact_scenes.style_struct(style)))
        for k, dt in (("kps", np.float64), ("box", np.float32), ("keep", np.int32), ("keep_count", np.int32), ("seg", np.int32), ("img", np.uint8)):
            f.write(np.ascontiguousarray(scene[k], dt).tobytes())


def test_header_redacts_the_scenes_bitwise_as_the_reference_under_asan_ubsan(tmp_path):
    exe = _compile(str(tmp_path))
    if exe is None:
        pytest.skip("no compiler with a static AddressSanitizer runtime")
    st = redact_scenes.styles()
    S = redact_ref.Style
    cases = [(f"street_{k}", redact_scenes.street(), v, 0) for k, v in st.items()]
    cases += [(f"street_cell{c}", redact_scenes.street(), S(cell=c), 0) for c in redact_ref.CELLS]
    cases += [(f"street_{fb}", redact_scenes.street(), S(cell=4, fallback=fb), 0) for fb in ("box", "none")]
    cases += [("street_wide", redact_scenes.street(96, 128), S(cell=16, expand=64, head_min=256, top_frac=256), 0),
              ("tiny", redact_scenes.street(3, 5), S(cell=4, region="person"), 0), ("crowd", redact_scenes.crowd(), S(cell=4), 0),
              ("two_images_0", redact_scenes.two_images(), st["head_mosaic"], 0), ("two_images_1", redact_scenes.two_images(), st["person_fill"], 1)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")      # the environment as it is, plus the sanitizer's options
    for name, scene, style, image in cases:
        src, out = str(tmp_path / f"{name}.bin"), str(tmp_path / f"{name}.bgr")
        _write(src, scene, style, image)
        r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
        assert r.stdout.startswith("OK "), r.stdout
        got = np.fromfile(out, np.uint8).reshape(scene["img"].shape)
        want = redact_scenes.reference(scene, style, image)
        assert (want != scene["img"]).any(), name                                # the scene redacts something
        np.testing.assert_array_equal(got, want, err_msg=name)
