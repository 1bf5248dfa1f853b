"""The overlay text's rules (simple_pose_amd/csrc/sp_label.h, sp_font.h) under AddressSanitizer + UBSan, on the CPU:
tests/label_core_main.cpp is a stand-alone program, statically linked against the sanitizer runtimes (nothing has to be preloaded for them)
and run as a subprocess in the test's own environment.  It draws the cases of tests/label_scenes.py - the ones the GPU tests draw - and
every image is compared bit for bit with tests/label_ref.py.  This checks the header the kernels share, bounds and bits; it never runs on a
GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import label_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
         "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simple_pose_amd", "csrc")]


def _compile(tmp):
    """-> path of the sanitized program, or None when no compiler here links a static ASan runtime."""
    src, exe = os.path.join(ROOT, "tests", "label_core_main.cpp"), os.path.join(tmp, "label_core_main")
    candidates = [(os.environ.get("CXX") or "g++", ["-static-libasan", "-static-libubsan"]), ("clang++", []), ("/opt/rocm/lib/llvm/bin/clang++", [])]
    for cxx, extra in candidates:
        if shutil.which(cxx) is None:
            continue
        r = subprocess.run([cxx] + FLAGS + extra + [src, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        if "asan" not in (r.stderr or "").lower() and "sanitize" not in (r.stderr or "").lower():
            raise AssertionError(f"{cxx} failed to compile tests/label_core_main.cpp:\n{r.stderr}")
    return None


def _write(path, case):
    sc = case["scene"]
    h, w = sc["img"].shape[:2]
    alloc = sc["box"].shape[0]
    rows = alloc if case["rows"] is None else case["rows"]
    images = sc["keep_count"].size
    cap = case["caption"] if case["caption"] is not None else np.zeros((images, 64), np.uint8)
    with open(path, "wb") as f:
        f.write(np.array([h, w, rows, images, case["image"], int(case["with_ids"]), int(case["caption"] is not None), alloc], np.int32).tobytes())
        f.write(bytes(label_scenes.style_struct(case["style"])))
        kc = sc["keep_count"] if case["keep_count"] is None else case["keep_count"]
        for a, dt in ((sc["box"], np.float32), (sc["score"], np.float64), (sc["track_id"], np.int32), (sc["keep"], np.int32), (kc, np.int32),
                      (sc["seg"], np.int32), (cap, np.uint8), (sc["img"], np.uint8)):
            f.write(np.ascontiguousarray(a, dt).tobytes())


def test_header_draws_the_cases_bitwise_as_the_reference_under_asan_ubsan(tmp_path):
    exe = _compile(str(tmp_path))
    if exe is None:
        pytest.skip("no compiler with a static AddressSanitizer runtime")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")      # the environment as it is, plus the sanitizer's options
    drawn = 0
    for case in label_scenes.cases():
        name = case["name"]
        src, out = str(tmp_path / f"{name}.bin"), str(tmp_path / f"{name}.bgr")
        _write(src, case)
        r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
        assert r.stdout.startswith("OK "), r.stdout
        img = case["scene"]["img"]
        got = np.fromfile(out, np.uint8).reshape(img.shape)
        want = label_scenes.reference(case)
        assert bool((want != img).any()) == case["draws"], name                  # the case draws something, or is one of the no-ops
        np.testing.assert_array_equal(got, want, err_msg=name)
        drawn += int(case["draws"])
    assert drawn >= 20
