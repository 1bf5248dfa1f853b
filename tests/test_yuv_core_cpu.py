"""The patch functions of simple_pose_amd/csrc/sp_yuv.h - the code a thread of the YUV <-> BGR kernels runs - under AddressSanitizer + UBSan
on the CPU: tests/yuv_core_main.cpp is a stand-alone program, statically linked against the sanitizer runtimes (nothing has to be preloaded
for them) and run as a subprocess in the test's own environment.  It converts frames of the edge shapes in exactly-sized heap buffers
(both formats, both directions, tight and padded pitches, base offsets 0 and 1, and 33x130 in 16-byte pitches for the wide path with a
tail), compares every one with a per-pixel loop over the contract, checks that pitch padding keeps its fill, and compares the BT.601
full-range pixel functions with the JPEG decoder's and encoder's over all 2^24 triples.  It never runs on a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
         "-I" + os.path.join(ROOT, "simple_pose_amd", "csrc")]
SHAPES = 9
CASES = SHAPES * 2 * 2 * 2 * 2 + 2 * 2 * 4 * 2


def _compile(tmp):
    """-> path of the sanitized program, or None when no compiler here links a static ASan runtime."""
    src, exe = os.path.join(ROOT, "tests", "yuv_core_main.cpp"), os.path.join(tmp, "yuv_core_main")
    candidates = [(os.environ.get("CXX") or "g++", ["-static-libasan", "-static-libubsan"]), ("clang++", []), ("/opt/rocm/lib/llvm/bin/clang++", [])]
    for cxx, extra in candidates:
        if shutil.which(cxx) is None:
            continue
        r = subprocess.run([cxx] + FLAGS + extra + [src, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        if "asan" not in (r.stderr or "").lower() and "sanitize" not in (r.stderr or "").lower():
            raise AssertionError(f"{cxx} failed to compile tests/yuv_core_main.cpp:\n{r.stderr}")
    return None


def test_patch_functions_match_the_per_pixel_loop_under_asan_ubsan(tmp_path):
    exe = _compile(str(tmp_path))
    if exe is None:
        pytest.skip("no compiler with a static AddressSanitizer runtime")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")      # the environment as it is, plus the sanitizer's options (bounds, not leaks)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    out = r.stdout.splitlines()
    assert sum(l.startswith("OK ") for l in out) == CASES and out[-1] == "PASSED: 0 failures"
    assert "JPEG decode: 0 of 16777216 triples differ from sp_jpeg_ycc_to_bgr" in out
    assert "JPEG encode: 0 of 50331648 samples differ from sp_jpeg_enc_ycc" in out
    patches = [l for l in out if l.startswith("PATCHES ")][0].split()
    assert int(patches[2]) > 0 and int(patches[4]) > 0          # both the 16-byte and the byte path ran
