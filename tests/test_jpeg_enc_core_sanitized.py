"""The encoder core (simple_pose_amd/csrc/sp_jpeg_enc.h) and the host planner (sp_jpeg_enc_plan.h) under AddressSanitizer + UBSan, on
the CPU: tests/jpeg_enc_core_main.cpp is a stand-alone program, statically linked against the sanitizer runtimes (nothing has to be
preloaded for them) and run as a subprocess in the test's own environment.  It encodes every fixture image serially through the inline
functions the kernels call and compares with the file libjpeg-turbo wrote, then encodes the 17x23 noise image into every capacity from 0
to one byte short of its file, which has to end in the overflow status with nothing written.  It never runs on a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g16_jpeg_enc.npz")
SWEEP = ("noise_17x23", 420, 95, 0)
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
         "-I" + os.path.join(ROOT, "simple_pose_amd", "csrc")]


def _compile(tmp):
    """-> path of the sanitized program, or None when no compiler here links a static ASan runtime."""
    src, exe = os.path.join(ROOT, "tests", "jpeg_enc_core_main.cpp"), os.path.join(tmp, "jpeg_enc_core_main")
    candidates = [(os.environ.get("CXX") or "g++", ["-static-libasan", "-static-libubsan"]), ("clang++", []), ("/opt/rocm/lib/llvm/bin/clang++", [])]
    for cxx, extra in candidates:
        if shutil.which(cxx) is None:
            continue
        r = subprocess.run([cxx] + FLAGS + extra + [src, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        if "asan" not in (r.stderr or "").lower() and "sanitize" not in (r.stderr or "").lower():
            raise AssertionError(f"{cxx} failed to compile tests/jpeg_enc_core_main.cpp:\n{r.stderr}")
    return None


def test_core_encodes_the_fixture_and_refuses_every_short_capacity_under_asan_ubsan(tmp_path):
    exe = _compile(str(tmp_path))
    if exe is None:
        pytest.skip("no compiler with a static AddressSanitizer runtime")
    z = np.load(GOLDEN, allow_pickle=False)
    names = bytes(z["image_names"]).decode().split("\n")
    for i, name in enumerate(names):
        (tmp_path / f"{name}.bgr").write_bytes(bytes(z["images"][z["image_offsets"][i]:z["image_offsets"][i + 1]]))
    lines, swept = [], 0
    for c, (i, sub, q, r) in enumerate(z["cases"].tolist()):
        jpg = tmp_path / f"case{c}.jpg"
        jpg.write_bytes(bytes(z["bytes"][z["offsets"][c]:z["offsets"][c + 1]]))
        h, w = z["image_shapes"][i].tolist()
        sweep = int((names[i], sub, q, r) == SWEEP)
        swept += sweep
        lines.append(f"case{c}_{names[i]}_{sub}_q{q}_r{r} {tmp_path / (names[i] + '.bgr')} {w} {h} {sub} {q} {r} {jpg} {sweep}")
    assert swept == 1
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")      # the environment as it is, plus the sanitizer's options (bounds, not leaks)
    r = subprocess.run([exe, str(manifest)], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    out = r.stdout.splitlines()
    assert sum(l.startswith("OK ") for l in out) == len(lines) and out[-1] == "PASSED: 0 failures"
    assert any(l.startswith("SWEEP ") and l.endswith(": 0 not refused cleanly") for l in out)
