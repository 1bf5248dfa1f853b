"""The progressive entropy core (simple_pose_amd/csrc/sp_jpeg_prog.h) and the scan parser (sp_jpeg_parse_scans.h) under AddressSanitizer +
UBSan, on the CPU: tests/jpeg_prog_core_main.cpp is a stand-alone program, statically linked against the sanitizer runtimes (nothing has to
be preloaded for them) and run as a subprocess in the test's own environment.  It parses and decodes every fixture file of
g17_jpeg_prog.npz and compares with the expected pixels; then, for three files (the non-interleaved geometry, restart segments, EOB runs
with correction bits), every truncation after the first SOS and 300 seeded single-byte corruptions after SOF, which only have to end in
a parser code or a status.  This is the check that the bounds logic the kernel shares is sound; it never runs on a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g17_jpeg_prog.npz")
FUZZ_CASES = ("p_17x9_420", "p_r2_33x17_420", "p_flat_96x96_444")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
         "-I" + os.path.join(ROOT, "simple_pose_amd", "csrc")]


def _compile(tmp):
    """-> path of the sanitized program, or None when no compiler here links a static ASan runtime."""
    src, exe = os.path.join(ROOT, "tests", "jpeg_prog_core_main.cpp"), os.path.join(tmp, "jpeg_prog_core_main")
    candidates = [(os.environ.get("CXX") or "g++", ["-static-libasan", "-static-libubsan"]), ("clang++", []), ("/opt/rocm/lib/llvm/bin/clang++", [])]
    for cxx, extra in candidates:
        if shutil.which(cxx) is None:
            continue
        r = subprocess.run([cxx] + FLAGS + extra + [src, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        if "asan" not in (r.stderr or "").lower() and "sanitize" not in (r.stderr or "").lower():
            raise AssertionError(f"{cxx} failed to compile tests/jpeg_prog_core_main.cpp:\n{r.stderr}")
    return None


def test_progressive_core_decodes_the_fixture_and_survives_damaged_input_under_asan_ubsan(tmp_path):
    exe = _compile(str(tmp_path))
    if exe is None:
        pytest.skip("no compiler with a static AddressSanitizer runtime")
    z = np.load(GOLDEN, allow_pickle=False)
    names = bytes(z["names"]).decode().split("\n")
    lines = []
    for i, name in enumerate(names):
        jpg = tmp_path / f"{name}.jpg"
        jpg.write_bytes(bytes(z["bytes"][z["offsets"][i]:z["offsets"][i + 1]]))
        exp = "-"
        if z["code"][i] == 0:
            exp = str(tmp_path / f"{name}.bgr")
            with open(exp, "wb") as f:
                f.write(bytes(z["pixels"][z["pixel_offsets"][i]:z["pixel_offsets"][i + 1]]))
        lines.append(f"{name} {jpg} {exp} {int(name in FUZZ_CASES)}")
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")      # the environment as it is, plus the sanitizer's options (bounds, not leaks)
    r = subprocess.run([exe, str(manifest)], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    out = r.stdout.splitlines()
    assert sum(l.startswith("OK ") for l in out) == len(names) and out[-1] == "PASSED: 0 failures"
    for name in FUZZ_CASES:
        assert any(l.startswith(f"FUZZ {name} truncations") for l in out) and any(l.startswith(f"FUZZ {name} corruptions") for l in out)
