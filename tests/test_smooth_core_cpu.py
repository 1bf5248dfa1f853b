"""The smoother's per-joint rules (simple_pose_amd/csrc/sp_smooth.h) under AddressSanitizer + UBSan, on the CPU: tests/smooth_core_main.cpp
is a stand-alone program, statically linked against the sanitizer runtimes (nothing has to be preloaded for them), compiled with
contraction off and run as a subprocess in the test's own environment.  It filters the sequences of tests/smooth_scenes.py - the ones the
GPU test sends through the kernel - and every frame's output and state are compared bit for bit with tests/smooth_ref.py.  This checks the
header the kernel shares, bounds and bits; it never runs on a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import smooth_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
         "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simple_pose_amd", "csrc")]


def _compile(tmp):
    """-> path of the sanitized program, or None when no compiler here links a static ASan runtime."""
    src, exe = os.path.join(ROOT, "tests", "smooth_core_main.cpp"), os.path.join(tmp, "smooth_core_main")
    candidates = [(os.environ.get("CXX") or "g++", ["-static-libasan", "-static-libubsan"]), ("clang++", []), ("/opt/rocm/lib/llvm/bin/clang++", [])]
    for cxx, extra in candidates:
        if shutil.which(cxx) is None:
            continue
        r = subprocess.run([cxx] + FLAGS + extra + [src, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        if "asan" not in (r.stderr or "").lower() and "sanitize" not in (r.stderr or "").lower():
            raise AssertionError(f"{cxx} failed to compile tests/smooth_core_main.cpp:\n{r.stderr}")
    return None


def _write(path, case, frames):
    slots, J = smooth_scenes.CASES[case]
    p = smooth_scenes.PARAMS
    with open(path, "wb") as f:
        f.write(np.array([slots, J, frames[0]["kps"].shape[0], len(frames)], np.int32).tobytes())
        f.write(np.array([p["min_cutoff"], p["beta"], p["d_cutoff"], p["max_gap"], p["in_vis_thre"]], np.float64).tobytes())
        for fr in frames:
            f.write(np.array([fr["now"]], np.float64).tobytes())
            for k, dt in (("kps", np.float64), ("box", np.float32), ("track_id", np.int32), ("keep", np.int32), ("keep_count", np.int32),
                          ("seg", np.int32), ("t_id", np.int32)):
                f.write(np.ascontiguousarray(fr[k], dt).tobytes())


def test_header_filters_the_sequences_bitwise_as_the_reference_under_asan_ubsan(tmp_path):
    exe = _compile(str(tmp_path))
    if exe is None:
        pytest.skip("no compiler with a static AddressSanitizer runtime")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")      # the environment as it is, plus the sanitizer's options
    for case, (slots, J) in smooth_scenes.CASES.items():
        frames, want = smooth_scenes.sequence(case), smooth_scenes.reference(case)
        rows = frames[0]["kps"].shape[0]
        src, out = str(tmp_path / f"{case}.bin"), str(tmp_path / f"{case}.out")
        _write(src, case, frames)
        r = subprocess.run([exe, src, out], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, f"{case}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
        assert r.stdout.startswith("OK "), r.stdout
        raw, off = open(out, "rb").read(), 0
        for f, (want_kps, st) in enumerate(want):
            for name, ref, dt, shape in (("kps_smooth", want_kps, np.float64, (rows, J, 3)), ("s_id", st.id, np.int32, (slots,)),
                                         ("s_x", st.x, np.float64, (slots, J, 2)), ("s_dx", st.dx, np.float64, (slots, J, 2)),
                                         ("s_t", st.t, np.float64, (slots, J)), ("s_n", st.n, np.int32, (slots, J))):
                nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
                got = np.frombuffer(raw[off:off + nbytes], dt).reshape(shape)
                off += nbytes
                smooth_scenes.bits_equal(got, ref, f"{case} frame {f} {name}")
        assert off == len(raw), case
        ev = want[-1][1].events
        assert all(ev.values()), (case, ev)                                      # the sequence went through every branch of the rules
