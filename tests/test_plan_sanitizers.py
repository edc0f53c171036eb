"""The host planning code of the C ABI (fiat_amd/csrc/plan.hpp: recurrence programs, C0 transform, cooperative
schedule, fragment packings) compiled with AddressSanitizer + UndefinedBehaviorSanitizer and run on the CPU
(GPU sanitizers are not available on this pool)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plan_code_under_asan_ubsan(tmp_path):
    exe = tmp_path / "plan_sanitize"
    src = os.path.join(ROOT, "tests", "native", "plan_sanitize.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert "programs ok" in run.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_counter_handout_under_asan_ubsan(tmp_path):
    """The hand-out of work counters to launches (fiat_amd/csrc/counter_handout.hpp) against simulated streams: one stream
    with 1 000 launches, two and three interleaved, one stream lagging by 63 / 64 / 65 / 500 pending launches, 70 streams,
    a captured launch replayed against direct ones.  No two launches that the device does not order ever run on one
    counter; the former round-robin rule over 64 counters fails the same checker."""
    exe = tmp_path / "counter_handout"
    src = os.path.join(ROOT, "tests", "native", "counter_handout.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert "hand-out ok" in run.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_device_buffer_under_asan_ubsan(tmp_path):
    """The owner of device memory (fiat_amd/csrc/device_buffer.hpp) on a counting heap that fails its k-th allocation or
    copy: moves free the target's old allocation exactly once, a failed upload leaves the buffer empty and leaks nothing,
    a build-then-commit of five buffers leaves the handle bit for bit as it was under a failure at each of its ten steps,
    and the stream-ordered scratch is released on scope exit."""
    exe = tmp_path / "device_buffer"
    src = os.path.join(ROOT, "tests", "native", "device_buffer.cpp")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", str(exe), src], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers ok" in run.stdout
