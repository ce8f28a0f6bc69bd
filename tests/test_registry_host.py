"""Who owns an algorithm's engine (csrc/registry.hpp) — on CPU, with a stub engine: the registry behind InitAlgorithm, gsc_release_algorithm
and gsc_replace_algorithm and the micro-batcher in front of an engine are compiled with g++ into tests/native/registry_check.cpp, whose stub
engine poisons itself when destroyed and aborts when a call reaches it afterwards.  It checks that a release waits for the calls in flight and
for the callers parked in the micro-batcher, that a call is served whole by the engine it found when it entered, that a refused build changes
nothing, that lifecycle operations on one id serialise, and that the other ids stay reachable while one builds.  The same source runs a second
time under ThreadSanitizer, as the stand-alone program it is.  The GPU leg is tests/test_gpu_lifecycle.py."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "registry_check.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Werror", "-pthread"]


def _build(name, extra):
    exe = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++"] + extra + FLAGS + ["-o", exe, SRC])
    return exe


def test_registry_drains_swaps_and_serialises():
    out = subprocess.run([_build("registry_check", ["-O2"])], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "REGISTRY-OK" in out.stdout, out.stdout + out.stderr


def test_registry_is_clean_under_thread_sanitizer(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=thread", "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0:
        pytest.skip("this g++ has no ThreadSanitizer runtime")
    out = subprocess.run([_build("registry_check_tsan", ["-O1", "-g", "-fsanitize=thread"])], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66"))
    assert out.returncode == 0 and "REGISTRY-OK" in out.stdout and "ThreadSanitizer" not in out.stderr, out.stdout[-2000:] + out.stderr[-6000:]
