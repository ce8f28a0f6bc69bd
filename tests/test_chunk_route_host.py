"""Which kernels a chunk of statements takes (csrc/chunk_route.hpp) — on CPU: the routing policy of the prover is a pure function of the
call's size, the configuration and a few facts about the engine, compiled with g++ alone into tests/native/chunk_route_check.cpp, whose
table holds the expected value of every route field for the sizes around each threshold, every knob the route reads, both retries and
each name of a dominant kernel.  The GPU legs (tests/test_gpu_parity.py, tests/test_gpu_replicas.py) show that the stages follow it."""
import os
import subprocess

from conftest import ROOT


def test_every_route_field_of_the_table():
    exe = os.path.join(ROOT, "build", "chunk_route_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "chunk_route_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "ROUTE-OK" in out.stdout, out.stdout + out.stderr
