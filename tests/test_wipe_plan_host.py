"""What a call clears from device memory, and when (csrc/wipe_plan.hpp) — on CPU: the plan is a pure function of the chunk's route, a few sizes and
the lane's region table, compiled with g++ alone into tests/native/wipe_plan_check.cpp.  For every route chunk_route can return (small / generic /
resident witness, latency / batch, evaluation / coefficient form, fused / recoded digits, the quotient beside the wire sets or not, with and
without a commitment) and B in {64, 128, 256}, n in {1, 5, 64, B - 3}: the two phases together cover what the stages write, phase A holds nothing
a later stage touches, the marked plane rows are never zeroed, no public region appears.  The GPU legs (tests/test_gpu_secrets_full.py) show
that the engine's buffers really are clean afterwards."""
import os
import subprocess

from conftest import ROOT


def test_every_route_is_covered_and_no_phase_runs_before_a_regions_last_reader():
    exe = os.path.join(ROOT, "build", "wipe_plan_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "wipe_plan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "WIPE-PLAN-OK" in out.stdout, out.stdout[-4000:] + out.stderr[-2000:]
