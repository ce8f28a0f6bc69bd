"""The carry-folded Montgomery products of bn254_fp29.hpp (the G1 field's mul / sqr / fmms in device code) against Field29's,
through a host build of the same header: the column terms, as the device code groups them, must give identical limbs."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "csrc")


def test_chained_products_match_field29():
    exe = os.path.join(ROOT, "build", "fp29_chain_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "native", "fp29_chain_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    n, bad = map(int, out.stdout.split())
    assert n == 400000 and bad == 0 and out.returncode == 0
