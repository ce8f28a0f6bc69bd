"""CPU tests of the few-proof verifier path (no GPU needed):
- csrc/verify_few_dev.hpp (the lane-sliced device code of k_verify_few.hip) compiled for the host, the lanes of a group walked in a
  loop, gives the serial results of csrc/verify_dev.hpp operation for operation (tests/native/verify_few_check.cpp);
- the new symbols are declared in include/libprove.h, exported by libprove.so and wrapped in Python;
- GSC_VERIFY_FEW_MAX is documented where the other GSC_* variables are."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "csrc")
NEW = ["gsc_verify_json", "gsc_verify_last_path", "gsc_debug_verify_path", "gsc_debug_pairing_few"]


@pytest.fixture(scope="module")
def few_check():
    exe = os.path.join(ROOT, "build", "verify_few_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "native", "verify_few_check.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_lane_sliced_code_on_the_host_agrees_with_the_serial_code(few_check, seed):
    p = subprocess.run([few_check, str(seed)], capture_output=True, timeout=600)
    out = p.stdout.decode()
    assert p.returncode == 0 and "FAIL" not in out, out
    assert out.split()[0] == "ok" and int(out.split()[1]) > 100


def test_new_symbols_declared_exported_and_wrapped(gsc):
    header = open(os.path.join(ROOT, "include", "libprove.h")).read()
    for sym in NEW:
        assert (" " + sym + "(") in header, sym
        assert sym in gsc.EXPORTS, sym
    if not os.path.exists(gsc.LIB_PATH):
        gsc.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", gsc.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(NEW) <= exported
    for fn in ("verify_json", "verify_last_path", "debug_verify_path"):
        assert callable(getattr(gsc, fn))


def test_few_max_is_documented():
    assert "GSC_VERIFY_FEW_MAX" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "GSC_VERIFY_FEW_MAX" in open(os.path.join(ROOT, "include", "libprove.h")).read()
