"""The case tables and references of tests/test_gpu_tower.py (tests/devref.py), proven without a GPU: the element functions of
gsc_debug_tower_ops (csrc/debug_tower_ops.hpp) are built for the host (tests/native/tower_check.cpp; HostGroup stands for the 8-lane
groups of path 1) and must satisfy every table: values against the big-integer references, and the bounds verify_dev.hpp documents on
the raw limbs that come back.  The generic pairing reference is compared with verify_dev.hpp's and verify_few_dev.hpp's whole pairing
built for the host.  What the GPU tests then find can only lie in the device build."""
import os
import subprocess
import sys

import pytest

import devref as D


@pytest.fixture(scope="module")
def tower_exe():
    return D.native_exe("tower_check")


_PARAMS = [(0, op) for op in range(len(D.TOWER_NAMES))] + [(1, op) for op in D.TOWER_PATH1_OPS]


@pytest.mark.parametrize("path,op", _PARAMS, ids=["%s-path%d" % (D.TOWER_NAMES[op], path) for path, op in _PARAMS])
def test_host_tower_op_matches_the_reference(tower_exe, path, op):
    case = D.tower_case(op)
    n = len(case.rows) if path == 0 else min(len(case.rows), max(D.GROUP_COUNTS))
    assert n % 64 and (op not in D.TOWER_HEAVY or n <= 16)
    outs, flags = D.native_tower_ops(tower_exe, path, op, case.rows[:n])
    assert not case.mismatches(path, outs, flags, n)


def test_word_counts_agree_with_the_wrapper():
    import gsc_loader
    g = gsc_loader.load()
    for path in (0, 1):
        for op in range(len(D.TOWER_NAMES)):
            if path == 0 or op in D.TOWER_PATH1_OPS:
                assert g.tower_words(path, op) == D.tower_words(path, op)
            else:
                with pytest.raises(RuntimeError):
                    g.tower_words(path, op)


@pytest.mark.parametrize("path", [2, 3], ids=["per-thread", "lane-sliced"])
def test_host_pairing_equals_the_generic_reference(tower_exe, path):
    cases = D.pairing_cases()
    assert 8 <= len(cases) <= 10
    rows = [D._w1(D.to_mont(p[0][0])) + D._w1(D.to_mont(p[1][0])) + D._w2((D.to_mont(q[0][0]), D.to_mont(q[0][1]))) + D._w2((D.to_mont(q[1][0]), D.to_mont(q[1][1])))
            for p, q, _ in cases]
    outs, _ = D.native_tower_ops(tower_exe, path, 0, rows, wout=108)
    for (p, q, want), o in zip(cases, outs):
        assert tuple(v for c in D._v12(o) for v in c) == want


def test_hook_declared_exported_and_wrapped(gsc):
    sym = "gsc_debug_tower_ops"
    header = open(os.path.join(D.ROOT, "include", "libprove.h")).read()
    assert ("extern int " + sym + "(int path, int op, const int32_t *in, size_t n, int32_t *out, uint8_t *flags);") in header
    assert sym in gsc.EXPORTS and callable(gsc.debug_tower_ops)
    assert "gsc_*" in open(os.path.join(D.CSRC, "exports.map")).read()
    if not os.path.exists(gsc.LIB_PATH):
        gsc.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", gsc.LIB_PATH]).decode()
    assert sym in {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_no_production_unit_includes_the_hook_header():
    users = [f for f in sorted(os.listdir(D.CSRC)) if f.endswith((".hip", ".cpp", ".hpp")) and '#include "debug_tower_ops.hpp"' in open(os.path.join(D.CSRC, f)).read()]
    assert users == ["k_debug_tower.hip"]


def test_hook_refuses_unknown_selectors_and_a_process_without_test_hooks(gsc):
    """both answers come before anything touches a device"""
    for path, op in ((2, 0), (-1, 0), (0, len(D.TOWER_NAMES)), (0, -1), (1, D.T_MUL2), (1, D.T_LINES_OF)):
        assert gsc.lib().gsc_debug_tower_ops(path, op, None, 0, None, None) == -1
    code = ("import sys, ctypes as C; sys.path.insert(0, %r); import gsc_loader; g = gsc_loader.load(); a = (C.c_int32 * 9)(); f = C.create_string_buffer(1); "
            "print('rc=%%d' %% g.lib().gsc_debug_tower_ops(0, 0, a, 1, (C.c_int32 * 9)(), f))" % D.ROOT)
    env = {k: v for k, v in os.environ.items() if k != "GSC_ENABLE_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600, check=True).stdout.decode()
    assert "rc=-1" in out.split() and "refused:" in out.split()      # the library says why on stdout
