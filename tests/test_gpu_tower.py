"""GPU unit tests of the verifier's arithmetic, one operation at a time (gsc_debug_tower_ops): the Fp / Fp2 helpers, the Fp12 tower, the
Miller steps and the final exponentiation of csrc/verify_dev.hpp (path 0, one element per thread) and the lane-sliced Fp12 operations
of csrc/verify_few_dev.hpp (path 1, one element per 8-lane group).  Operands are raw limbs of every class verify_dev.hpp admits —
canonical values, values just inside +-5p, lazy sums of two reduced values, negative top limbs — and every result is compared, by exact
integer equality, with a big-integer reference that knows nothing of the device's formulas (tests/devref.py); the raw limbs that come
back must also keep the bounds the header documents.  The whole reduced pairing of both gsc_debug_pairing paths must equal a generic
chord-and-tangent computation on E(Fp12) coefficient for coefficient.  tests/test_debug_tower_host.py proves the same tables and
references on a host build first."""
import os
import subprocess
import sys

import pytest

import devref as D

pytestmark = pytest.mark.gpu
ROOT = D.ROOT
_ids = lambda op: D.TOWER_NAMES[op]


@pytest.mark.parametrize("op", range(len(D.TOWER_NAMES)), ids=_ids)
def test_per_thread_op_matches_the_reference(gsc, op):
    case = D.tower_case(op)
    assert len(case.rows) % 64 and (op not in D.TOWER_HEAVY or len(case.rows) <= 16)
    outs, flags = gsc.debug_tower_ops(0, op, case.rows)
    assert not case.mismatches(0, outs, flags)


@pytest.mark.parametrize("op", D.TOWER_PATH1_OPS, ids=_ids)
def test_group_op_matches_the_reference(gsc, op):
    """1, 7, 8, 9 and 65 groups: the groups of a wave that hold no element run on the identity beside the others, whose results must not
    change; the slices of the two pad lanes come back zero (TowerCase.mismatches)"""
    case = D.tower_case(op)
    for n in D.GROUP_COUNTS:
        if n <= (16 if op in D.TOWER_HEAVY else len(case.rows)):
            outs, flags = gsc.debug_tower_ops(1, op, case.rows[:n])
            assert not case.mismatches(1, outs, flags, n), n


def test_is_one12_sees_every_group_position_of_a_wave(gsc):
    """wave j of the table holds seven ones and, at group position j, an element that is not one"""
    case = D.tower_case(D.T_IS_ONE12)
    _, flags = gsc.debug_tower_ops(1, D.T_IS_ONE12, case.rows)
    assert not case.mismatches(1, [()] * len(flags), flags)
    assert [i for i in range(64) if not flags[i]] == [9 * j for j in range(8)]


@pytest.mark.parametrize("few", [False, True], ids=["per-thread", "few"])
def test_pairing_equals_the_generic_reference(gsc, few):
    cases = D.pairing_cases()
    got = gsc.debug_pairing([(p[0][0], p[1][0]) for p, _, _ in cases], [q for _, q, _ in cases], few=few)
    assert got == [want for _, _, want in cases]


def test_unknown_selectors_are_refused(gsc):
    row = [(0,) * 108]
    for path, op in ((2, 0), (-1, 0), (0, len(D.TOWER_NAMES)), (0, -1), (1, D.T_MUL2), (1, D.T_DBL_STEP), (1, D.T_LINES_OF)):
        with pytest.raises(RuntimeError):
            gsc.debug_tower_ops(path, op, row)
        assert gsc.lib().gsc_debug_tower_ops(path, op, None, 0, None, None) == -1


def test_tower_hook_refused_without_test_hooks():
    code = ("import sys, ctypes as C; sys.path.insert(0, %r); import gsc_loader; g = gsc_loader.load(); a = (C.c_int32 * 9)(); f = C.create_string_buffer(1); "
            "print('rc=%%d' %% g.lib().gsc_debug_tower_ops(0, 0, a, 1, (C.c_int32 * 9)(), f))" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "GSC_ENABLE_TEST_HOOKS"}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600, check=True).stdout.decode()
    assert "rc=-1" in out.split() and "refused:" in out.split()      # the library says why on stdout
