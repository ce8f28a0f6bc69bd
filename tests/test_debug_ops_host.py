"""The case tables and references of the per-operation GPU tests (tests/devref.py), proven without a GPU: the element functions of the
test hooks (csrc/debug_ops.hpp) are built for the host, where every product of bn254_fp29.hpp is plain C, and must reproduce the
predictions limb for limb and point for point.  What tests/test_gpu_limbs.py and tests/test_gpu_curve.py then find can only lie in
the device code."""
import pytest

import devref as D


@pytest.fixture(scope="module")
def limb_exe():
    return D.native_exe("fp29_limb_check")


@pytest.fixture(scope="module")
def curve_exe():
    return D.native_exe("curve9_check")


@pytest.mark.parametrize("op,cls", D.limb_params(), ids=lambda v: D.OP_NAMES.get(v, v) if isinstance(v, int) else v)
@pytest.mark.parametrize("field", [0, 1, 2])
def test_host_limbs_match_the_prediction(limb_exe, field, op, cls):
    operands, want = D.limb_case(field, op, cls)
    assert len(want) == len(operands[0]) and len(want) % 64
    got = D.native_limb_ops(limb_exe, field, op, operands)
    assert not D.limb_mismatches(got, want)


def test_every_op_and_field_sees_4096_elements():
    for op, classes in D.LIMB_CLASSES.items():
        assert sum(len(D.limb_case(0, op, c)[1]) for c in classes) >= 4096, D.OP_NAMES[op]


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
def test_host_group_law_matches_the_affine_reference(curve_exe, group):
    cases = D.curve_cases(group)
    assert {c.k for c in cases} >= {1, 2, 3, 64, 257, 10}
    for c in cases:
        out, flags = D.native_curve_ops(curve_exe, group, c.op, *c.packed())
        assert not c.mismatches(out, flags), c.name
