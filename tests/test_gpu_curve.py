"""GPU unit tests of the XYZZ group law (Curve9 of bn254_fp29.hpp) through gsc_debug_curve_ops, for G1 (over the carry-chained Fp29f
products) and G2 (over Fp2x), against the affine chord-and-tangent reference of tests/devref.py: dbl, madd<true>, madd<false>, add and
to_aff on generic, equal and opposite points, infinity on either side, XYZZ operands under scales lambda != 1 (p - 1 and extreme digits
among them), accumulations of 2, 3, 64 and 257 points with repeats and opposite points part-way — and the contract the MSM hot path
relies on: madd<false> on P = +-Q leaves ZZ = 0 mod p, and ZZ stays 0 under further additions.  tests/test_debug_ops_host.py runs the
same cases through a host build first, so a failure here lies in the device code."""
import pytest

import devref as D

pytestmark = pytest.mark.gpu
_cases = {g: {c.name: c for c in D.curve_cases(g)} for g in (0, 1)}


@pytest.mark.parametrize("name", sorted(_cases[0]))
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
def test_device_group_law_matches_the_affine_reference(gsc, group, name):
    c = _cases[group][name]
    out, flags = gsc.debug_curve_ops(group, c.op, *c.packed())
    assert not c.mismatches(out, flags)


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
def test_fast_madd_on_equal_or_opposite_points_zeroes_zz_for_good(gsc, group):
    c = _cases[group]["madd_fast_zero_sticks"]
    assert c.k == 10      # P, +-P, then 8 more additions
    out, flags = gsc.debug_curve_ops(group, c.op, *c.packed())
    assert set(flags) == {D.FLAG_ZZ0_FIRST | D.FLAG_ZZ0_LAST}
    # ... and the exact form on the very same inputs gives the true sums
    exact = D.CurveCase(group, "exact", D.MADD_EXACT, c.elems)
    assert not exact.mismatches(*gsc.debug_curve_ops(group, D.MADD_EXACT, *exact.packed()))


def test_malformed_calls_are_refused(gsc):
    c = _cases[0]["madd_exact_generic"]
    pts, inf, lam, n, k = c.packed()
    with pytest.raises(RuntimeError):      # no such group
        gsc.debug_curve_ops(2, c.op, bytes(2 * len(pts)), inf, bytes(2 * len(lam)), n, k)
    with pytest.raises(RuntimeError):      # no such op
        gsc.debug_curve_ops(0, 6, pts, inf, lam, n, k)
    with pytest.raises(RuntimeError):      # dbl takes one point
        gsc.debug_curve_ops(0, D.DBL, pts, inf, lam, n, k)
    with pytest.raises(RuntimeError):      # infinity cannot be an affine operand
        gsc.debug_curve_ops(0, c.op, pts, bytes([0, 1]) * n, lam, n, k)
