"""GPU unit tests of the radix-2^29 products and reductions on RAW limbs (gsc_debug_limb_ops): every operand class bn254_fp29.hpp
admits — tight, signed-tight, loose, limbs at their extremes, negative top limbs — goes to the device code exactly as generated, and the
limbs that come back must equal the big-integer prediction of tests/devref.py one for one.  Field 2 is Fp29f: in device code its
mul / sqr / fmms are the carry-chained multiply-add sequences (namespace madc) under every G1 kernel, which no host build executes;
tests/test_debug_ops_host.py proves the same cases and predictions on a CPU first."""
import pytest

import devref as D

pytestmark = pytest.mark.gpu
_ids = lambda v: D.OP_NAMES.get(v, v) if isinstance(v, int) else v


@pytest.mark.parametrize("op,cls", D.limb_params(), ids=_ids)
@pytest.mark.parametrize("field", [0, 1, 2], ids=["Fp29", "Fr29", "Fp29f"])
def test_device_limbs_match_the_prediction(gsc, field, op, cls):
    operands, want = D.limb_case(field, op, cls)
    got = gsc.debug_limb_ops(field, op, *operands)
    assert len(got) == len(want) and not D.limb_mismatches(got, want)


@pytest.mark.parametrize("op,cls", D.limb_params(), ids=_ids)
def test_chained_products_equal_the_plain_ones_limb_for_limb(gsc, op, cls):
    operands, _ = D.limb_case(2, op, cls)
    assert not D.limb_mismatches(gsc.debug_limb_ops(2, op, *operands), gsc.debug_limb_ops(0, op, *operands))


def test_unknown_selectors_are_refused(gsc):
    one = [(1,) + (0,) * 8]
    for field, op in ((3, 0), (-1, 0), (0, 6), (2, -1)):
        with pytest.raises(RuntimeError):
            gsc.debug_limb_ops(field, op, one, one, one, one)
    with pytest.raises(RuntimeError):      # mul without its second operand
        gsc.debug_limb_ops(2, 0, one)
