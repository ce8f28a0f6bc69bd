"""GPU unit tests of the MSM kernels alone, through gsc_debug_msm (include/libprove.h): signed recoding at c = 4 .. 17, bit groups with their
per-wave prediction check, short rows with the double-and-add escape, window octets of expanded wide wires, byte-plane scalars, the ZZ = 0
repair after madd<false>, the lanes-are-bases latency kernels, the three reduction kernels, Horner with an addend and the XCD-aware slice
placement — on bases P_k = b_k G whose discrete logarithms the test knows and on adversarial scalars, one pattern per column.

The reference is one scalar multiplication per column, (sum_k s_kp b_k mod r) G in Jacobian integer arithmetic (tests/devref.py), compared byte
for byte with the canonical coordinates and the infinity flag of EVERY column.  The recoded digit words, gok and group_ok are compared with a
Python model of the layouts in csrc/kernels.hpp, and the info block says which slices and reduction kernels ran, so a case cannot pass by
silently taking another path.  tests/test_msm_model_host.py proves the reference, the digit model and the case table on a CPU first, and
tests/test_msm_layout_host.py the host-side geometry; a failure here lies in the device code."""
import pytest

import devref as D

pytestmark = pytest.mark.gpu
R = D.R
_results = {}


def _mismatched_columns(case, res):
    want, winf = case.expected()
    w = 64 if case.group == 0 else 128
    return [(p, res["inf"][p], winf[p]) for p in range(case.ncols) if res["out"][w * p:w * p + w] != want[w * p:w * p + w] or res["inf"][p] != winf[p]]


@pytest.mark.parametrize("name", D.msm_case_names())
@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
def test_msm_kernels_match_one_scalar_multiplication_per_column(gsc, group, name):
    case = D.msm_case_table(group)[name]
    res = _results[group, name] = case.call(gsc)
    info, pl = res["info"], case.plan
    # the route that ran: the layout, the slices, the reduction levels
    assert (info[0], info[1], info[2], info[3]) == (pl.nflat, pl.nbit, pl.nexpanded, len(pl.wide))
    assert info[4] == D.msm_windows(case.c) and info[44] == case.ncols and info[47] == pl.cv
    for k, v in case.expect.items():
        assert info[k] == v, (name, k, info[k], v, info[:48])
    for part, at in ((pl.nflat, 9), (len(pl.wide), 26)):      # every level's groups feed the next; the last one leaves one group
        levels = [(info[at + 1 + 2 * i], info[at + 2 + 2 * i]) for i in range(info[at])]
        assert bool(levels) == bool(part) and (not levels or levels[0][0] == info[5 if at == 9 else 7])
        for (ns, by_proof), nxt in zip(levels, levels[1:] + [(1, 0)]):
            assert nxt[0] == (ns + (31 if by_proof else 63)) // (32 if by_proof else 64)
    # the recoders' output, word for word
    assert res["group_ok"] == case.group_ok()
    flat, gok = case.flat_model()
    assert res["gok"] == gok
    assert res["flat_digits"] == flat
    assert res["win_digits"] == case.win_model()
    # every column's sum
    assert not _mismatched_columns(case, res)[:4]


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
def test_every_route_ran(gsc, group):
    """the info blocks of a few named cases show each route of the kernels at least once per group"""
    run = lambda name: _results.get((group, name)) or D.msm_case_table(group)[name].call(gsc)      # (the calls above, when they ran in this session)
    levels = lambda info, at: [(info[at + 1 + 2 * i], info[at + 2 + 2 * i]) for i in range(info[at])]
    assert levels(run("win_c8_n64_8slices")["info"], 26) == [(8, 0)]                          # butterfly, one level
    assert levels(run("win_c8_n520_butterfly_twice")["info"], 26) == [(65, 0), (2, 0)]         # butterfly, two levels
    assert levels(run("win_c6_n520_by_proof")["info"], 26) == [(65, 1), (3, 0)]                # by proof (groups of 32, 32 and 1 slices), then butterfly
    assert levels(run("flat_narrow_n520_per8")["info"], 9) == [(65, 0), (2, 0)]
    r = run("mixed_horner_addend")
    assert r["info"][43] == 1 and r["info"][0] and r["info"][3]                                # Horner with the flat sum as addend
    r = run("bits_one_wave_not_ternary")
    assert r["gok"] == bytes([1, 1, 1, 0]) and r["group_ok"] == b"\1\1"                        # a gok of 0 beside a gok of 1
    assert run("bits_collision_same_base")["group_ok"] == b"\0\1"                              # a group_ok of 0
    r = run("win_digit_bases_40_walk_19_p0")
    assert r["info"][3] == 19 and r["info"][46] == 5                                           # digits laid out for 40 bases, 19 walked
    assert run("win_c16_n9_mont1")["info"][4] == 16 and run("win_c17_n24_mont0")["info"][4] == 15
    assert len(run("win_c17_n24_mont0")["win_digits"]) == 2 * 16 * 15 * 3 * 128                # two words per (window, octet, column)
    r = run("win_few_c6_n129_p32_per64")
    assert r["info"][44] == 32 and r["info"][7] == 3 and levels(r["info"], 26) == [(3, 0)]     # latency kernels, windowed and flat
    assert run("flat_few_oct65_p32")["info"][5] == 2


def _tiny(group, **kw):
    b = [5, 7, 11]
    a = dict(kind=[D.KIND_WIDE] * 3, rows=[0, 1, 2], scalars=[1] * 192 + [0] * 64, n_rows=4, c=6)
    a.update(kw)
    return D.MsmCase(group, "tiny", b, a.pop("kind"), a.pop("rows"), a.pop("scalars"), a.pop("n_rows"), a.pop("c"), **a)


@pytest.mark.parametrize("group", [0, 1], ids=["G1", "G2"])
def test_a_point_off_the_curve_is_refused(gsc, group):
    """the refusal that needs the device: the bytes are raw and finite, the decode kernel finds them off the curve"""
    case = _tiny(group)
    good = case.points()
    assert not _mismatched_columns(case, case.call(gsc))
    bad = bytearray(good); bad[-1] ^= 1      # y + 1 or y - 1 of the last base
    case.points = lambda: bytes(bad)
    with pytest.raises(RuntimeError):
        case.call(gsc)


def test_a_twist_point_outside_the_subgroup_is_refused(gsc):
    """on the twist y^2 = x^3 + 3 / (9 + u) but not of order r (the cofactor is not 1): the subgroup kernel's answer"""
    x, pt = 1, None
    while pt is None:      # a square root in Fp2 through the norm: p = 3 mod 4
        a0, a1 = D.f_add(D.f_mul(D.f_mul((x, 0), (x, 0)), (x, 0)), D.CURVE_B[1])
        s = pow((a0 * a0 + a1 * a1) % D.P, (D.P + 1) // 4, D.P)
        for half in ((a0 + s) * pow(2, -1, D.P) % D.P, (a0 - s) * pow(2, -1, D.P) % D.P):
            y0 = pow(half, (D.P + 1) // 4, D.P)
            if y0 and y0 * y0 % D.P == half:
                y = (y0, a1 * pow(2 * y0, -1, D.P) % D.P)
                if D.on_curve(1, ((x, 0), y)):
                    pt = ((x, 0), y)
        x += 1
    assert D.ec_mul(R, pt) is not None      # not of order r
    case = _tiny(1)
    case.points = lambda: D.raw_point(1, pt) * 3
    with pytest.raises(RuntimeError):
        case.call(gsc)


def test_malformed_calls_are_refused(gsc):
    with pytest.raises(RuntimeError):
        _tiny(0, c=18).call(gsc)
    with pytest.raises(RuntimeError):
        _tiny(0, batch=64, nproofs=33).call(gsc)
    with pytest.raises(RuntimeError):
        _tiny(0, per_win=12).call(gsc)
    with pytest.raises(RuntimeError):      # canonical scalars with a narrow base
        _tiny(0, kind=[D.KIND_NARROW] * 3, rowlen=[4] * 3, mont=0).call(gsc)
    case = _tiny(0)
    case.scalars[5] = R                     # a scalar that is not below r (to_bytes still fits 32 bytes)
    with pytest.raises(RuntimeError):
        case.call(gsc)
    assert not _mismatched_columns(_tiny(0), _tiny(0).call(gsc))
