"""GPU unit tests of the proof assembly kernels alone, through gsc_debug_assemble (include/libprove.h): k_prep_rs, k_fin_scalarmul,
k_fin_scalarmul_few, k_fin_combine, k_points_to_affine_be and k_challenge_from_point, launched by the hook in the prover's order on sums the test
chose — every point a known multiple of the generator, handed over as an XYZZ image under a scale (1, p - 1, all limbs at their maximum, random),
one pattern per column: scalars at the edges (0, 1, r - 1, bit 253, lambda, 2^128 ...), degenerate operands in each of k_fin_combine's additions,
each input at infinity alone and all at once, flagged columns at every byte position of a flag word between clean ones.

The reference is integer arithmetic on the discrete logarithms (tests/devref.py AssembleCase), compared byte for byte on EVERY column: out (a
flagged part keeps the fill byte), flags, tmp, cpts, commit, the rows of W, the mask, the halves the kernel got.  The latency kernel is also held
against the batch kernel's bytes, and, through glv_in, run on halves glv_split never returns (a negative k1, chunks of 31 in every position, the
fifth word).  tests/test_assemble_model_host.py proves the reference and the table on a CPU first; a failure here lies in the device code."""
import ctypes

import pytest

import devref as D

pytestmark = pytest.mark.gpu
KEYS = ("out", "flags", "tmp", "tmp_inf", "W", "mask_out", "cpts", "commit", "glv")
WIDTH = {"out": 256, "flags": 1, "W": 32, "mask_out": 32, "commit": 32}


def _run(gsc, case, nproofs=0, has_c=True, has_commit=True, fill=0xA5, unit_scales=False, halves=None, n_wires=3):
    glv_in = None if halves is None else b"".join(D.glv_record(0, rec) for col in halves for rec in col)
    res = gsc.debug_assemble(case.batch, case.sets(has_c, has_commit, unit_scales), case.rs(), nproofs=nproofs, mask=case.mask(), n_wires=n_wires, fill=fill, glv_in=glv_in)
    assert res["rc"] == 0
    return res


def _mismatches(case, res, want):
    """(output, column) of every difference"""
    B, bad = case.batch, []
    for key in KEYS:
        if want.get(key) is None:
            assert res[key] is None, key
            continue
        assert len(res[key]) == len(want[key]), key
        if res[key] == want[key]:
            continue
        if key in WIDTH:
            w = WIDTH[key]
            bad += [(key, p % B if key == "W" else p) for p in range(len(want[key]) // w) if res[key][w * p:w * p + w] != want[key][w * p:w * p + w]]
        else:
            w = {"tmp": 64, "tmp_inf": 1, "cpts": 64, "glv": 88}[key]
            bad += [(key, p if key == "glv" else p % B) for p in range(len(want[key]) // w) if res[key][w * p:w * p + w] != want[key][w * p:w * p + w]]
    return [(key, p, case.cols[p]["name"]) for key, p in bad]


@pytest.fixture(scope="module")
def table():
    return D.assemble_table()


@pytest.fixture(scope="module")
def batch_run(gsc, table):
    return _run(gsc, table)


def test_batch_kernel_on_the_table(table, batch_run):
    assert not _mismatches(table, batch_run, table.expected())[:6]
    want = table.expected()
    assert want["cpts"][64 * 16:64 * 17] == bytes(64) == batch_run["cpts"][64 * 16:64 * 17] and want["flags"][16] == 8       # a commitment at infinity
    assert batch_run["cpts"][64 * (64 + 21):64 * (65 + 21)] == bytes(64) and batch_run["flags"][21] == 16


def test_batch_kernel_another_fill_unit_scales_other_rows(gsc, table):
    """a flagged part leaves its bytes alone whatever they were; every sum once with ZZ = ZZZ = 1; k_prep_rs's rows behind another number of wires"""
    res = _run(gsc, table, fill=0x00, unit_scales=True, n_wires=0)
    assert not _mismatches(table, res, table.expected(fill=0x00))[:6]


@pytest.mark.parametrize("has_c,has_commit", [(False, True), (True, False), (False, False)], ids=["no_c", "no_commitment", "neither"])
def test_batch_kernel_without_c_without_the_commitment(gsc, table, has_c, has_commit):
    res = _run(gsc, table, has_c=has_c, has_commit=has_commit)
    assert not _mismatches(table, res, table.expected(has_c=has_c, has_commit=has_commit))[:6]


@pytest.mark.parametrize("nproofs,rot", [(1, 0), (1, 1), (3, 0), (32, 0), (32, 32)])
def test_latency_kernel_on_the_table(gsc, table, batch_run, nproofs, rot):
    """the first nproofs columns through k_fin_scalarmul_few on glv_split's halves; the table's second half comes first with rot = 32"""
    case = table.rotated(rot)
    res = _run(gsc, case, nproofs=nproofs)
    want = case.expected(nproofs=nproofs)
    assert want["glv"] == b"".join(D.glv_record(c[key]) for c in case.cols[:nproofs] for key in ("s", "r"))
    assert not _mismatches(case, res, want)[:6]
    for p in range(nproofs):      # ... and the batch kernel's bytes for the same columns
        q = (p + rot) % 64
        assert res["out"][256 * p:256 * p + 256] == batch_run["out"][256 * q:256 * q + 256] and res["flags"][p] == batch_run["flags"][q], (p, case.cols[p]["name"])
        for role in (0, 1):
            assert res["tmp"][64 * (64 * role + p):64 * (64 * role + p + 1)] == batch_run["tmp"][64 * (64 * role + q):64 * (64 * role + q + 1)], (p, role)
    for p in range(nproofs, 64):      # the columns the latency kernel does not own: Ar's bytes and flag untouched, tmp at infinity
        assert res["out"][256 * p:256 * p + 64] == bytes([0xA5]) * 64 and not res["flags"][p] & 1 and res["tmp_inf"][p] == 1 == res["tmp_inf"][64 + p]


@pytest.mark.parametrize("rot,has_c", [(0, True), (32, False)])
def test_latency_kernel_on_chosen_halves(gsc, table, rot, has_c):
    """glv_in: all four sign pairs, every chunk 31, one chunk alone at each position of each half, the fifth word — on every pattern of the table"""
    case, halves = table.rotated(rot), D.assemble_halves()
    res = _run(gsc, case, nproofs=32, has_c=has_c, halves=halves)
    assert not _mismatches(case, res, case.expected(nproofs=32, has_c=has_c, halves=halves))[:6]


def test_ragged_batch_of_67(gsc):
    """a second workgroup of three columns, the p >= batch guards, a flag word used in part"""
    case = D.assemble_table(67)
    want = case.expected()
    assert len(set(want["flags"][64:])) == 3 and all(want["flags"][64:])
    assert not _mismatches(case, _run(gsc, case), want)[:6]
    res = _run(gsc, case, nproofs=3)
    assert not _mismatches(case, res, case.expected(nproofs=3))[:6]


def test_refusals(gsc, table, capfd):
    """each returns -1 with its reason on stdout; the device's own refusal: a point that is not on the curve"""
    case = D.AssembleCase(table.cols[32:36])
    sets, rs = case.sets(), case.rs()
    ok = lambda **kw: gsc.debug_assemble(kw.pop("batch", 4), kw.pop("sets", sets), kw.pop("rs", rs), **kw)["rc"]
    def printed():
        ctypes.CDLL(None).fflush(None)      # the library's stdio buffer
        return capfd.readouterr().out
    printed()
    assert ok() == 0 and "gsc_debug_assemble" not in printed()
    be = lambda v: int(v).to_bytes(32, "big")
    edit = lambda name, part, at, data: dict(sets, **{name: tuple(x[:at] + data + x[at + len(data):] if i == part else x for i, x in enumerate(sets[name]))})
    for kw, why in (({"batch": 0}, "batch is 1 .. 256"), ({"batch": 257}, "batch is 1 .. 256"), ({"nproofs": 33}, "nproofs beyond"), ({"nproofs": 5}, "nproofs beyond"),
                    ({"rs": D.R.to_bytes(32, "little") + rs[32:]}, "not below r"), ({"mask": b"\xff" * 128}, "mask that is not below r"),
                    ({"sets": edit("k", 2, 0, bytes(32))}, "scale that is zero: K"), ({"sets": edit("b2", 2, 0, be(D.P) + be(1))}, "not below p: B2"),
                    ({"sets": {k: v for k, v in sets.items() if k != "z"}}, "missing: Z"), ({"sets": {k: v for k, v in sets.items() if k != "d"}}, "D and Pok"),
                    ({"glv_in": bytes(88 * 4)}, "glv_in without nproofs"),
                    ({"sets": edit("a", 0, 63, bytes([sets["a"][0][63] ^ 1]))}, "not on the curve / in the group: A"),
                    ({"sets": edit("b2", 0, 128 + 127, bytes([sets["b2"][0][255] ^ 1]))}, "not on the curve / in the group: B2")):
        assert ok(**kw) == -1, why
        assert why in printed(), why
    assert ok() == 0
