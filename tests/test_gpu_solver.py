"""GPU unit tests of the witness solver kernels alone, through gsc_debug_solve (include/libprove.h): k_solver<HAS_DIV, WPB>, k_solver_count,
k_solver_few, k_solver_count_few and the kernels of k_wit_small.hip on small synthetic constraint systems whose column patterns put bits, wide
values, zero divisors and refused lookups into ONE wave — the mixed-lane branches, expression lengths at every boundary of the window, slot and
chunk machinery, divisions by a known factor that is zero, out-of-range hint inputs, and `status` per column, none of which the two ciphers' own
circuits reach.

The reference is tests/solver_model.py: a sequential solver in Python integers (held against the oracle and an independent checker by
tests/test_solver_model_host.py, which also replays the builders' layouts on the host: a failure here lies in the device code).  The comparison is
exact — these are integers: every element of W, A, B, C of every satisfied column is below r and, times 2^-256, equals the reference; the set of
unsatisfied columns equals the reference's; in the batch route `status` names the reference's first failing instruction.  The info block says
which route ran, so a case cannot pass by taking another one."""
import pytest

import solver_model as M

pytestmark = pytest.mark.gpu
R = M.R
FILL = 0xA5
_results = {}


def _run(gsc, name):
    if name not in _results:
        _results[name] = M.case_table()[name].call(gsc, FILL)
    return _results[name]


def _rows(buf, batch):
    """bytes [row][column][32] -> rows of stored integers"""
    n = len(buf) // (32 * batch)
    return [[int.from_bytes(buf[32 * (r * batch + p):32 * (r * batch + p) + 32], "little") for p in range(batch)] for r in range(n)]


def _compare(case, res):
    desc, cols, masks, commits = case.made()
    ref = case.reference()
    B, n, n_in = case.batch, case.ncols(), desc["n_public"] + desc["n_secret"]
    assert res["rc"] == 0, res["why"]
    assert res["info"][7] == 0, "a resident launch gave up at its barrier"
    unsat = {p for p in range(n) if isinstance(ref[p], int)}
    assert bool(unsat) == case.expect_fail
    assert {p for p in range(n) if res["status"][p] != 0xFFFFFFFF} == unsat
    if case.mode == 1 and case.expect_flag is not None:
        assert res["flag"] == case.expect_flag
        if case.expect_flag:
            return      # mispredicted: the engine solves the chunk again generically, no row of this attempt is read
    if case.mode == 0 and not case.nproofs:      # status names the first failing instruction (its index in the level schedule)
        order = M.schedule(desc)[0]
        for p in unsat:
            assert res["status"][p] == order.index(ref[p]), (p, res["status"][p], ref[p])
    got = [_rows(res[k], B) for k in "WABC"]
    fill = int.from_bytes(bytes([FILL]) * 32, "little")
    for k in range(4):
        for r, row in enumerate(got[k]):
            for p in range(B):
                if p >= n:      # resident path: columns at or beyond nproofs keep what they held
                    assert row[p] == (fill if k or r >= n_in else (1 if r == 0 else cols[p][r - 1]) * M.MONT % R), ("untouched", "WABC"[k], r, p)
                elif p not in unsat:
                    assert row[p] < R and row[p] * M.MONT_INV % R == ref[p][k][r], ("WABC"[k], r, p)
    for r in range(n_in):      # the input rows of W are unchanged
        assert got[0][r] == [(1 if r == 0 else cols[p][r - 1]) * M.MONT % R for p in range(B)], r


@pytest.mark.parametrize("name", M.case_names(mode=0, resident=False))
def test_batch_kernels_match_the_reference(gsc, name):
    case = M.case_table()[name]
    res = _run(gsc, name)
    _compare(case, res)
    assert res["info"][4] == (8 if case.batch <= 2048 else 4) and res["info"][6] == 0


@pytest.mark.parametrize("name", M.case_names(mode=0, resident=True))
def test_resident_kernels_match_the_reference(gsc, name):
    case = M.case_table()[name]
    res = _run(gsc, name)
    _compare(case, res)
    assert res["info"][4] == 0 and res["info"][6] >= 1
    if case.workgroups:
        assert res["info"][5] == case.workgroups


@pytest.mark.parametrize("name", M.case_names(mode=1))
def test_small_integer_kernels_match_the_reference(gsc, name):
    case = M.case_table()[name]
    res = _run(gsc, name)
    assert res["info"][8] == 1, res["why"]
    _compare(case, res)


def test_every_generic_route_ran(gsc):
    infos = {n: _run(gsc, n)["info"] for n in M.case_names(mode=0)}
    batch = {n: i for n, i in infos.items() if not M.case_table()[n].nproofs}
    few = {n: i for n, i in infos.items() if M.case_table()[n].nproofs}
    assert {i[4] for i in batch.values()} == {8, 4}                                           # WPB 8 and WPB 4
    assert {i[2] for i in batch.values()} == {0, 1} and {i[2] for i in few.values()} == {0, 1}      # HAS_DIV true and false
    assert any(i[9] and i[11] for i in batch.values())                                         # a level with n_long > 0
    assert any(i[10] for i in batch.values()) and any(i[10] for i in few.values())             # a count level on both paths
    assert any(i[6] > 1 for i in few.values())                                                 # generic levels split by a count level: two launches
    assert not any(i[7] for i in few.values())                                                 # no resident launch gave up
    assert {i[5] for i in few.values()} >= {1, 17, 128}                                        # the caller's grids and the engine's choice
    mix = infos["level_mix"]
    assert mix[0] == 1 and mix[14] == (0 | 3 << 1 | 16 << 12)                                  # 3 long ops and 13 short ones in one level
    d = infos["depth_40"]
    assert d[0] == 40 and all(d[14 + l] == 2 << 12 for l in range(18))
    rc = infos["randomize_commit_70"]
    assert rc[1] < rc[0] and rc[14 + rc[1]] == 1 << 12                                         # the commitment in a level of its own


def test_every_small_route_ran(gsc):
    infos = {n: _run(gsc, n)["info"] for n in M.case_names(mode=1)}
    assert all(i[8] == 1 for i in infos.values())
    assert max(i[13] for i in infos.values()) > 16           # the chain with more than one bundle per wave (16 waves share a level's bundles)
    assert min(i[13] for i in infos.values() if i[12]) <= 16
    assert any(_run(gsc, n)["flag"] for n in infos) and not all(_run(gsc, n)["flag"] for n in infos)


def test_small_path_refuses_what_it_cannot_solve(gsc):
    for what, (build, why) in M.small_refusals().items():
        c, cols = build(64)
        case = M.Case("refusal", lambda batch, c=c, cols=cols: (c, cols), mode=1,
                      classes=lambda desc, ref, c=c: ([1] * c.n_wires, [1] * c.n_constraints, [1] * c.n_constraints, [1] * c.n_constraints))
        res = case.call(gsc)
        assert res["rc"] == -2 and why in res["why"] and res["info"][8] == 0, (what, res["rc"], res["why"])


def test_malformed_calls_are_refused(gsc):
    good = M.case_table()["status_first_failure"]
    desc, cols, _, _ = good.made()
    in_W = b"".join(M.to_mont_bytes(1 if w == 0 else cols[p][w - 1]) for w in range(desc["n_public"] + desc["n_secret"]) for p in range(64))
    assert gsc.debug_solve(desc, in_W)["rc"] == 0
    for what, (bad, why) in M.malformed_descriptions().items():
        n_in = bad["n_public"] + bad["n_secret"]
        res = gsc.debug_solve(bad, M.to_mont_bytes(1) * (64 * n_in))
        assert res["rc"] == -1, what
        if why:
            assert res["why"] == why, (what, res["why"])
        assert res["status"] == [0] * 64 and not any(res["W"]), what      # nothing ran, nothing came back
    assert "coefficient ids 0..4" in gsc.debug_solve(M.malformed_descriptions()["coefficient ids 0..4 wrong"][0], M.to_mont_bytes(1) * (64 * 3))["why"]
    assert "index column" in gsc.debug_solve(M.malformed_descriptions()["an index column that is not 0..n-1"][0], M.to_mont_bytes(1) * (64 * 3))["why"]
    assert gsc.debug_solve(desc, in_W, batch=64, nproofs=33)["rc"] == -1
    assert gsc.debug_solve(desc, in_W + in_W[:len(in_W) // 2], batch=96)["rc"] == -1
    need = 32 * 64 * (desc["n_public"] + desc["n_secret"] + desc["n_internal"])
    assert gsc.debug_solve(desc, in_W, caps=[need - 1] + [32 * 64 * desc["n_constraints"]] * 3)["rc"] == -1      # a buffer too small
    assert gsc.debug_solve(desc, in_W)["rc"] == 0
