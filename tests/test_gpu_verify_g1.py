"""GPU unit tests of the verifier's G1 stage, everything between a proof's bytes and the first Miller loop, through gsc_debug_verify_g1
(include/libprove.h): k_verify_key_points, k_verify_tables, k_verify_prep, k_verify_batch_scale / _sum and k_verify_claims_scale / _sums / _fixed,
run by build_key, prep_chunk and the production launchers on trapdoor keys (tests/verifymodel.py): every key point a known multiple of the
generator, every proof a tuple of logarithms, the randomizers chosen by the test.  The expected bytes are integer arithmetic mod r followed by one
multiplication of the generator, and the comparison is exact on EVERY returned field of every proof, part and table entry: the key points' status,
both window tables, ok, A, B, C, L, D, PoK, rho A, the batched check's okv, the fixed points and the flag of the chunk and of every part, the parts'
sums of rho.  One exception, fixed here before any run: in the large case (4097 proofs) rho A is compared for the proofs at positions 0 and 63 of
every block of 64 and for the designated special proofs only (verifymodel._large_case); its sums depend on every proof all the same.

The cases reach what honest keys with random randomizers never do: equal and opposite operands in lsum, in the table builders and in every
reduction tree, points at infinity everywhere, undecodable columns between valid ones, sums of rho that carry into the fifth word, parts of 1, 2, 63,
64, 65 and 129 proofs, 65 blocks.  tests/test_verify_g1_model_host.py proves the model and the table on a CPU first, and that every case reaches
what it claims; a failure here lies in the device mapping.

The last tests need no hook: with the trapdoor, valid proofs exist by construction, so the public entry points are held against the model's verdicts
and libverify.so's on ordinary and degenerate valid proofs and on each of them with one coordinate or one public byte changed."""
import ctypes

import pytest

import keyraw as KR
import verifymodel as M
from conftest import golden_bytes

pytestmark = pytest.mark.gpu
KEYS = ("chacha_plain", "chacha_coll", "aes_plain", "aes_coll", "aes_linf")
_runs = {}


def _run(gsc, key_name, shape, path=1, fill=M.FILL):
    """one call of the hook per (case, path, fill), shared by the tests that read it"""
    at = (key_name, shape, path, fill)
    if at not in _runs:
        c = M.case(key_name, shape)
        proofs, lens, sigs, rnd = c.inputs()
        _runs[at] = gsc.debug_verify_g1(c.key.algo, c.key.vk_bytes(), proofs, lens, sigs, rnd, ends=c.ends, path=path, fill=fill)
        assert _runs[at]["rc"] == 0
    return _runs[at]


@pytest.mark.parametrize("key_name", KEYS)
def test_key_points_and_window_tables(gsc, key_name):
    """all 144 x 256 (and 32 x 256) entries, and k_verify_key_points' status of every key point in either encoding"""
    c = M.case(key_name, 1)
    res = _run(gsc, key_name, 1)
    table, ctable = c.expected_tables()
    assert res["key_status"][:len(c.key.key_status())] == c.key.key_status()
    assert res["key_status"][len(c.key.key_status()):] == bytes([M.FILL]) * (len(res["key_status"]) - len(c.key.key_status()))
    assert not M.table_mismatches(res["table"], table)[:6]
    assert not M.table_mismatches(res["ctable"], ctable)[:6]
    assert not M.mismatches(c, res, c.expected())[:6]


@pytest.mark.parametrize("shape", (63, 64, 65, 130, "valid66"))
@pytest.mark.parametrize("key_name", KEYS)
def test_chunk(gsc, key_name, shape):
    c = M.case(key_name, shape)
    want = c.expected()
    assert want["flag"] == (b"\1" if shape == "valid66" else b"\0")
    assert not M.mismatches(c, _run(gsc, key_name, shape), want)[:6]


@pytest.mark.parametrize("path", (1, 2))
@pytest.mark.parametrize("key_name", KEYS)
def test_parts(gsc, key_name, path):
    """parts of 1, 2, 63, 64, 65 and 129 proofs in one chunk, on both Miller paths"""
    c = M.case(key_name, "parts")
    want = c.expected()
    assert list(want["pflag"]) == [1, 1, 1, 1, 0, 1] and want["flag"] == b"\0"
    assert not M.mismatches(c, _run(gsc, key_name, "parts", path), want)[:6]


@pytest.mark.parametrize("shape", (1, 65, "valid66"))
@pytest.mark.parametrize("key_name", KEYS)
def test_chunk_on_the_few_proof_path(gsc, key_name, shape):
    c = M.case(key_name, shape)
    assert not M.mismatches(c, _run(gsc, key_name, shape, 2), c.expected())[:6]


@pytest.mark.parametrize("path", (1, 2))
def test_large_chunk_of_65_blocks(gsc, path):
    c = M.case("chacha_plain", "large")
    want = c.expected()
    assert want["flag"] == b"\1" and sum(want["ok"]) == c.n - 4
    assert not M.mismatches(c, _run(gsc, "chacha_plain", "large", path), want)[:6]


def test_another_fill_byte(gsc):
    """what the kernels leave alone keeps whatever was there: the points of a proof without ok, D without a commitment, the parts' Pedersen pairs"""
    c = M.case("chacha_coll", "parts")
    res = _run(gsc, "chacha_coll", "parts", 1, 0x00)
    assert not M.mismatches(c, res, c.expected(fill=0x00))[:6]
    assert res["ctable"] == bytes(len(res["ctable"])) and res["g1"][65 * 3:65 * 4] == bytes(65)


def test_refusals(gsc, capfd):
    """bad arguments: -1 and a line; a key with a point off the curve: -2; a key of another circuit: -3; nothing is written"""
    c = M.case("chacha_plain", 1)
    proofs, lens, sigs, rnd = c.inputs()
    vk = c.key.vk_bytes()

    def printed():
        ctypes.CDLL(None).fflush(None)
        return capfd.readouterr().out
    printed()
    call = lambda **kw: gsc.debug_verify_g1(kw.pop("algo", 0), kw.pop("vk", vk), proofs, lens, sigs, rnd, **kw)
    untouched = lambda res: all(set(res[k]) <= {M.FILL} for k in ("key_status", "table", "ok", "g1", "g2", "okv", "fixed", "flag"))
    for kw, rc, why in (({"path": 0}, -1, "path is 1 or 2"), ({"path": 3}, -1, "path is 1 or 2"), ({"ends": (2,)}, -1, "part ends"), ({"algo": 3}, -1, "algorithm is 0 .. 2"),
                        ({"vk": vk[:-1]}, -2, "vk: "), ({"algo": 1}, -3, "not one of the algorithm's circuit")):
        res = call(**kw)
        assert res["rc"] == rc and untouched(res), why
        assert why in printed(), why
    x = 4
    while KR.sqrt_fp(KR.g1_rhs(x)) is not None:
        x += 1
    at = 64                    # beta in G1, compressed, behind the raw alpha
    res = call(vk=vk[:at] + bytes([0x80]) + KR.be(x)[1:] + vk[at + 32:])
    assert res["rc"] == -2 and untouched(res) and "vk: bad point" in printed()
    assert call()["rc"] == 0


def test_every_branch_was_reached():
    """each item of the list of what honest inputs never reach has a case; the model's own evidence (verifymodel.reached), not an instrumented device"""
    got = set()
    for key_name, shape in M.CASES:
        got |= M.reached(M.case(key_name, shape))
    assert got >= set(M.WHY), sorted(set(M.WHY) - got)


# ---- verdicts on trapdoor keys through the public entry points ----
def _items(key_name):
    """(name, proof bytes, length, signals, the model's verdict): every column; each valid one with a bit of C's x changed, and with a public byte changed"""
    cols, out = M.columns(key_name), []
    for p in cols.all():
        slot, length = p.slot()
        out.append((p.name, slot, length, p.sig, p.verdict()))
    for p in cols.valid:
        slot, length = p.slot()
        b = bytearray(slot); b[96 + 31] ^= 1
        out.append((p.name + "/C.x", bytes(b), length, p.sig, 0))
        w = bytearray(p.win); w[77] ^= 0x10
        q = M.Proof(p.name + "/public", p.key, bytes(w), p.A, p.B, p.C, p.D, p.PoK, a_point=p.a_point)
        out.append((q.name, slot, length, q.sig, q.verdict()))
    return out


@pytest.fixture(scope="module")
def trapdoor_verifiers(gsc):
    """the trapdoor keys that have a valid proof with L at infinity, in the GPU verifier and in libverify.so; the golden keys and the automatic
    path come back afterwards"""
    names = {0: "chacha_coll", 1: "aes_linf"}
    try:
        for algo, name in names.items():
            vk = M.keys()[name].vk_bytes()
            assert gsc.verify_init(algo, vk) and gsc.init_verifier(algo, vk)
        yield names
    finally:
        gsc.debug_verify_path(0)
        for algo, name in ((0, "vk.chacha20"), (1, "vk.aes128")):
            assert gsc.verify_init(algo, golden_bytes(name)) and gsc.init_verifier(algo, golden_bytes(name))


def _model_and_libverify(gsc, algo, items):
    want = [v for *_, v in items]
    for name, slot, length, sig, v in items:
        assert int(gsc.verify({"cipher": gsc.ALGORITHM_NAMES[algo], "proof": slot[:length], "publicSignals": sig})) == v, name
    return want


@pytest.mark.parametrize("algo", (0, 1))
def test_verdicts_proof_by_proof(gsc, trapdoor_verifiers, algo):
    items = _items(trapdoor_verifiers[algo])
    want = _model_and_libverify(gsc, algo, items)
    for tag in ("A_inf", "C_inf", "L_inf") + (("D_PoK_inf",) if algo else ()):
        assert any(n.startswith(tag) and v == 1 for n, *_, v in items), tag
    assert 20 <= len(items) and sum(want) == len(M.columns(trapdoor_verifiers[algo]).valid) + (0 if algo else 1)
    args = (algo, b"".join(s for _, s, *_ in items), [l for _, _, l, *_ in items], b"".join(s for *_, s, _ in items))
    for path in (1, 2):
        assert gsc.debug_verify_path(path) == 0
        assert gsc.verify_raw(*args) == want and gsc.verify_last_path(algo) == path
        assert gsc.verify_raw_batched(*args) == want
    assert gsc.debug_verify_path(0) == 0
    assert gsc.verify_all(*args) == 0
    good = [it for it in items if it[4]]
    gargs = (algo, b"".join(s for _, s, *_ in good), [l for _, _, l, *_ in good], b"".join(s for *_, s, _ in good))
    assert gsc.verify_all(*gargs) == 1 and gsc.verify_raw_batched(*gargs) == [1] * len(good)


@pytest.mark.parametrize("algo", (0, 1))
def test_verdicts_claim_by_claim(gsc, trapdoor_verifiers, algo):
    """a degenerate valid proof alone, first and last in a claim; claims that hold one changed item fail, the others hold"""
    items = _items(trapdoor_verifiers[algo])
    good, bad = [it for it in items if it[4]], [it for it in items if not it[4]]
    deg = [it for it in good if it[0].split("/")[0] in ("A_inf", "C_inf", "L_inf", "L_inf_commit", "D_PoK_inf")]
    assert len(deg) >= 3
    claims = []
    for d in deg:
        claims += [[d], [d] + good[:3], good[:3] + [d], [d] + good[:2] + [bad[len(claims) % len(bad)]], [bad[(len(claims) + 1) % len(bad)]] + good[:2] + [d]]
    claims.append(good)
    flat = [it for cl in claims for it in cl]
    ends, at = [], 0
    for cl in claims:
        at += len(cl); ends.append(at)
    want = [int(all(it[4] for it in cl)) for cl in claims]
    assert 0 < sum(want) < len(want)
    _model_and_libverify(gsc, algo, deg)
    for path in (1, 2):
        assert gsc.debug_verify_path(path) == 0
        assert gsc.verify_claims(algo, b"".join(it[1] for it in flat), [it[2] for it in flat], b"".join(it[3] for it in flat), ends) == want
    assert gsc.debug_verify_path(0) == 0
