"""The quotient fold as three group transforms on the device (k_quot_bases.hip).

The hook gsc_debug_quot_fold_dft runs launch_quot_fold_dft on caller-supplied bases U_i = u_i G, V_i = v_i G of known exponents; the expected
U', V' come from the DENSE formulas on the exponents (quot_fold_model.fold_dense) and a pure-Python scalar multiplication, compared byte for
byte with their infinity flags.  L = 4 and 6 are the smallest domains at which the index negation, the (k + 1) mod n wrap, g^_0 and the
bit-reversed loads of the second pass can go wrong; every m at which a set is empty or a single element is there.

Then whole provers in child processes: ChaCha20-V3's transforms must build the sets that the engine's dense sums built before they were retired
(digests of 64 proofs and of the +-1 quotient sums, recorded from that route: tests/golden/quot_fold_chacha20_dense.json), GSC_QUOTIENT_FOLD=2
still means folded, and AES-128 folded against unfolded: the same proof bytes, accepted by libverify, and the same quotient sums for inputs
whose every c_i is +-1."""
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import quot_fold_model as qm
from conftest import ROOT, golden_bytes
from quot_fold_model import R

pytestmark = pytest.mark.gpu


# ---- the hook on small domains ------------------------------------------------------------------------------------------------------------
def _points(exps):
    enc = [qm.g1_mul(e) for e in exps]
    return b"".join(p for p, _ in enc), bytes(f for _, f in enc)


def _run(gsc, L, m, perm, u, v, identity_as_null=False):
    """the hook's (U', flags, V', flags) and the same from the dense formulas on the exponents"""
    n = 1 << L
    ub, uf = _points(u)
    vb, vf = _points(v)
    got = gsc.debug_quot_fold_dft(L, m, None if identity_as_null else perm, ub, uf, vb, vf)
    U2, V2 = qm.fold_dense(qm.Domain(n), m, perm, u, v)
    assert len(U2) + len(V2) == 2 * m - 1 <= 127
    return got, _points(U2) + _points(V2), (U2, V2)


@pytest.mark.parametrize("kind", ["identity", "scattered"])
@pytest.mark.parametrize("L,m", [(L, m) for L in (4, 6) for m in (2, (1 << L) // 2, (1 << L) // 2 + 1, (1 << L) - 1, 1 << L)])
def test_hook_equals_the_dense_formulas_on_known_exponents(gsc, L, m, kind):
    n = 1 << L
    rng = random.Random(1000 * L + 10 * m + len(kind))
    perm = list(range(n))
    if kind == "scattered":
        rng.shuffle(perm)
    u, v = [rng.randrange(1, R) for _ in range(m)], [rng.randrange(1, R) for _ in range(n)]
    got, want, _ = _run(gsc, L, m, perm, u, v, identity_as_null=kind == "identity")      # (NULL stands for the identity)
    assert got[1] == bytes(m) and got[3] == bytes(m - 1)
    assert got == want


def test_hook_with_the_engines_table_order_and_inputs_at_infinity(gsc):
    L, m = 4, 9
    n, rng = 1 << L, random.Random(77)
    perm = qm.table_order(n)
    u, v = [rng.randrange(1, R) for _ in range(m)], [rng.randrange(1, R) for _ in range(n)]
    u[0] = u[3] = u[m - 1] = 0                         # U_i at infinity on input: U'_i is the folded sum alone
    v[2] = 0                                           # a live V, and a dropped one: its share is missing from every sum
    v[m + 1] = 0
    got, want, (U2, V2) = _run(gsc, L, m, perm, u, v)
    assert all(U2) and all(V2)
    assert got == want


def test_hook_flags_a_folded_base_that_is_the_point_at_infinity(gsc):
    L, m = 4, 9
    n, rng = 1 << L, random.Random(78)
    perm = qm.table_order(n)
    u, v = [rng.randrange(1, R) for _ in range(m)], [rng.randrange(1, R) for _ in range(n)]
    # the folded sums do not depend on u or on the live v: choose u_5 and v_3 as minus their sums
    S_u, S_v = qm.fold_dense(qm.Domain(n), m, perm, [0] * m, [0] * (m - 1) + v[m - 1:])
    u[5], v[3] = -S_u[5] % R, -S_v[3] % R
    got, want, (U2, V2) = _run(gsc, L, m, perm, u, v)
    assert [i for i in range(m) if not U2[i]] == [5] and [i for i in range(m - 1) if not V2[i]] == [3]
    assert got[1] == bytes(5) + b"\x01" + bytes(m - 6)                 # U'_5 comes back flagged ...
    assert got[3] == bytes(3) + b"\x01" + bytes(m - 5)                 # ... and so does V'_3: reported, not dropped
    assert got[0][64 * 5:64 * 6] == bytes(64) and got[2][64 * 3:64 * 4] == bytes(64)
    assert got == want


def test_hook_refuses_arguments_outside_its_range(gsc):
    ub, uf = _points([1, 2])
    vb, vf = _points(list(range(1, 5)))
    with pytest.raises(RuntimeError):
        gsc.debug_quot_fold_dft(2, 2, [0, 1, 2, 2], ub, uf, vb, vf)    # not a permutation
    lib = gsc.lib()
    out = [bytes(64 * 4), bytes(4), bytes(64 * 4), bytes(4)]
    for L, m in ((1, 2), (18, 2), (2, 1), (2, 5)):
        assert lib.gsc_debug_quot_fold_dft(L, m, None, ub, uf, vb, vf, *out) == -1, (L, m)
    assert gsc.debug_quot_fold_dft(2, 2, None, ub, uf, vb, vf)[1] == bytes(2)


# ---- whole provers: the sets the engine builds ------------------------------------------------------------------------------------------------
N = 64

_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import bench, gsc_loader
g = gsc_loader.load()
algo, rows = int(sys.argv[6]), int(sys.argv[8])
name = ["chacha20", "aes-128-ctr"][algo]
pk = open(sys.argv[7], "rb").read() if algo else bench.golden("pk.chacha20")
assert g.init_algorithm(algo, pk, bench.golden(["r1cs.chacha20", "r1cs.aes128"][algo]))
print("DESCRIBE", g.describe(algo))
n = 64
recs = bench.provable(bench.xoshiro_records(n, 0xD0F7 << 20), name)
g.set_deterministic_randomness(int(sys.argv[3]), int(sys.argv[4]), 0x5555)
ok, proofs, lens, cts = g.prove_raw(algo, recs, n)
assert ok == n and set(lens) == {196 if algo else 164}, (ok, set(lens))
kname, ms, stmts, cols, nb = g.last_dominant_kernel(algo)
assert kname.startswith("k_msm_win") and nb == [32768, 131072][algo], (kname, nb)      # the set's n positions, folded or not
abc = open(sys.argv[5], "rb").read()
assert len(abc) == 3 * rows * 64 * 32
pts, flags = g.debug_z_sum(algo, abc, rows)
open(sys.argv[2], "wb").write(recs + proofs + cts + pts + flags)
print("CHILD-OK")
"""


def _signed_rows(rng, rows):
    """a, b, c = a b: [rows][64] big-endian field elements, every entry +-1"""
    one = np.frombuffer((1).to_bytes(32, "big"), np.uint8)
    minus = np.frombuffer((R - 1).to_bytes(32, "big"), np.uint8)
    sa, sb = rng.integers(0, 2, (rows, 64), dtype=np.uint8), rng.integers(0, 2, (rows, 64), dtype=np.uint8)
    mats = [np.where(s[:, :, None] == 1, minus, one) for s in (sa, sb, sa ^ sb)]
    return np.stack(mats).astype(np.uint8).tobytes()


def _children(tmp, algo, folds, rows, pk_path="-", extra=()):
    abc_path = str(tmp / "abc.bin")
    open(abc_path, "wb").write(_signed_rows(np.random.default_rng(0xD0F7 + algo), rows))
    r, s = 0x1234567, 0xabcdef0123456789abcdef
    out = {}
    for fold in folds:
        env = {k: v for k, v in os.environ.items() if not k.startswith("GSC_")}
        env.update({"GSC_MAX_BATCH": "64", "GSC_WINDOW_Z": "8", "GSC_W_TABLE_GB": "8", "GSC_ENABLE_TEST_HOOKS": "1"})
        env.update(extra)
        if fold is not None:
            env["GSC_QUOTIENT_FOLD"] = fold
        path = str(tmp / ("out%s.bin" % fold))
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path, str(r), str(s), abc_path, str(algo), pk_path, str(rows)], env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
        blob = open(path, "rb").read()
        cut = [112 * N, 196 * N, 64 * N, 64 * 64, 64]
        assert len(blob) == sum(cut)
        parts, at = [], 0
        for c in cut:
            parts.append(blob[at:at + c]); at += c
        out[fold] = dict(zip(("recs", "proofs", "cts", "pts", "flags"), parts), describe=[l for l in p.stdout.splitlines() if l.startswith("DESCRIBE")][0])
    return out


def _same_outputs(a, b, proof_len):
    assert a["recs"] == b["recs"] and a["cts"] == b["cts"]
    assert a["proofs"] == b["proofs"]
    assert len({a["proofs"][196 * k:196 * k + proof_len] for k in range(N)}) == N
    assert a["flags"] == b["flags"] == bytes(64)                        # no column sums to the point at infinity
    assert a["pts"] == b["pts"]
    assert len({a["pts"][64 * k:64 * k + 64] for k in range(64)}) == 64      # 64 different columns, 64 different points


def _field(describe, key):
    return [w for w in describe.split() if w.startswith(key + "=")][0].split("=", 1)[1]


@pytest.fixture(scope="module")
def chacha_runs(tmp_path_factory):
    return _children(tmp_path_factory.mktemp("fold_dft_chacha"), 0, (None, "2"), 23617)


def test_chacha20_transforms_build_the_sets_the_dense_sums_built(chacha_runs):
    """tests/golden/quot_fold_chacha20_dense.json: digests of what this very child gave when the sets were folded term by term (the retired dense
    route, GSC_QUOTIENT_FOLD=1 at the commit the file names; it agreed there, byte for byte, with the transforms)."""
    want = json.loads(golden_bytes("quot_fold_chacha20_dense.json"))
    run = chacha_runs[None]
    assert " Z=32768 " in run["describe"] and "Zlive=23616 " in run["describe"] and "Zfold=dft " in run["describe"], run["describe"]
    assert (want["proofs"], want["proof_bytes"], want["rows"]) == (N, 164, 23617)
    proofs = [run["proofs"][196 * k:196 * k + 164] for k in range(N)]
    assert hashlib.sha256(b"".join(proofs)).hexdigest() == want["sha256_proofs"]
    assert hashlib.sha256(run["pts"] + run["flags"]).hexdigest() == want["sha256_points_flags"]
    assert len(set(proofs)) == N
    assert run["flags"] == bytes(64)                                       # no column sums to the point at infinity
    assert len({run["pts"][64 * k:64 * k + 64] for k in range(64)}) == 64      # 64 different columns, 64 different points


def test_chacha20_knob_value_2_still_means_folded(chacha_runs):
    # (2 used to choose the transforms over the dense sums: hosts that set it keep initialising, and get the default)
    default, two = chacha_runs[None], chacha_runs["2"]
    for key in ("Z", "Zlive", "Zfold", "Qtiles"):
        assert _field(two["describe"], key) == _field(default["describe"], key), (key, two["describe"])
    assert _field(two["describe"], "Zfold") == "dft"


@pytest.fixture(scope="module")
def aes_runs(aes_keys, tmp_path_factory):
    pk_path = os.path.join(ROOT, "build", "keys", "pk.aes128")
    assert os.path.exists(pk_path)
    # (no latency layouts: these children prove one batch of 64 and share the device with the session's own algorithms)
    return _children(tmp_path_factory.mktemp("fold_dft_aes"), 1, (None, "0"), 8192, pk_path, {"GSC_FEW_Z_GB": "0", "GSC_FEW_WIDE": "0"})


def test_aes128_is_folded_by_default_and_says_so(aes_runs):
    on, off = aes_runs[None], aes_runs["0"]
    m = int(_field(on["describe"], "constraints"))
    assert _field(on["describe"], "domain") == "2^17" and 2 <= m < 131072
    assert _field(on["describe"], "Zlive") == str(m - 1) and _field(on["describe"], "Zfold") == "dft", on["describe"]
    assert "Zlive" not in off["describe"] and "Zfold=off(GSC_QUOTIENT_FOLD=0)" in off["describe"], off["describe"]
    assert _field(on["describe"], "Z") == _field(off["describe"], "Z") == "131072"


def test_aes128_folded_and_unfolded_sets_give_the_same_proofs_and_sums(aes_runs):
    # (the sums: a, b with entries +-1 on the first 8192 rows — the hook cases above are what weigh every U')
    _same_outputs(aes_runs[None], aes_runs["0"], 196)


def test_aes128_proofs_from_the_folded_sets_verify(gsc, aes_runs, aes_keys):
    sys.path.insert(0, ROOT)
    import bench
    on = aes_runs[None]
    assert gsc.init_verifier(1, aes_keys["aes128"][2])
    items = [("aes-128-ctr", on["proofs"][196 * k:196 * k + 196], bench.signals_of("aes-128-ctr", on["recs"][112 * k:112 * (k + 1)], on["cts"][64 * k:64 * k + 64])) for k in range(N)]
    assert bench.verify_items(gsc, items) == [True] * N
