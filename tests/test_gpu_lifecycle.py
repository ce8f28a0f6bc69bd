"""Key lifecycle on the device: gsc_release_algorithm, gsc_replace_algorithm, gsc_memory_info, gsc_key_generation.

Every case runs in a prover process of its own (tests/lifecycle_child.py: the session's fixtures keep their algorithms loaded), one at a time,
with the small engine of tests/test_gpu_quot_fold.py (c = 8, 64 proofs per lane: an init takes about a second); after a child that aborted or
ran into its time limit no further child is started.  Key A is the golden pk.chacha20 / vk.chacha20, key B comes from gsc_setup on the same
circuit with a fixed seed; verdicts are gsc_verify_raw's under vk A or vk B; 65 statements (two 64-column groups) under fixed randomness, and
one of them once more as a single Prove through the micro-batcher.

The memory margin of the release case: what the one unwinding path the parent commit has — a key refused at its last G2 point — leaves behind
between three refused InitAlgorithm calls of one process (profiles/r18_unwind_parent.txt: free memory moved by at most UNWIND_LEFT bytes), plus one
allocation granule of the runtime (GRANULE, 2 MiB: the step in which hipMemGetInfo's free moved there) for the stream and event objects a live
engine adds.  The library's own count is exactly 0 whatever the runtime keeps.  Measured: the three refused inits left the
same 308 056 948 736 bytes free, difference 0; free memory after the three releases of the release case: 307 289 391 104 bytes each, difference 0
(engines on new streams instead of pooled ones: the second release 922 746 880 bytes below the first, the runtime's per-queue scratch)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

N = 65
SMALL_ENGINE = {"GSC_MAX_BATCH": "64", "GSC_WINDOW_Z": "8", "GSC_W_TABLE_GB": "8", "GSC_ENABLE_TEST_HOOKS": "1"}
NOT_INIT = '"proving params are not initialized for cipher: chacha20"'
UNWIND_LEFT = 0
GRANULE = 2 << 20
_state = {"dead": None}


def _child(tmp, case, extra_env=None, timeout=300):
    if _state["dead"]:
        pytest.fail("not started: the child of case '%s' aborted or ran into its time limit" % _state["dead"])
    env = {k: v for k, v in os.environ.items() if not k.startswith("GSC_")}
    env.update(SMALL_ENGINE)
    env.update(extra_env or {})
    out = os.path.join(str(tmp), case + ".json")
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lifecycle_child.py"), ROOT, case, out, str(tmp)], env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _state["dead"] = case
        raise
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _state["dead"] = case
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    return json.load(open(out)), p.stdout


@pytest.fixture(scope="module")
def keys(tmp_path_factory):
    """the directory the children share: pk.b / vk.b from gsc_setup (made once), and their result files"""
    tmp = tmp_path_factory.mktemp("lifecycle")
    facts, _ = _child(tmp, "setup")
    assert facts["pk"] > 1 << 20 and facts["vk"] > 1000
    return tmp


@pytest.fixture(scope="module")
def replaced(keys):
    return _child(keys, "replace")[0]


def test_release_gives_everything_back_and_init_starts_afresh(keys):
    f, _ = _child(keys, "release")
    assert f["init"]["gen"] == 1 and f["init"]["provers"] > 1 << 28 and " key=%s gen=1" % f["init"]["key"] in f["describe"], f["init"]
    first_free = f["cycles"][0]["after"]["free"]
    for c in f["cycles"]:
        print("free after release: %d (first %+d), prover bytes %d" % (c["after"]["free"], c["after"]["free"] - first_free, c["after"]["provers"]))
        assert c["scan_before"] == 0 and c["release"] is True
        assert c["after"]["provers"] == 0 and c["after"]["gen"] == 0 and c["after"]["key"] is None and c["describe"] == "not initialised"
        assert c["prove"] == NOT_INIT and c["raw"] == -1
        assert c["release_again"] is False
        assert c["init"] is True and c["scan_after_init"] == 0
        assert c["again"]["gen"] == 1 and c["again"]["key"] == f["init"]["key"] and c["again"]["provers"] == f["init"]["provers"]
        assert c["same_proofs"]
        assert abs(c["after"]["free"] - first_free) <= UNWIND_LEFT + GRANULE
    # ... and the release is what gave it back: every byte the library counts was allocated on the device, so free memory rises by at least the
    # count, up to the same margin, from the engine serving (after the cycle before: the runtime's first-use allocations are behind it) to released
    for before, c in zip(f["cycles"], f["cycles"][1:]):
        assert c["after"]["free"] - before["again"]["free"] >= f["init"]["provers"] - (UNWIND_LEFT + GRANULE), (before["again"], c["after"])


def test_replace_serves_the_new_key_under_its_own_check(keys, replaced):
    f = replaced
    assert f["rc"] == 1 and f["before"]["gen"] == 1 and f["after"]["gen"] == 2
    assert f["before"]["key"] != f["after"]["key"] and len(f["after"]["key"]) == 16 and " gen=2" in f["describe"]
    assert f["after"]["provers"] == f["before"]["provers"]                     # same circuit, same settings: the old engine's bytes went, the new one's came
    assert "check=off" in f["describe_before"] and "check=on(" in f["describe"]
    assert f["stats0"] == [0, 0, 0, 0] and f["stats1"][0] >= 3 and f["stats1"][1] == N + 1 and f["stats1"][2] == 0, (f["stats0"], f["stats1"])
    assert f["under_b"] == [1] * N and f["under_a"] == [0] * N
    assert f["pb"] != f["pa"] and f["not_initialised"] == -1


def test_replaced_engine_gives_the_proofs_of_a_fresh_init(keys, replaced):
    fresh, _ = _child(keys, "fresh_b")
    assert fresh["proofs"] == replaced["pb"]
    assert fresh["key"] == replaced["after"]["key"] and fresh["gen"] == 1


def test_refused_replacement_changes_nothing(keys):
    f, out = _child(keys, "refused")
    lines = out.splitlines()
    said = lines[lines.index("REPLACE-BEGIN") + 1:lines.index("REPLACE-END")]
    assert f["rc"] == 0 and len(said) == 1 and said[0].startswith("pk: "), said         # the usual one line
    assert f["after"]["gen"] == f["before"]["gen"] == 1 and f["after"]["key"] == f["before"]["key"]
    assert f["after"]["provers"] == f["before"]["provers"] and f["after"]["verifiers"] == f["before"]["verifiers"]
    assert f["same_proofs"]
    assert f["rc_bad_vk"] == 0 and f["after_bad_vk"]["gen"] == 1 and f["after_bad_vk"]["key"] == f["before"]["key"] and "check=off" in f["describe"]
    assert f["after_bad_vk"]["provers"] == f["before"]["provers"] and f["after_bad_vk"]["verifiers"] == f["before"]["verifiers"]


def test_callers_are_served_across_swaps(keys):
    f, _ = _child(keys, "swaps")
    json_calls = lambda i: sum(d["inside"][i] for d in f["per"][:8])
    print("replace took %.2f s and %.2f s; the eight Prove callers: %.0f and %.0f proofs/s meanwhile, %.0f proofs/s with nothing building; per thread inside the replaces: %s"
          % (f["replace_s"][0], f["replace_s"][1], json_calls(0) / f["replace_s"][0], json_calls(1) / f["replace_s"][1], json_calls(2) / f["idle_s"], [d["inside"][:2] for d in f["per"]]))
    assert f["rc"] == [1, 1] and f["gens"] == [2, 3]
    for t, d in enumerate(f["per"]):
        assert d["other"] == 0 and d["not_init"] == 0, (t, d)                  # no call fails
        assert d["both"] == 0 and d["neither"] == 0 and d["a"] > 0, (t, d)      # every proof under exactly one of the two keys
        assert d["late_not_a"] == 0, (t, d)                                    # after the last replace returned: A's
        assert d["inside"][0] >= 5 and d["inside"][1] >= 5, (t, d)             # served while a replace builds
    assert sum(d["b"] for d in f["per"]) > 0
    assert f["end"]["key"] is not None and f["end"]["gen"] == 3


def test_release_under_load_serves_or_says_not_initialised(keys):
    f, _ = _child(keys, "release_load")
    print("release under nine callers took %.3f s" % f["release_s"])
    assert f["rc"] is True and f["after"]["provers"] == 0 and f["after"]["gen"] == 0
    for t, d in enumerate(f["per"]):
        assert d["other"] == 0 and d["b"] == 0 and d["both"] == 0 and d["neither"] == 0, (t, d)      # a valid proof under A, or the not-initialised answer
        assert d["a"] > 0 and d["not_init"] > 0, (t, d)
    assert f["init"] is True and f["same_proofs"]


def test_replace_and_release_cover_every_replica(keys):
    f, _ = _child(keys, "replicas", {"GSC_DEVICES": "0,0"})
    assert " devices=2 " in f["describe0"]
    assert len(f["served_a"]) == 2 and all(c > 0 for c, s in f["served_a"])
    assert f["rc"] == 1 and f["served_swapped"] == [[0, 0], [0, 0]] and f["after"]["gen"] == 2 and "check=on(" in f["describe1"]
    assert len(f["served_b"]) == 2 and all(c > 0 for c, s in f["served_b"]) and sum(s for c, s in f["served_b"]) == N + 1
    assert f["after"]["provers"] == f["before"]["provers"] and f["after"]["verifiers"] > f["before"]["verifiers"]
    assert f["release"] is True and f["end"]["provers"] == 0 and f["end"]["gen"] == 0 and f["end"]["verifiers"] == f["before"]["verifiers"]
