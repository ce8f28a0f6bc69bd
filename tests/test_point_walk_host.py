"""CPU tests of the key-point walk (csrc/formats.hpp walk_points, parse_pk): gnark's decoder reads every point of a key compressed or raw by
the flag bits of its first byte, and so does the host parser.  tests/native/point_walk_check.cpp is built from csrc/formats.cpp with g++,
once plainly and once under AddressSanitizer + UBSan (a stand-alone program run as its own process: these are parsers of caller bytes),
and run on synthetic slices and on the reference's pk.chacha20, unmodified and with points rewritten to the raw form (tests/keyraw.py)."""
import os
import struct
import subprocess

import pytest

import keyraw
from conftest import ROOT, golden_bytes

CSRC = os.path.join(ROOT, "gnark-symmetric-crypto_amd", "csrc")
BUILD = os.path.join(ROOT, "build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-static-libasan", "-static-libubsan"]


def _build(name, extra):
    exe = os.path.join(BUILD, name)
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra +
                          ["-o", exe, os.path.join(ROOT, "tests", "native", "point_walk_check.cpp"), os.path.join(CSRC, "formats.cpp")])
    return exe


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def walk_exe(request):
    return _build("point_walk_check_" + request.param, SAN if request.param != "plain" else [])


def _run(exe, *args):
    # the sanitized build is a stand-alone program with its own instrumented main and the runtimes linked in statically: whatever else the
    # environment preloads into a process, the runtime's position in the link order says nothing about this program
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120, env=env)


def test_synthetic_slices(walk_exe):
    """0, 1, 2 and 5 elements, all compressed / all raw / alternating / raw last, every truncation, counts the bytes cannot hold"""
    out = _run(walk_exe, "self")
    assert out.returncode == 0 and "WALK-OK" in out.stdout, out.stdout + out.stderr


def _dump(exe, key_bytes, tag):
    src, dst = os.path.join(BUILD, "walk_%s.pk" % tag), os.path.join(BUILD, "walk_%s.sets" % tag)
    open(src, "wb").write(key_bytes)
    out = _run(exe, "pk", src, dst)
    if out.returncode != 0:
        return out, None
    b = open(dst, "rb").read()
    sets, o = {}, 0
    while o < len(b):
        ln, = struct.unpack_from("<I", b, o); o += 4
        name = b[o:o + ln].decode(); o += ln
        n, nx = struct.unpack_from("<QQ", b, o); o += 16
        x = b[o:o + nx]; o += nx
        ny, = struct.unpack_from("<Q", b, o); o += 8
        y = b[o:o + ny]; o += ny
        sets[name] = (n, x, y)
    return out, sets


@pytest.fixture(scope="module")
def third_raw_pk():
    """pk.chacha20 with every third point of the first 300 of each slice (and alpha / beta / delta of both groups) raw"""
    pk = golden_bytes("pk.chacha20")
    choose = lambda name, i: i < 300 and i % 3 == 0
    return pk, keyraw.rewrite_pk(pk, choose), choose


def test_reference_pk_compressed_and_mixed(walk_exe, third_raw_pk):
    pk, mixed, choose = third_raw_pk
    assert len(mixed) > len(pk)
    out0, base = _dump(walk_exe, pk, "plain")
    out1, got = _dump(walk_exe, mixed, "mixed")
    assert base is not None and got is not None, out0.stdout + out0.stderr + out1.stdout + out1.stderr
    assert out0.stdout == out1.stdout                                  # the same domain and wire counts
    secs = {name: (group, elems) for name, group, _, elems in keyraw.pk_sections(pk)}
    for name, (n, x, y) in base.items():
        assert y == b"", name                                          # a compressed-only key: no y bytes anywhere, x as stored
        if name in secs:
            group, elems = secs[name]
            assert n == len(elems) and x == b"".join(pk[o:o + sz] for o, sz in elems), name
        else:
            assert n == 0                                              # ChaCha20-V3 has no commitment key
    nraw = 0
    for name, (n, x, y) in got.items():
        n0, x0, _ = base[name]
        assert n == n0, name                                           # the same point counts
        if not n:
            continue
        group, elems = secs[name]
        cb = 32 if group == 0 else 64
        assert len(x) == n * cb and len(y) == n * cb, name             # every set of this key has a raw element
        for i, (o, sz) in enumerate(elems):
            xi, yi, x0i = x[cb * i:cb * i + cb], y[cb * i:cb * i + cb], x0[cb * i:cb * i + cb]
            if choose(name, i):
                raw = keyraw.to_raw(group, pk[o:o + sz])
                assert xi[0] & 0xC0 == 0 and xi == raw[:cb] and yi == raw[cb:], (name, i)      # y exactly where it was supplied
                assert xi[1:] == x0i[1:] and xi[0] == x0i[0] & 0x3F, (name, i)                  # ... and the x of the compressed form
                nraw += 1
            else:
                assert xi == x0i and yi == bytes(cb), (name, i)         # x and flag as stored, no y
    assert nraw == 3 + 4 * 100 + 2 + 100


def test_malformed_keys_are_refused_with_a_pk_message(walk_exe, third_raw_pk):
    pk, mixed, _ = third_raw_pk
    o = keyraw.PK_HEADER
    cases = {
        "trailing": mixed + b"\x00",
        "cut_inside_raw_alpha": mixed[:o + 40],
        "cut_inside_raw_slice_element": mixed[:o + 3 * 64 + 4 + 64 + 32 + 5],
        "count_overruns": mixed[:o + 3 * 64] + (0x7FFFFFFF).to_bytes(4, "big") + mixed[o + 3 * 64 + 4:],
        "count_one_more": mixed[:o + 3 * 64] + (int.from_bytes(mixed[o + 3 * 64:o + 3 * 64 + 4], "big") + 1).to_bytes(4, "big") + mixed[o + 3 * 64 + 4:],
        "header_only": mixed[:o],
    }
    for tag, b in cases.items():
        out, sets = _dump(walk_exe, b, tag)
        assert out.returncode == 3 and out.stdout.startswith(("REFUSED pk: ", "REFUSED unexpected end of data")), (tag, out.stdout + out.stderr)
        if tag != "count_one_more":      # (a count off by one shifts everything behind it: whichever check meets the debris first refuses it)
            assert out.stdout.startswith("REFUSED pk: "), (tag, out.stdout)
    # one raw element less in G1.A than the wire flags announce: the consistency check counts points, not bytes
    na_at = o + 3 * 64
    na = int.from_bytes(mixed[na_at:na_at + 4], "big")
    secs = {name: elems for name, _, _, elems in keyraw.pk_sections(mixed)}
    last_o, last_sz = secs["g1.A"][-1]
    short = mixed[:na_at] + (na - 1).to_bytes(4, "big") + mixed[na_at + 4:last_o] + mixed[last_o + last_sz:]
    out, _ = _dump(walk_exe, short, "short")
    assert out.returncode == 3 and "pk: inconsistent slice sizes" in out.stdout, out.stdout + out.stderr
