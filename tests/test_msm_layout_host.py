"""The host-side geometry of the MSM kernels, built for the host (tests/native/msm_geometry_check.cpp): xcd_slice and slice_bounds
(csrc/msm_dev.hpp), msm_slices, the row segments, the layout planner that build_set and gsc_debug_msm share and msm_geometry, the slices and
scratch of a call that msm_run, alloc_lane and gsc_debug_msm share (csrc/msm_layout.hpp), the reduction levels (csrc/kernels.hpp).  The self-check
also runs once under ASan + UBSan as a stand-alone program; the planner is held against a Python statement of the same rules (devref.FlatPlan,
devref.sort_bases) on hand-built classes, msm_geometry against the one below."""
import os
import struct
import subprocess

import pytest

import devref as D
from conftest import ROOT

BUILD = os.path.join(ROOT, "build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-static-libasan", "-static-libubsan"]
EXPAND_MAX, EXPAND_C, NARROW_MAX_BITS = 64, 15, 14      # csrc/engine_impl.hpp


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def geometry_exe(request):
    exe = os.path.join(BUILD, "msm_geometry_check_" + request.param)
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", D.CSRC] +
                          (SAN if request.param != "plain" else []) + ["-o", exe, os.path.join(ROOT, "tests", "native", "msm_geometry_check.cpp")])
    return exe


def test_slice_geometry_and_reduction_levels(geometry_exe):
    out = subprocess.run([geometry_exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout == "ok\n", out.stdout + out.stderr


def _classes():
    """(name, status, rows, cls, uniform, bit_groups, margin, expand_cv): 0, 7, 8 and 9 bits; narrow lengths; 0, 1 and 65 wide wires either side of
    EXPAND_MAX; points at infinity dropped"""
    out = []
    def add(name, cls_of_base, status=None, uniform=0, bit_groups=1, margin=1, expand_cv=0, rows=None):
        n = len(cls_of_base)
        rows = rows if rows is not None else [3 * i + 1 for i in range(n)]
        cls = [255] * (max(rows) + 2 if rows else 2)
        for r, c in zip(rows, cls_of_base):
            if r < len(cls):
                cls[r] = c
        out.append((name, status or [0] * n, rows, cls, uniform, bit_groups, margin, expand_cv))
    add("empty", [])
    for nbits in (0, 7, 8, 9):
        add("bits%d_narrow_wide1" % nbits, [0, 1][:nbits % 2] + [1, 0] * (nbits // 2) + [2, 8, 13, 14, 3] + [255])
        add("bits%d_only" % nbits, [1] * nbits)
    add("narrow_lengths", [2, 3, 7, 12, 13, 14, 15, 200], margin=0)             # 15 and 200 are wide: beyond NARROW_MAX_BITS
    add("narrow_margin2", [2, 12, 13], margin=2)                                  # 13 + 2 > 14: wide
    add("wide64_expanded", [0] * 8 + [255] * 64)                                  # at EXPAND_MAX: window octets at EXPAND_C
    add("wide65_windowed", [0] * 8 + [255] * 65)                                  # beyond: the windowed kernel
    add("wide1", [255])
    add("infinity_dropped", [0, 1, 0, 0, 1, 0, 0, 0, 0, 5, 255], status=[0, 2, 0, 0, 0, 2, 0, 0, 0, 0, 2])
    add("no_bit_groups", [0, 1, 5, 255], bit_groups=0)                            # everything wide
    add("row_beyond_classes", [0, 0, 5], rows=[1, 900, 2])                        # a row the classes do not cover is wide
    add("uniform", [0, 1, 5, 255] * 5, uniform=1)                                 # Z: no flat part
    add("uniform_expand8", [0, 1, 5, 255] * 5, uniform=1, expand_cv=8)            # the latency layout of the quotient bases: every base as octets
    add("expand_cv4", [0] * 9 + [255] * 3, expand_cv=4)                           # the narrowest digits: the most octets per wire
    return out


@pytest.mark.parametrize("case", _classes(), ids=lambda c: c[0])
def test_planner_matches_the_python_statement(geometry_exe, case):
    name, status, rows, cls, uniform, bit_groups, margin, expand_cv = case
    n, zero_row = len(status), 77777
    payload = struct.pack("<10i", n, uniform, bit_groups, margin, NARROW_MAX_BITS, expand_cv, EXPAND_MAX, EXPAND_C, zero_row, len(cls))
    payload += bytes(status) + struct.pack("<%dI" % n, *rows) + bytes(cls)
    out = subprocess.run([geometry_exe, "layout"], input=payload, capture_output=True, timeout=60, check=True).stdout
    nbit, nexp, cv, nflat, noct, nwide, nsegs = struct.unpack("<7I", out[:28])
    at = [28]
    def take(fmt, k):
        v = struct.unpack_from("<%d%s" % (k, fmt), out, at[0]); at[0] += k * struct.calcsize(fmt)
        return list(v)
    src, shift, frows, length = take("I", nflat), take("I", nflat), take("I", nflat), take("I", nflat)
    octwin, wide, off = take("i", noct), take("I", nwide), take("Q", nflat)
    entries, = take("Q", 1)
    assert at[0] == len(out)
    plan = D.FlatPlan(*D.sort_bases(status, rows, cls, bool(uniform), bit_groups, margin, NARROW_MAX_BITS), rows, zero_row, bool(uniform), expand_cv, EXPAND_MAX, EXPAND_C)
    assert (nbit, nexp, cv, nflat) == (plan.nbit, plan.nexpanded, plan.cv, plan.nflat)
    assert (src, shift, frows, length, octwin, wide) == (plan.src, plan.shift, plan.frows, plan.len, plan.octwin, plan.wide)
    # what every layout must satisfy whatever the rules: whole octets, whole bit groups, every finite base exactly once outside the padding
    assert nflat % 8 == 0 and nbit % 8 == 0 and noct == nflat // 8
    assert off == [sum(length[:i]) for i in range(nflat)] and entries == sum(length) and nsegs == sum((l + 255) // 256 for l in length)
    finite = [i for i in range(n) if status[i] != 2]
    plain = [s for s, r, o in zip(src, frows, range(nflat)) if r != zero_row and octwin[o // 8] < 0]
    assert sorted(plain + sorted(set(s for s, o in zip(src, range(nflat)) if octwin[o // 8] >= 0)) + wide) == finite


def test_the_hand_built_classes_cover_the_rules():
    plans = {c[0]: D.FlatPlan(*D.sort_bases(c[1], c[2], c[3], bool(c[4]), c[5], c[6], NARROW_MAX_BITS), c[2], 77777, bool(c[4]), c[7], EXPAND_MAX, EXPAND_C) for c in _classes()}
    assert plans["bits7_only"].nbit == 0 and plans["bits7_only"].len[:7] == [2] * 7 and plans["bits7_only"].frows[7] == 77777      # demoted, padded
    assert plans["bits9_only"].nbit == 8 and plans["bits9_only"].len[8] == 2
    assert plans["wide64_expanded"].nexpanded == 64 and plans["wide64_expanded"].cv == 15 and not plans["wide64_expanded"].wide
    assert plans["wide65_windowed"].nexpanded == 0 and len(plans["wide65_windowed"].wide) == 65
    assert plans["uniform"].nflat == 0 and len(plans["uniform"].wide) == 20
    assert plans["uniform_expand8"].nflat == 20 * 32 and plans["uniform_expand8"].octwin[:5] == [0, 8, 16, 24, 0]
    octs = (D.msm_windows(4) + 7) // 8
    assert plans["expand_cv4"].octwin[2:2 + octs + 1] == list(range(0, 8 * octs, 8)) + [0] and plans["expand_cv4"].nflat == 16 + 3 * 8 * octs
    w64 = plans["wide64_expanded"]      # 17 windows of 15 bits in three octets: seven padding slots of shift 0 and length 1
    assert w64.len[8:32] == [1 << 14] * 17 + [1] * 7 and w64.shift[8:32] == [15 * q for q in range(17)] + [0] * 7 and w64.octwin[1:5] == [0, 8, 16, 0]
    assert len(plans["infinity_dropped"].src) == 8 and plans["infinity_dropped"].nbit == 0
    assert plans["narrow_lengths"].len[:6] == [4, 8, 128, 4096, 8192, 16384] and plans["narrow_lengths"].nexpanded == 2


# ---- msm_geometry: the slices of a call and the scratch it can write ----
MSM_REDUCE_FANIN = 32
_ceil = lambda a, b: -(-a // b)


def _slices(nbases, nwin, most, B):
    """msm_slices: slices of up to `most` bases, shorter ones while that leaves fewer than ~8k waves; whole octets, no empty slice"""
    gw = (B // 64) * nwin
    n = (max(_ceil(nbases, most), _ceil(8192, gw)) + 7) & ~7
    per = ((_ceil(nbases, n) + 7) & ~7) or 8
    return _ceil(nbases, per) or 1, per


def _geometry(shape, B, latency, win_slice=256, per_flat=0, per_win=0):
    """the rules, stated once more: (flat_slices, flat_per, win_slices, win_per, few_wide_slices, pa, pb, sj, digit_words, gok_bytes)"""
    nflat, nbit, nwide, c, nwin, digit_bases, few_wide_nflat = shape
    few = lambda n: _ceil(_ceil(n, 8), 64)
    fs = fp = ws = wp = fws = 0
    if nflat and latency:
        fs, fp = few(nflat), 512
    elif nflat and per_flat:
        fs, fp = _ceil(nflat, per_flat), per_flat
    elif nflat:
        fs, fp = _slices(nflat, 1, 256, B)
    if latency and few_wide_nflat:      # side by side in the same partial buffer
        fws, fp = few(few_wide_nflat), 512
        fs += fws
    if nwide and per_win:
        ws, wp = _ceil(nwide, per_win), per_win
    elif nwide:
        ws, wp = _slices(nwide, nwin, win_slice, B)
        if latency and ws > _ceil(nwide, 512):
            ws, wp = _ceil(nwide, 512), 512
    sj = B * nwin if nwide else 0
    pa = max(fs * B, ws * B * nwin)
    pb = max(_ceil(fs, MSM_REDUCE_FANIN) * B, _ceil(ws, MSM_REDUCE_FANIN) * B * nwin)
    digits = max(nflat // 8 * B, _ceil(few_wide_nflat, 8) * 64 if latency else 0,
                 nwin * _ceil(digit_bases or nwide, 8) * B * (2 if c > 16 else 1) if nwide else 0)
    gok = max(nbit // 8 * (B // 64), nbit // 8 * D.MSM_FEW_PROOFS) if nflat else 0
    return fs, fp, ws, wp, fws, pa, pb, sj, digits, gok


def _shapes():
    """name -> (nflat, nbit, nwide, c, nwin, digit_bases, few_wide_nflat).  The first five are ChaCha20-V3's sets as gsc_describe names them
    (profiles/r18_ab_default.txt): grouped bits, an octet of narrow rows and padding, one wide wire expanded into the 24 slots of its 17 windows
    at EXPAND_C = 15; Z folded; C with a windowed part"""
    w = D.msm_windows
    expanded = 8 * _ceil(w(EXPAND_C), 8)
    return {
        "chacha_A": (22000 + 8 + expanded, 22000, 0, 16, w(16), 0, 0),
        "chacha_B": (12528 + 8 + expanded, 12528, 0, 16, w(16), 0, 0),
        "chacha_K": (22128 + 8 + expanded, 22128, 0, 16, w(16), 0, 0),
        "chacha_Z": (0, 0, 23616, 17, w(17), 32768, 0),                 # 23616 live of 32768 digit bases, two words per digit octet
        "chacha_C": (23280 + 8, 23280, 336, 16, w(16), 0, 0),
        "flat_only": (520, 16, 0, 6, w(6), 0, 0),
        "flat_one_octet": (8, 0, 0, 16, w(16), 0, 0),
        "windowed_only": (0, 0, 1000, 16, w(16), 0, 0),
        "windowed_c17": (0, 0, 129, 17, w(17), 0, 0),
        "both": (72, 8, 65, 8, w(8), 0, 0),
        "digit_bases": (0, 0, 19, 6, w(6), 40, 0),
        "few_wide": (23288, 23280, 336, 16, w(16), 0, 336 * 8 * _ceil(w(8), 8)),      # the windowed part once more as (base, window) rows of 8-bit digits
        "few_wide_alone": (0, 0, 70, 16, w(16), 0, 70 * 8 * _ceil(w(8), 8)),
        "empty": (0, 0, 0, 16, w(16), 0, 0),
    }


def _calls():
    out = []
    for name, shape in _shapes().items():
        for B in (64, 128, 1024, 8192):
            out.append((name, shape, B, 0, 256, 0, 0))
        out.append((name, shape, 64, 1, 256, 0, 0))
        out.append((name, shape, 128, 0, 64, 0, 0))                    # GSC_WIN_SLICE
        out.append((name, shape, 64, 0, 256, 8, 0)); out.append((name, shape, 64, 0, 256, 0, 64)); out.append((name, shape, 128, 0, 256, 512, 8))      # the overrides
        out.append((name, shape, 64, 1, 256, 8, 64))                   # a latency call reads per_win, not per_flat
    return out


def test_geometry_matches_the_python_statement(geometry_exe):
    calls = _calls()
    text = "".join("%d %d %d %d %d %d %d %d %d %d %d %d\n" % (shape + (B, lat, ws, pf, pw)) for _, shape, B, lat, ws, pf, pw in calls)
    out = subprocess.run([geometry_exe, "geometry"], input=text, capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert len(out) == len(calls)
    for (name, shape, B, lat, ws, pf, pw), line in zip(calls, out):
        got = tuple(int(x) for x in line.split())
        assert got == _geometry(shape, B, bool(lat), ws, pf, pw), (name, B, lat, ws, pf, pw)
        # whatever the rules: whole octets per slice, the slices cover the bases, a flat slice holds at most 512, the first reduction level fits pb
        nflat, nbit, nwide, c, nwin = shape[:5]
        fs, fp, wsl, wp, fws, pa, pb, sj = got[:8]
        assert fp % 8 == 0 and fp <= 512 and wp % 8 == 0 and (fs - fws) * fp >= nflat and wsl * wp >= nwide and fws * 512 >= (shape[6] if lat else 0)
        assert bool(fs - fws) == bool(nflat) and bool(wsl) == bool(nwide)
        assert pa >= fs * B and pa >= wsl * sj and pb >= _ceil(fs, 32) * B and pb >= _ceil(wsl, 32) * sj


def test_the_lanes_scratch_is_the_batch_calls_and_the_latency_call_at_64():
    """alloc_lane's rule, on the Python statement: a latency call never needs more partial sums, window sums or verdicts than the batch call of 64
    columns over the same set, and more digit words only for a latency layout of the windowed part"""
    for name, shape in _shapes().items():
        batch, lat = _geometry(shape, 64, False), _geometry(shape, 64, True)
        if not shape[6]:
            assert all(l <= b for l, b in zip(lat[5:], batch[5:])), name
        assert lat[7] == batch[7] and lat[9] == batch[9], name
