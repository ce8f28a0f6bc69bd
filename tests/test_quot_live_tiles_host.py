"""Host-only check (no GPU) of the fact the quotient's live-tile launch rests on (k_ntt.hip launch_quotient, kernels.hpp quot_live_tiles).

Workgroup g of the last quotient kernel reads, couples and writes the coset indices whose low Llo bits are g, and nothing else.  The Z set's
table order (quot_digit_index; Python twin: quot_fold_model.table_order, pinned to the C++ by test_quot_index.py) is tile-major in those
workgroups, so the positions 0 .. live-1 that the fold keeps need exactly the first ceil(live / G) of them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from quot_fold_model import table_order

LS = range(4, 18)
CIRCUITS = {"chacha20": (15, 23616, 93), "aes128": (17, 74898, 147), "aes256": (17, 99434, 195)}      # L, live = constraints - 1, tiles


def _shape(L):
    Lhi = (L + 1) // 2
    return 1 << L, 1 << Lhi, L - Lhi      # n, G (positions per tile), Llo (the tile is the index's low Llo bits)


def live_tiles(L, live):
    """quot_live_tiles of kernels.hpp; 0 stands for every position"""
    n, G, Llo = _shape(L)
    return min(max(-(-live // G), 1), 1 << Llo) if live else 1 << Llo


def _lives(L):
    n, G, _ = _shape(L)
    return sorted({1, G - 1, G, G + 1, n - G, n - 1, n} - {0})


@pytest.fixture(scope="module")
def tile_of_position():
    """per L: the workgroup of the last quotient kernel that holds table position t"""
    out = {}
    for L in LS:
        n, G, Llo = _shape(L)
        order = np.array(table_order(n), dtype=np.int64)
        assert np.array_equal(np.sort(order), np.arange(n))
        out[L] = order & ((1 << Llo) - 1)
    return out


@pytest.mark.parametrize("L", LS)
def test_table_positions_of_a_tile_are_the_indices_with_its_low_bits(tile_of_position, L):
    n, G, Llo = _shape(L)
    tiles = tile_of_position[L].reshape(1 << Llo, G)      # row g: positions [g G, (g + 1) G)
    assert np.array_equal(tiles, np.repeat(np.arange(1 << Llo)[:, None], G, axis=1))
    # ... and a permutation with G positions per tile leaves no index of those low bits elsewhere


@pytest.mark.parametrize("L", LS)
def test_ceil_live_over_g_tiles_hold_the_live_positions_and_no_fewer_do(tile_of_position, L):
    for live in _lives(L):
        needed = np.unique(tile_of_position[L][:live])
        assert np.array_equal(needed, np.arange(live_tiles(L, live))), (L, live)


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_the_three_circuits(tile_of_position, name):
    L, live, want = CIRCUITS[name]
    assert live_tiles(L, live) == want
    assert np.array_equal(np.unique(tile_of_position[L][:live]), np.arange(want))
    assert np.all(tile_of_position[L][live:] >= want - 1)      # the dropped positions: the rest of the last live tile, then dead tiles only


def test_the_launcher_counts_the_same_tiles(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "quot_live_tiles_check")
    subprocess.check_call([hipcc, "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "native", "quot_live_tiles_check.cpp")])
    pairs = [(L, live) for L in LS for live in [0] + _lives(L) + [(1 << L) + 1, 3 << L]] + [(L, live) for L, live, _ in CIRCUITS.values()]
    out = subprocess.run([exe] + [str(v) for p in pairs for v in p], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert [int(x) for x in out.stdout.split()] == [live_tiles(L, live) for L, live in pairs]
