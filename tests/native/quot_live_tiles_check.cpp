// Host-only: prints kernels.hpp quot_live_tiles(L, live) for the pairs "L live" on the command line, one value per line (tests/test_quot_live_tiles_host.py
// compares them with the tiles that the table order itself says hold the positions 0 .. live-1).
#include "../../gnark-symmetric-crypto_amd/csrc/kernels.hpp"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
    if (argc < 3 || argc % 2 != 1) return 2;
    for (int i = 1; i + 1 < argc; i += 2) printf("%u\n", gsc::quot_live_tiles(atoi(argv[i]), (size_t)strtoull(argv[i + 1], nullptr, 10)));
    return 0;
}
