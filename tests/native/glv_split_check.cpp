// Host build of the scalar split behind the latency path's scalar multiplications (csrc/glv.hpp, glv_split), as stage_upload calls it.
// tests/test_assemble_model_host.py holds the Python model of the split and the case table of tests/test_gpu_assemble.py against it.
//   stdin : n (int32 LE) | n canonical scalars, 8 x u32 LE each
//   stdout: n records of 48 bytes: k1[5], k2[5], neg (u32 LE) | u32: what glv_split returned
#include "glv.hpp"
#include <cstdio>
#include <cstring>
#include <vector>

int main() {
    int32_t n;
    if (fread(&n, 4, 1, stdin) != 1 || n < 0) return 2;
    std::vector<uint32_t> scalars(8 * (size_t)n), out(12 * (size_t)n);
    if (fread(scalars.data(), 32, (size_t)n, stdin) != (size_t)n) return 2;
    for (size_t i = 0; i < (size_t)n; i++) {
        gsc::GlvSplit s;
        memset(&s, 0, sizeof s);
        const bool ok = gsc::glv_split(&scalars[8 * i], s);
        memcpy(&out[12 * i], s.k1, 20); memcpy(&out[12 * i + 5], s.k2, 20);
        out[12 * i + 10] = s.neg; out[12 * i + 11] = ok ? 1u : 0u;
    }
    return fwrite(out.data(), 48, (size_t)n, stdout) == (size_t)n ? 0 : 2;
}
