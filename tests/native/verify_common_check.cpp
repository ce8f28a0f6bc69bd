// Host check of verify_common (the rules libverify.so and the GPU verifier share), driven by tests/test_verify_gpu_host.py.
//   stdin lines: "W <algorithm> <signals hex>"          -> the 144 window bytes (hex)
//                "S <commitment 0/1> <length> <slot hex>" -> 1 if the proof passes the host pre-check, else 0
//                "B <algorithm> <window>"              -> "<first K index> <shift>"
#include "verify_common.hpp"
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

static std::vector<uint8_t> unhex(const std::string& h) { std::vector<uint8_t> v; for (size_t i = 0; i + 1 < h.size(); i += 2) v.push_back((uint8_t)std::stoi(h.substr(i, 2), nullptr, 16)); return v; }

int main() {
    std::string op;
    while (std::cin >> op) {
        if (op == "W") {
            int algo; std::string h; std::cin >> algo >> h;
            const auto sig = unhex(h); uint8_t win[gsc::verify::kWindows];
            gsc::verify::public_windows(algo, sig.data(), win);
            for (uint8_t b : win) printf("%02x", b);
            printf("\n");
        } else if (op == "S") {
            int hc; size_t len; std::string h; std::cin >> hc >> len >> h;
            auto slot = unhex(h); slot.resize(196);
            printf("%d\n", (int)(len <= 196 && gsc::verify::proof_shape_ok(slot.data(), len, hc != 0)));
        } else if (op == "B") {
            int algo; size_t j; std::cin >> algo >> j;
            uint32_t f, s; gsc::verify::window_base(algo, j, f, s);
            printf("%u %u\n", f, s);
        }
        fflush(stdout);
    }
    return 0;
}
