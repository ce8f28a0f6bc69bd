// Host build of the tower test hook (csrc/debug_tower_ops.hpp): the element functions gsc_debug_tower_ops runs on the device, compiled
// by g++ with the HIP headers, so that the case tables and references of tests/devref.py are proven without a GPU
// (tests/test_debug_tower_host.py).  Path 1 runs on HostGroup, one group per element.  Two more paths exist here only, for the exact
// pairing reference: 2 = final_exp(miller<3>(P, Q)) of verify_dev.hpp, 3 = the same through lines_of, miller_few and the lane-sliced
// final exponentiation; their element is (xP, yP, xQ, yQ) = 54 words in, an Fp12 value = 108 words out.
//   stdin:  int32 path, op, n, then n elements of raw int32 words;  stdout: n elements of result words, then n flag bytes
#include "debug_tower_ops.hpp"
#include <cstdio>
#include <vector>

using namespace gsc::vfy;
namespace few = gsc::vfy::few;

int main() {
    int32_t hdr[3];
    if (fread(hdr, 4, 3, stdin) != 3) return 2;
    const int path = hdr[0], op = hdr[1];
    const size_t n = (size_t)hdr[2];
    const bool pairing = path == 2 || path == 3;
    if (!pairing && !dbg::tower_has(path, op)) return 3;
    const size_t iw = pairing ? 3 * dbg::kW2 : dbg::tower_in_words(op), ow = pairing ? dbg::kW12 : dbg::tower_out_words(path, op);
    std::vector<int32_t> in(iw * n), out(ow * n + 1);
    std::vector<uint8_t> flags(n + 1);
    if (fread(in.data(), 4, iw * n, stdin) != iw * n) return 2;
    std::vector<e2> slots(few::kSlots * few::kGroup);
    const few::HostGroup g{slots.data()};
    for (size_t i = 0; i < n; i++) {
        const int32_t* e = in.data() + iw * i;
        int32_t* o = out.data() + ow * i;
        if (path == 0) flags[i] = (uint8_t)dbg::tower_op(op, e, o);
        else if (path == 1) {
            bool flag;
            const few::HostGroup::V v = dbg::tower_group_op(g, op, e, flag);
            flags[i] = flag;
            if (ow) for (int k = 0; k < few::kGroup; k++) dbg::st2(o + dbg::kW2 * k, v.v[k]);
        } else {
            VP1 p; p.x = dbg::ld1(e); p.y = dbg::ld1(e + dbg::kW1); p.inf = 0;
            VP2 q; q.x = dbg::ld2(e + dbg::kW2); q.y = dbg::ld2(e + 2 * dbg::kW2); q.inf = 0;
            if (path == 2) {
                const VP1 none_p[3] = {VP1{F::zero(), F::zero(), 1}, VP1{F::zero(), F::zero(), 1}, VP1{F::zero(), F::zero(), 1}};
                const Line* none_l[3] = {nullptr, nullptr, nullptr}; const bool none_inf[3] = {true, true, true};
                dbg::st12(o, final_exp(miller<3>(p, q, true, none_p, none_l, none_inf)));
            } else {
                std::vector<Line> lv(kLineSteps);
                lines_of(q, lv.data());
                const few::Stream off = few::no_stream();
                const few::HostGroup::V v = few::final_exp(g, few::miller_few(g, few::stream(&p, lv.data(), false, false, true), off, off, off, 1));
                for (int k = 0; k < few::kSlices; k++) dbg::st2(o + dbg::kW2 * k, v.v[k]);
            }
        }
    }
    fwrite(out.data(), 4, ow * n, stdout);
    fwrite(flags.data(), 1, n, stdout);
    return 0;
}
