// Host harness of tests/test_solver_model_host.py (plain g++ against csrc/formats.cpp and csrc/wit_small.cpp, no device):
//   solver_desc_dump dump  <r1cs file> <out>     the description gsc_debug_solve takes (include/libprove.h), from gnark's R1CS file
//   solver_desc_dump build <description> <out>   build_solver_program, build_few_program and build_small_program on a description: the three
//                                                program layouts, for the test's integer replay; "REFUSED: <text>" and exit code 3 when a builder throws
// Files are streams of little-endian u32: scalars, then vectors as [count, values ...].
#include "formats.hpp"
#include "wit_small.hpp"
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

using namespace gsc;

namespace {
std::vector<uint32_t> read_words(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    std::vector<uint32_t> w; uint32_t buf[4096]; size_t n;
    while ((n = fread(buf, 4, 4096, f)) > 0) w.insert(w.end(), buf, buf + n);
    fclose(f);
    return w;
}
std::vector<uint8_t> read_bytes(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    std::vector<uint8_t> w; uint8_t buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) w.insert(w.end(), buf, buf + n);
    fclose(f);
    return w;
}
struct Out {
    std::vector<uint32_t> w;
    void u(uint64_t v) { w.push_back((uint32_t)v); }
    template <class V> void vec(const V& v) { u(v.size()); for (auto x : v) w.push_back((uint32_t)x); }
    void vec64(const std::vector<int64_t>& v) { u(v.size()); for (int64_t x : v) { w.push_back((uint32_t)(uint64_t)x); w.push_back((uint32_t)((uint64_t)x >> 32)); } }
    void save(const char* path) const { FILE* f = fopen(path, "wb"); if (!f || fwrite(w.data(), 4, w.size(), f) != w.size()) throw std::runtime_error("cannot write the output"); fclose(f); }
};
struct In {
    const std::vector<uint32_t>& w; size_t i = 0;
    uint32_t u() { if (i >= w.size()) throw std::runtime_error("description: truncated"); return w[i++]; }
    std::vector<uint32_t> vec() { const uint32_t n = u(); if (n > w.size() - i) throw std::runtime_error("description: truncated vector"); std::vector<uint32_t> v(w.begin() + i, w.begin() + i + n); i += n; return v; }
};

void put_desc(Out& o, const R1csFile& cs) {
    o.u(cs.n_public); o.u(cs.n_secret); o.u(cs.n_internal); o.u(cs.n_constraints); o.u(cs.has_commitment ? 1 : 0); o.u(cs.commit_wire);
    o.vec(cs.calldata); o.vec(cs.blueprint); o.vec(cs.constraint_off); o.vec(cs.wire_off);
    std::vector<uint32_t> kinds, lens, flat;
    for (size_t b = 0; b < cs.bp_kind.size(); b++) { kinds.push_back(cs.bp_kind[b]); lens.push_back((uint32_t)cs.bp_entries[b].size()); flat.insert(flat.end(), cs.bp_entries[b].begin(), cs.bp_entries[b].end()); }
    o.vec(kinds); o.vec(lens); o.vec(flat); o.vec(cs.coeff_limbs); o.vec(cs.commit_private);
}
R1csFile get_desc(In& in) {
    R1csFile cs;
    cs.n_public = in.u(); cs.n_secret = in.u(); cs.n_internal = in.u(); cs.n_constraints = in.u(); cs.has_commitment = in.u() != 0; cs.commit_wire = in.u();
    cs.calldata = in.vec(); cs.blueprint = in.vec(); cs.constraint_off = in.vec(); cs.wire_off = in.vec();
    for (size_t q = 0; q < cs.calldata.size();) {      // as parse_r1cs derives the boundaries
        const uint32_t l = cs.calldata[q];
        if (l == 0 || q + l > cs.calldata.size()) throw std::runtime_error("r1cs: corrupt instruction length");
        cs.instr_start.push_back(q); q += l;
    }
    cs.instr_start.push_back(cs.calldata.size());
    if (cs.instr_start.size() - 1 != cs.blueprint.size() || cs.constraint_off.size() != cs.blueprint.size() || cs.wire_off.size() != cs.blueprint.size()) throw std::runtime_error("r1cs: instruction table size mismatch");
    const std::vector<uint32_t> kinds = in.vec(), lens = in.vec(), flat = in.vec();
    size_t at = 0;
    for (size_t b = 0; b < kinds.size(); b++) {
        if (kinds[b] > BP_LOOKUP || b >= lens.size() || lens[b] > flat.size() - at) throw std::runtime_error("description: blueprints");
        cs.bp_kind.push_back((BlueprintKind)kinds[b]); cs.bp_entries.emplace_back(flat.begin() + at, flat.begin() + at + lens[b]); at += lens[b];
    }
    for (uint32_t b : cs.blueprint) if (b >= cs.bp_kind.size()) throw std::runtime_error("r1cs: blueprint id out of range");
    cs.coeff_limbs = in.vec(); cs.commit_private = in.vec();
    return cs;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: solver_desc_dump dump|build <in> <out>\n"); return 2; }
    try {
        Out o;
        if (!strcmp(argv[1], "dump")) {
            const std::vector<uint8_t> file = read_bytes(argv[2]);
            put_desc(o, parse_r1cs(file.data(), file.size()));
            o.save(argv[3]);
            return 0;
        }
        const std::vector<uint32_t> words = read_words(argv[2]);
        In in{words};
        const R1csFile cs = get_desc(in);
        const std::vector<uint32_t> cw = in.vec(), ca = in.vec(), cb = in.vec(), cc = in.vec(), ok = in.vec(), lo = in.vec(), hi = in.vec();
        const SolverProgram sp = build_solver_program(cs);
        o.u(sp.n_levels); o.u(sp.commit_level); o.u(sp.n_ops); o.u(sp.n_inversions); o.u(sp.n_tables);
        o.vec(sp.words); o.vec(sp.lookup_coeff); o.vec(sp.sched); o.vec(sp.level_kind); o.vec(sp.level_long); o.vec(sp.count_ops);
        const FewProgram fp = build_few_program(sp);
        o.vec(fp.ops); o.vec(fp.terms); o.vec(fp.level_start); o.vec(fp.count_ops); o.vec(fp.count_qoff); o.vec(fp.count_first);
        std::vector<int64_t> coef(lo.size()); std::vector<uint8_t> coef_ok(ok.begin(), ok.end());
        for (size_t i = 0; i < lo.size() && i < hi.size(); i++) coef[i] = (int64_t)(((uint64_t)hi[i] << 32) | lo[i]);
        auto bytes = [](const std::vector<uint32_t>& v) { return std::vector<uint8_t>(v.begin(), v.end()); };
        const SmallProgram P = build_small_program(sp, cs.n_wires(), cs.n_constraints, coef, coef_ok, bytes(cw), bytes(ca), bytes(cb), bytes(cc));
        o.u(P.ok ? 1 : 0); o.u(P.rows_per_group); o.u(P.scratch_row); o.u(P.n_levels); o.u(P.max_slots); o.u(P.n_rtiny); o.u(P.n_rgen);
        o.vec(P.levels); o.vec(P.tiny); o.vec(P.parts); o.vec(P.bits); o.vec(P.twire); o.vec64(P.tcoef);
        o.vec(P.rtiny); o.vec(P.rgen); o.vec(P.rtwire); o.vec64(P.rtcoef); o.vec(P.cls_a); o.vec(P.cls_b); o.vec(P.cls_c);
        o.save(argv[3]);
        printf("BUILT levels=%zu ops=%zu small=%d %s\n", sp.n_levels, sp.n_ops, P.ok ? 1 : 0, P.why.c_str());
        return 0;
    } catch (const std::exception& e) {
        printf("REFUSED: %s\n", e.what());
        return 3;
    }
}
