// The routing policy of the prover (csrc/chunk_route.hpp) on the CPU: a table of calls with the value of EVERY ChunkRoute field, written
// out by hand from the rules (the expressions prove_chunk used to derive between its launches), never by asking the
// function.  Built and run by tests/test_chunk_route_host.py; prints ROUTE-OK when every case holds.
#include "../../gnark-symmetric-crypto_amd/csrc/chunk_route.hpp"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace gsc;

namespace {
const char* const KW = "k_msm_win<Fp29f>";
const char* const KS = "k_wit_chain + k_wit_rows";
const char* const KL = "k_solver (one launch per level)";
const char* const KF = "k_solver_few";
const char* const KC = "k_solver_few + commitment MSM";

struct Want { bool latency, resident_wanted, small, resident, early_ab, early_b2, use_zfew, eval, z_digits_ready, overlap_q; const char* kernel; };
struct Case { const char* what; size_t n; EngineConfig cfg; RouteFacts f; RouteCall call; Want want; };

int check(const Case& c) {
    const ChunkRoute r = chunk_route(c.n, c.cfg, c.f, c.call);
    int bad = 0;
    auto flag = [&](const char* field, bool got, bool want) {
        if (got != want) { printf("FAIL %s (n = %zu): %s is %d, expected %d\n", c.what, c.n, field, (int)got, (int)want); bad++; }
    };
    flag("latency", r.latency, c.want.latency);
    flag("resident_wanted", r.resident_wanted, c.want.resident_wanted);
    flag("small", r.small, c.want.small);
    flag("resident", r.resident, c.want.resident);
    flag("early_ab", r.early_ab, c.want.early_ab);
    flag("early_b2", r.early_b2, c.want.early_b2);
    flag("use_zfew", r.use_zfew, c.want.use_zfew);
    flag("eval", r.eval, c.want.eval);
    flag("z_digits_ready", r.z_digits_ready, c.want.z_digits_ready);
    flag("overlap_q", r.overlap_q, c.want.overlap_q);
    if (strcmp(r.kernel_name, c.want.kernel)) { printf("FAIL %s (n = %zu): kernel_name is \"%s\", expected \"%s\"\n", c.what, c.n, r.kernel_name, c.want.kernel); bad++; }
    return bad;
}
}  // namespace

int main() {
    // ChaCha20-V3 as InitAlgorithm leaves it: few_max 32, a small-integer witness program, no commitment, every latency layout built
    EngineConfig cha; cha.few_max = 32;
    RouteFacts fcha; fcha.small_ok = true; fcha.quotient_eval = fcha.fuse_z_digits = fcha.zfew_flat = fcha.a_flat = fcha.b1_flat = fcha.b2_flat = true;
    // AES-V2: few_max 20, generic witness, one commitment
    EngineConfig aes; aes.few_max = 20;
    RouteFacts faes = fcha; faes.small_ok = false; faes.has_commitment = true;
    const RouteCall first;      // a first attempt: no debug vectors, both retries still allowed, no skip
    RouteCall no_small; no_small.allow_small = false;
    RouteCall no_resident; no_resident.allow_few_solver = false;
    RouteCall neither; neither.allow_small = neither.allow_few_solver = false;
    RouteCall skip; skip.skip_resident = true;
    RouteCall dbg; dbg.dbg = true;

    EngineConfig cha_nofew = cha; cha_nofew.few_path = 0;                    // few_solver stays 1
    EngineConfig aes_nofew = aes; aes_nofew.few_path = 0;
    EngineConfig cha_swf0 = cha; cha_swf0.small_witness_few = 0;
    EngineConfig cha_swf0_fs0 = cha_swf0; cha_swf0_fs0.few_solver = 0;
    EngineConfig cha_trace = cha; cha_trace.solver_trace = true;
    EngineConfig cha_qe0 = cha; cha_qe0.quotient_eval = 0;                   // (the route reads the FACT quotient_eval, not the wish)
    RouteFacts fcha_qe0 = fcha; fcha_qe0.quotient_eval = false;
    RouteFacts fcha_noz = fcha; fcha_noz.zfew_flat = false;
    RouteFacts fcha_noz_qe0 = fcha_noz; fcha_noz_qe0.quotient_eval = false;
    RouteFacts fcha_nofuse = fcha; fcha_nofuse.fuse_z_digits = false;
    EngineConfig cha_oq0 = cha; cha_oq0.overlap_quotient = 0;
    EngineConfig cha_oq2 = cha; cha_oq2.overlap_quotient = 2;
    RouteFacts fcha_noA = fcha; fcha_noA.a_flat = false;
    RouteFacts fcha_noB1 = fcha; fcha_noB1.b1_flat = false;
    RouteFacts fcha_noB2 = fcha; fcha_noB2.b2_flat = false;

    //                                                                    lat rw  sm  res eab eb2 zf  ev  zd  ov  kernel
    const std::vector<Case> cases = {
        // sizes around the two thresholds (few_max, one 64-column batch), ChaCha20 defaults
        {"chacha20 defaults", 1, cha, fcha, first,                        {1,  1,  1,  0,  1,  1,  1,  0,  0,  0,  KS}},
        {"chacha20 defaults", 32, cha, fcha, first,                       {1,  1,  1,  0,  1,  1,  1,  0,  0,  0,  KS}},
        {"chacha20 defaults", 33, cha, fcha, first,                       {0,  0,  1,  0,  0,  0,  0,  1,  1,  1,  KW}},
        {"chacha20 defaults", 64, cha, fcha, first,                       {0,  0,  1,  0,  0,  0,  0,  1,  1,  1,  KW}},
        {"chacha20 defaults", 65, cha, fcha, first,                       {0,  0,  1,  0,  0,  0,  0,  1,  1,  1,  KW}},
        // ... AES defaults: the resident solver with the commitment in the middle
        {"aes defaults", 1, aes, faes, first,                             {1,  1,  0,  1,  1,  1,  1,  0,  0,  0,  KC}},
        {"aes defaults", 20, aes, faes, first,                            {1,  1,  0,  1,  1,  1,  1,  0,  0,  0,  KC}},
        {"aes defaults", 21, aes, faes, first,                            {0,  0,  0,  0,  0,  0,  0,  1,  1,  1,  KW}},
        {"aes defaults", 32, aes, faes, first,                            {0,  0,  0,  0,  0,  0,  0,  1,  1,  1,  KW}},
        {"aes defaults", 33, aes, faes, first,                            {0,  0,  0,  0,  0,  0,  0,  1,  1,  1,  KW}},
        {"aes defaults", 64, aes, faes, first,                            {0,  0,  0,  0,  0,  0,  0,  1,  1,  1,  KW}},
        {"aes defaults", 65, aes, faes, first,                            {0,  0,  0,  0,  0,  0,  0,  1,  1,  1,  KW}},
        // few_path = 0 alone leaves the resident solver on: wanted either way, used where no small-integer program takes the witness
        {"few_path 0, few_solver 1 (chacha20)", 5, cha_nofew, fcha, first, {0,  1,  1,  0,  0,  0,  0,  1,  1,  1,  KW}},
        {"few_path 0, few_solver 1 (aes)", 5, aes_nofew, faes, first,     {0,  1,  0,  1,  0,  0,  0,  1,  1,  1,  KW}},
        {"few_path 0, few_solver 1 (aes)", 21, aes_nofew, faes, first,    {0,  0,  0,  0,  0,  0,  0,  1,  1,  1,  KW}},
        // the small-integer witness kept off the latency path
        {"small_witness_few 0", 5, cha_swf0, fcha, first,                 {1,  1,  0,  1,  1,  1,  1,  0,  0,  0,  KF}},
        {"small_witness_few 0", 40, cha_swf0, fcha, first,                {0,  0,  1,  0,  0,  0,  0,  1,  1,  1,  KW}},
        {"small_witness_few 0, few_solver 0", 5, cha_swf0_fs0, fcha, first, {1, 0,  0,  0,  1,  1,  1,  0,  0,  0,  KL}},
        // the solver trace stamps the generic kernels: no small path
        {"solver_trace", 5, cha_trace, fcha, first,                       {1,  1,  0,  1,  1,  1,  1,  0,  0,  0,  KF}},
        {"solver_trace", 100, cha_trace, fcha, first,                     {0,  0,  0,  0,  0,  0,  0,  1,  1,  1,  KW}},
        // the two retries, and both
        {"allow_small false", 5, cha, fcha, no_small,                     {1,  1,  0,  1,  1,  1,  1,  0,  0,  0,  KF}},
        {"allow_small false", 70, cha, fcha, no_small,                    {0,  0,  0,  0,  0,  0,  0,  1,  1,  1,  KW}},
        {"allow_few_solver false", 5, cha_swf0, fcha, no_resident,        {1,  1,  0,  0,  1,  1,  1,  0,  0,  0,  KL}},
        {"allow_few_solver false (aes)", 1, aes, faes, no_resident,       {1,  1,  0,  0,  1,  1,  1,  0,  0,  0,  KL}},
        {"allow_few_solver false, small still on", 5, cha, fcha, no_resident, {1, 1, 1,  0,  1,  1,  1,  0,  0,  0,  KS}},
        {"both retries taken", 5, cha, fcha, neither,                     {1,  1,  0,  0,  1,  1,  1,  0,  0,  0,  KL}},
        // the give-up penalty says skip
        {"skip (aes)", 1, aes, faes, skip,                                {1,  1,  0,  0,  1,  1,  1,  0,  0,  0,  KL}},
        {"skip, small witness", 5, cha, fcha, skip,                       {1,  1,  1,  0,  1,  1,  1,  0,  0,  0,  KS}},
        // the latency layout of the quotient bases present / absent, the quotient form 1 / 0: a latency call and a batch call
        {"zfew, quotient_eval 0", 5, cha_qe0, fcha_qe0, first,            {1,  1,  1,  0,  1,  1,  1,  0,  0,  0,  KS}},
        {"no zfew, quotient_eval 1", 5, cha, fcha_noz, first,             {1,  1,  1,  0,  1,  1,  0,  1,  0,  0,  KS}},
        {"no zfew, quotient_eval 0", 5, cha_qe0, fcha_noz_qe0, first,     {1,  1,  1,  0,  1,  1,  0,  0,  0,  0,  KS}},
        {"zfew, quotient_eval 1", 100, cha, fcha, first,                  {0,  0,  1,  0,  0,  0,  0,  1,  1,  1,  KW}},
        {"zfew, quotient_eval 0", 100, cha_qe0, fcha_qe0, first,          {0,  0,  1,  0,  0,  0,  0,  0,  0,  0,  KW}},
        {"no zfew, quotient_eval 1", 100, cha, fcha_noz, first,           {0,  0,  1,  0,  0,  0,  0,  1,  1,  1,  KW}},
        {"no zfew, quotient_eval 0", 100, cha_qe0, fcha_noz_qe0, first,   {0,  0,  1,  0,  0,  0,  0,  0,  0,  0,  KW}},
        // the last quotient kernel does not write the digits: nothing to run beside
        {"fuse_z_digits 0", 100, cha, fcha_nofuse, first,                 {0,  0,  1,  0,  0,  0,  0,  1,  0,  0,  KW}},
        {"fuse_z_digits 0", 5, cha, fcha_nofuse, first,                   {1,  1,  1,  0,  1,  1,  1,  0,  0,  0,  KS}},
        // the quotient beside the wire sets: below 4096 columns (4032 statements: B = 4032; 4033: B = 4096), always, never
        {"overlap_quotient 0", 4032, cha_oq0, fcha, first,                {0,  0,  1,  0,  0,  0,  0,  1,  1,  0,  KW}},
        {"overlap_quotient 0", 4033, cha_oq0, fcha, first,                {0,  0,  1,  0,  0,  0,  0,  1,  1,  0,  KW}},
        {"overlap_quotient 1", 4032, cha, fcha, first,                    {0,  0,  1,  0,  0,  0,  0,  1,  1,  1,  KW}},
        {"overlap_quotient 1", 4033, cha, fcha, first,                    {0,  0,  1,  0,  0,  0,  0,  1,  1,  0,  KW}},
        {"overlap_quotient 1", 4096, cha, fcha, first,                    {0,  0,  1,  0,  0,  0,  0,  1,  1,  0,  KW}},
        {"overlap_quotient 2", 4032, cha_oq2, fcha, first,                {0,  0,  1,  0,  0,  0,  0,  1,  1,  1,  KW}},
        {"overlap_quotient 2", 4096, cha_oq2, fcha, first,                {0,  0,  1,  0,  0,  0,  0,  1,  1,  1,  KW}},
        // debug vectors are fetched between the stages: one stream
        {"dbg", 100, cha, fcha, dbg,                                      {0,  0,  1,  0,  0,  0,  0,  1,  1,  0,  KW}},
        {"dbg, overlap_quotient 2", 100, cha_oq2, fcha, dbg,              {0,  0,  1,  0,  0,  0,  0,  1,  1,  0,  KW}},
        {"dbg", 1, cha, fcha, dbg,                                        {1,  1,  1,  0,  1,  1,  1,  0,  0,  0,  KS}},
        // a wire set whose windowed part has no latency layout (GSC_FEW_WIDE=0): its sum stays on the main stream
        {"A without a latency layout", 5, cha, fcha_noA, first,           {1,  1,  1,  0,  0,  0,  1,  0,  0,  0,  KS}},
        {"B1 without a latency layout", 5, cha, fcha_noB1, first,         {1,  1,  1,  0,  0,  0,  1,  0,  0,  0,  KS}},
        {"B2 without a latency layout", 5, cha, fcha_noB2, first,         {1,  1,  1,  0,  1,  0,  1,  0,  0,  0,  KS}},
        {"A without a latency layout, batch call", 100, cha, fcha_noA, first, {0, 0, 1,  0,  0,  0,  0,  1,  1,  1,  KW}},
    };
    int bad = 0;
    for (const Case& c : cases) bad += check(c);
    if (bad) { printf("ROUTE-FAILED: %d fields\n", bad); return 1; }
    printf("ROUTE-OK %zu cases\n", cases.size());
    return 0;
}
