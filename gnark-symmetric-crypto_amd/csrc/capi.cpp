// C-ABI of libprove (see include/libprove.h) and the JSON host logic behind it.
//
// Mirrors, symbol for symbol, the reference's cgo exports (libraries/prover/libprove.go:17-47) and the
// dispatch / JSON layer they call (libraries/prover/impl/prove_impl.go:65-143, provers.go:53-59, :79-89, :172-182):
// algorithm registry, idempotent InitAlgorithm, Go-encoding/json-compatible input decoding, the
// {"proof":{"proofJson"},"publicSignals"} output, and "panic -> JSON" error reporting.
#include "../../include/libprove.h"
#include "engine.hpp"
#include "dispatch.hpp"
#include "formats.hpp"
#include "registry.hpp"
#include "glv.hpp"
#include "host_ciphers.hpp"
#include "json.hpp"
#include "setup.hpp"
#include "phase2_gpu.hpp"
#include "sigma_gpu.hpp"
#include "srs_gpu.hpp"
#include "srs_contrib.hpp"
#include "srs_contrib_gpu.hpp"
#include "msm_debug.hpp"
#include "solver_debug.hpp"
#include "assemble_debug.hpp"
#include <sys/random.h>
#include <cerrno>
#include <condition_variable>
#include <deque>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

using namespace gsc;

namespace {

const char* kAlgorithmNames[3] = {"chacha20", "aes-128-ctr", "aes-256-ctr"};   // prove_impl.go:21-25

// The algorithms (registry.hpp): an engine and the micro-batcher in front of it per id.  Every entry point takes ONE snapshot
// when it enters and is served by it until it returns, whatever gsc_release_algorithm / gsc_replace_algorithm do meanwhile.
using ServedAlgo = Served<Algorithm>;
using Snapshot = Registry<ServedAlgo>::Ref;
Registry<ServedAlgo> g_reg;
Snapshot snapshot(int cipher) { return g_reg.snapshot((size_t)cipher); }
Algorithm* algo_of(const Snapshot& s) { return s ? s->algo.get() : nullptr; }
std::mutex g_mu;      // the fixed randomness below
bool g_fixed_rand = false; uint8_t g_r[32], g_s[32], g_mask[32];   // little-endian canonical; written under g_mu, read by fill_randomness under g_mu
DebugVectors g_debug;
// The gsc_debug_* entry points and gsc_set_deterministic_randomness exist for the parity tests only: fixing (r, s, mask) removes
// zero-knowledge for every caller of the process.  They refuse to work unless the process was started with
// GSC_ENABLE_TEST_HOOKS=1; the variable is read ONCE, when the library is loaded, so code running inside the host cannot
// switch them on later.
const bool g_test_hooks = test_hooks_enabled();
bool hooks_refused(const char* what) {
    if (g_test_hooks) return false;
    printf("%s refused: test hooks are disabled (start the process with GSC_ENABLE_TEST_HOOKS=1)\n", what);
    return true;
}

// OS CSPRNG bytes, fetched 16 KiB at a time per thread: a batch of 8192 proofs draws ~25 000 scalars, and one getrandom() system
// call per scalar was a measurable part of the step (the GPU idles meanwhile).  The buffer is wiped as it is consumed.
void csprng_bytes(uint8_t* out, size_t n) {
    thread_local uint8_t pool[16384]; thread_local size_t have = 0;
    while (n) {
        if (!have) {
            size_t got = 0;
            while (got < sizeof pool) {
                const ssize_t k = getrandom(pool + got, sizeof pool - got, 0);
                if (k > 0) got += (size_t)k;
                else if (k < 0 && errno == EINTR) continue;
                else throw std::runtime_error(std::string("getrandom failed: ") + strerror(errno));   // e.g. ENOSYS under seccomp: fail the request, never spin or fall back
            }
            have = sizeof pool;
        }
        const size_t take = n < have ? n : have;
        uint8_t* src = pool + (sizeof pool - have);
        memcpy(out, src, take);
        volatile uint8_t* wipe = src; for (size_t i = 0; i < take; i++) wipe[i] = 0;
        out += take; n -= take; have -= take;
    }
}
void random_fr_le(uint8_t out[32]) {   // uniform in [0, r) by rejection (fr.SetRandom in the reference)
    for (;;) {
        uint8_t be[32]; csprng_bytes(be, 32);
        be[0] &= 0x3F;
        if (memcmp(be, kFrModBE, 32) < 0) { for (int i = 0; i < 32; i++) out[i] = be[31 - i]; return; }
    }
}

// A Go panic value, already rendered as the JSON that libprove.go:33-43 would return.
struct GoPanic { std::string json; };
[[noreturn]] void panic_string(const std::string& msg) { throw GoPanic{json_quote(msg)}; }

int find_cipher(const std::string& name) { for (int i = 0; i < 3; i++) if (name == kAlgorithmNames[i]) return i; return -1; }

bool ascii_fold_eq(const std::string& a, const char* b) {
    size_t n = strlen(b); if (a.size() != n) return false;
    for (size_t i = 0; i < n; i++) { char x = a[i], y = b[i]; if (x >= 'A' && x <= 'Z') x += 32; if (y >= 'A' && y <= 'Z') y += 32; if (x != y) return false; }
    return true;
}

struct Decoded {
    std::string cipher; std::vector<uint8_t> key, nonce, input; uint32_t counter = 0;
    Decoded() = default; Decoded(Decoded&&) = default; Decoded& operator=(Decoded&&) = default; Decoded(const Decoded&) = delete; Decoded& operator=(const Decoded&) = delete;
    ~Decoded() { if (!key.empty()) explicit_bzero(key.data(), key.size()); }      // the decoded key does not linger on the heap
};

// encoding/json semantics for InputParams (provers.go:53-59): case-insensitive keys, unknown keys ignored, the first
// type error is remembered while decoding continues, []uint8 from base64 string / null / array of 0..255.
struct TypeError { bool set = false; std::string json; };
void type_error(TypeError& te, const std::string& value, size_t offset, const char* field) {
    if (te.set) return;
    te.set = true;
    te.json = "{\"Value\":" + json_quote(value) + ",\"Type\":{},\"Offset\":" + std::to_string(offset) + ",\"Struct\":\"InputParams\",\"Field\":" + json_quote(field) + "}";
}
size_t go_offset(const JsonValue& v) { return (v.kind == JsonValue::Array || v.kind == JsonValue::Object) ? v.start + 1 : v.offset; }

void decode_bytes(const JsonValue& v, std::vector<uint8_t>& out, TypeError& te, const char* field) {
    switch (v.kind) {
        case JsonValue::Null: out.clear(); return;
        case JsonValue::String: {
            size_t bad = 0; std::vector<uint8_t> tmp;
            if (!base64_decode(v.text, tmp, bad)) throw GoPanic{std::to_string(bad)};   // base64.CorruptInputError is an int64
            out = std::move(tmp); return;
        }
        case JsonValue::Array: {
            std::vector<uint8_t> tmp;
            for (const JsonValue& e : v.items) {
                uint8_t b = 0;
                if (e.kind == JsonValue::Number) {
                    const std::string& t = e.text; bool ok = !t.empty() && t.find_first_not_of("0123456789") == std::string::npos && t.size() <= 3;
                    unsigned val = ok ? (unsigned)atoi(t.c_str()) : 256;
                    if (val > 255) type_error(te, "number " + t, e.offset, field); else b = (uint8_t)val;
                } else if (e.kind != JsonValue::Null) type_error(te, e.go_kind(), go_offset(e), field);
                tmp.push_back(b);
            }
            out = std::move(tmp); return;
        }
        default: type_error(te, v.go_kind(), go_offset(v), field); return;
    }
}

Decoded decode_params(const JsonValue& root) {
    Decoded d; TypeError te;
    if (root.kind == JsonValue::Null) panic_string("runtime error: invalid memory address or nil pointer dereference");
    if (root.kind != JsonValue::Object) { type_error(te, root.go_kind(), go_offset(root), ""); 
        // Go reports Struct/Field empty for a top-level mismatch
        throw GoPanic{"{\"Value\":" + json_quote(root.go_kind()) + ",\"Type\":{},\"Offset\":" + std::to_string(go_offset(root)) + ",\"Struct\":\"\",\"Field\":\"\"}"}; }
    for (const auto& kv : root.members) {
        const JsonValue& v = kv.second;
        if (ascii_fold_eq(kv.first, "cipher")) {
            if (v.kind == JsonValue::String) d.cipher = v.text; else if (v.kind != JsonValue::Null) type_error(te, v.go_kind(), go_offset(v), "cipher");
        } else if (ascii_fold_eq(kv.first, "key")) decode_bytes(v, d.key, te, "key");
        else if (ascii_fold_eq(kv.first, "nonce")) decode_bytes(v, d.nonce, te, "nonce");
        else if (ascii_fold_eq(kv.first, "input")) decode_bytes(v, d.input, te, "input");
        else if (ascii_fold_eq(kv.first, "counter")) {
            if (v.kind == JsonValue::Number) {
                const std::string& t = v.text; bool ok = !t.empty() && t.find_first_not_of("0123456789") == std::string::npos && t.size() <= 10;
                unsigned long long val = ok ? strtoull(t.c_str(), nullptr, 10) : ~0ull;
                if (!ok || val > 0xFFFFFFFFull) type_error(te, "number " + t, v.offset, "counter"); else d.counter = (uint32_t)val;
            } else if (v.kind != JsonValue::Null) type_error(te, v.go_kind(), go_offset(v), "counter");
        }
    }
    if (te.set) throw GoPanic{te.json};
    return d;
}

// length checks of provers.go:81-89 / :174-182 (log.Panicf -> string panic), then the native cipher
ProofRequest make_request(int cipher, const Decoded& d) {
    ProofRequest q{};
    if (cipher == CHACHA20) { if (d.key.size() != 32) panic_string("key length must be 32: " + std::to_string(d.key.size())); }
    else if (d.key.size() != 32 && d.key.size() != 16) panic_string("key length must be 16 or 32: " + std::to_string(d.key.size()));
    if (d.nonce.size() != 12) panic_string("nonce length must be 12: " + std::to_string(d.nonce.size()));
    if (d.input.size() != 64) panic_string("plaintext length must be 64: " + std::to_string(d.input.size()));
    if (cipher != CHACHA20 && d.key.size() != (cipher == AES_128 ? 16u : 32u)) throw GoPanic{"{}"};   // frontend.NewWitness schema mismatch: an error value with no exported fields
    q.keylen = (uint32_t)d.key.size(); memcpy(q.key, d.key.data(), d.key.size());
    memcpy(q.nonce, d.nonce.data(), 12); q.counter = d.counter; memcpy(q.plaintext, d.input.data(), 64);
    if (cipher == CHACHA20) chacha20_xor_stream(q.key, q.nonce, q.counter, q.plaintext, q.ciphertext, 64);
    else aes_ctr_xor_stream(q.key, q.keylen, q.nonce, q.counter, q.plaintext, q.ciphertext, 64);
    return q;
}
void fill_randomness(ProofRequest& q) {
    if (g_test_hooks) {      // the fixed values can only ever be set in a test process
        std::lock_guard<std::mutex> l(g_mu);
        if (g_fixed_rand) { memcpy(q.r, g_r, 32); memcpy(q.s, g_s, 32); memcpy(q.mask, g_mask, 32); return; }
    }
    random_fr_le(q.r); random_fr_le(q.s); random_fr_le(q.mask);
}

std::string success_json(const ProofResult& r, const uint8_t ct[64]) {   // OutputParams, prove_impl.go:45-52
    return "{\"proof\":{\"proofJson\":\"" + base64_encode(r.proof, r.proof_len) + "\"},\"publicSignals\":\"" + base64_encode(ct, 64) + "\"}";
}

// What one call holds of the algorithms: at most one snapshot per cipher, taken when the call first needs the cipher and kept until the call
// returns — a ProveBatch call is served, from parsing to its last result, by the engines it found.
struct CallSnapshots {
    Snapshot held[3]; bool taken[3] = {false, false, false};
    const Snapshot& of(int cipher) { if (!taken[cipher]) { held[cipher] = snapshot(cipher); taken[cipher] = true; } return held[cipher]; }
};
// parses + validates one request; throws GoPanic
struct Prepared { int cipher; ProofRequest req; };
Prepared prepare(const JsonValue& v, CallSnapshots& snaps) {
    Decoded d = decode_params(v);
    const int cipher = find_cipher(d.cipher);
    if (cipher < 0) panic_string("could not find prover for" + d.cipher);                       // prove_impl.go:141 (sic: no space)
    if (!snaps.of(cipher)) panic_string("proving params are not initialized for cipher: " + d.cipher);   // :124-126
    Prepared p{cipher, make_request(cipher, d)};
    fill_randomness(p.req);
    return p;
}

struct Prove_return to_c(const std::string& s) {
    void* buf = malloc(s.size() ? s.size() : 1);           // C.CBytes
    if (!buf) return {nullptr, 0};
    memcpy(buf, s.data(), s.size());
    return {buf, (GoInt)s.size()};
}

std::string prove_one_json(const char* data, size_t len, DebugVectors* dbg) {
    try {
        JsonValue root;
        try { root = json_parse(data, len); } catch (const JsonSyntaxError& e) { throw GoPanic{"{\"Offset\":" + std::to_string(e.offset) + "}"}; }
        CallSnapshots snaps;
        Prepared p = prepare(root, snaps);
        const Snapshot& served = snaps.of(p.cipher);
        ProofResult res;
        if (dbg) served->algo->prove_batch(&p.req, 1, &res, dbg);          // test hook: straight to the device, keeps the intermediates
        else served->batcher->submit(p.req, res);                         // shares a device batch with concurrent callers
        if (res.status) throw GoPanic{"{}"};     // gnark solver / prover error: no exported fields
        return success_json(res, p.req.ciphertext);
    } catch (const GoPanic& g) {
        printf("%s\n", g.json.c_str());        // libprove.go:35 prints the panic value
        return g.json;
    } catch (const std::exception& e) {
        printf("%s\n", e.what());
        return json_quote(e.what());
    }
}

// A complete engine for `id` with its micro-batcher, from the environment as it stands now; throws std::runtime_error with a printable line.
// vk == nullptr (InitAlgorithm): the self-check as GSC_PROVE_CHECK says.  vk given (gsc_replace_algorithm): non-empty, the check is on under that key
// or there is no engine; empty, as GSC_PROVE_CHECK says.  outgoing: the engine this one will replace (its device bytes count as free for the widths).
std::unique_ptr<ServedAlgo> build_served(GoUint8 id, GoSlice provingKey, GoSlice r1cs, const GoSlice* vk, const ServedAlgo* outgoing) {
    if (!provingKey.data || provingKey.len <= 0 || !r1cs.data || r1cs.len <= 0) throw std::runtime_error("error reading proving key: EOF");
    EngineConfig cfg = config_from_env();
    if (outgoing) {
        const std::vector<int> devs = cfg.devices.empty() ? std::vector<int>{cfg.device} : cfg.devices;
        const auto old = outgoing->algo->replica_bytes();
        for (size_t i = 0; i < devs.size(); i++) cfg.outgoing_bytes.push_back(i < old.size() && old[i].first == devs[i] ? old[i].second : 0);
    }
    std::unique_ptr<Algorithm> algo(new Algorithm((Cipher)id, (const uint8_t*)provingKey.data, (size_t)provingKey.len, (const uint8_t*)r1cs.data, (size_t)r1cs.len, cfg));
    if (vk && vk->data && vk->len > 0) {
        if (!algo->prove_check_init((const uint8_t*)vk->data, (size_t)vk->len)) throw std::runtime_error("gsc_replace_algorithm: the verifying key was refused");
    } else if (cfg.prove_check) {      // GSC_PROVE_CHECK=1: the self-check under the verifying key of GSC_VK_DIR, or no algorithm at all
        static const char* const files[3] = {"vk.chacha20", "vk.aes128", "vk.aes256"};
        const std::string path = cfg.vk_dir + "/" + files[id];
        std::vector<uint8_t> key;
        if (FILE* f = cfg.vk_dir.empty() ? nullptr : fopen(path.c_str(), "rb")) {
            uint8_t buf[4096]; size_t got;
            while ((got = fread(buf, 1, sizeof buf, f)) > 0) key.insert(key.end(), buf, buf + got);
            fclose(f);
        }
        if (key.empty()) throw std::runtime_error("GSC_PROVE_CHECK=1: cannot read " + (cfg.vk_dir.empty() ? std::string("a verifying key: GSC_VK_DIR is not set") : path));
        if (!algo->prove_check_init(key.data(), key.size())) throw std::runtime_error("GSC_PROVE_CHECK=1: " + path + " refused");
    }
    uint8_t digest[32]; sha256_digest((const uint8_t*)provingKey.data, (size_t)provingKey.len, digest);
    char hex[17]; for (int i = 0; i < 8; i++) snprintf(hex + 2 * i, 3, "%02x", digest[i]);
    return std::unique_ptr<ServedAlgo>(new ServedAlgo(std::move(algo), hex));
}
// An engine that has left the registry and is idle, about to be freed: its lanes are at their idle image after every call, and
// this holds them against it once more.  The line below must never appear.
void retire(ServedAlgo& s, const char* who) {
    try {
        const size_t off = s.algo->scrub_before_free();
        if (off) printf("%s: %zu bytes of the outgoing engine's secret regions were off the idle image; every region was wiped before the free\n", who, off);
    } catch (const std::exception& e) { printf("%s: the outgoing engine could not be scanned: %s\n", who, e.what()); }
}

// a result for the caller to release with Free; false when malloc fails
bool hand_over(const std::vector<uint8_t>& f, void** out, size_t* len) {
    void* a = malloc(f.size() ? f.size() : 1);
    if (!a) return false;
    memcpy(a, f.data(), f.size());
    *out = a; *len = f.size();
    return true;
}

}  // namespace

long long gsc_verify_debug_pairing_impl(const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* out, bool few);      // verify_gpu.cpp
int gsc_verify_debug_path_impl(int mode);                                                             // verify_gpu.cpp
int gsc_verify_debug_randomizers_impl(const uint8_t* seed32, int all_ones);                           // verify_gpu.cpp
int gsc_verify_debug_g1_impl(const gsc_debug_verify_g1_args& args);                                   // verify_gpu.cpp

extern "C" {

void enforce_binding(void) {}

GoUint8 InitAlgorithm(GoUint8 algorithmID, GoSlice provingKey, GoSlice r1cs) {
    if (algorithmID > 2) return 0;                               // unknown id -> false (prove_impl.go:113)
    try {
        // already initialised: 1, the new key is dropped (prove_impl.go:74-76).  Otherwise the build — outside the registry's mutex: callers of the
        // other algorithms go on meanwhile; a second InitAlgorithm of this id waits for it and then finds the id initialised
        g_reg.init(algorithmID, [&] { return build_served(algorithmID, provingKey, r1cs, nullptr, nullptr); });
        return 1;
    } catch (const std::exception& e) {
        printf("%s\n", e.what());                                 // fmt.Println(err) in the reference
        return 0;
    }
}

GoUint8 gsc_release_algorithm(GoUint8 algorithmID) {
    if (algorithmID > 2) return 0;
    return g_reg.release(algorithmID, [](ServedAlgo& s) { retire(s, "gsc_release_algorithm"); }) ? 1 : 0;
}

int gsc_replace_algorithm(GoUint8 algorithmID, GoSlice provingKey, GoSlice r1cs, GoSlice verifyingKey) {
    if (algorithmID > 2) return -1;
    try {
        return g_reg.replace(algorithmID, [&](const ServedAlgo& serving) { return build_served(algorithmID, provingKey, r1cs, &verifyingKey, &serving); },
                             [](ServedAlgo& s) { retire(s, "gsc_replace_algorithm"); });
    } catch (const std::exception& e) {
        // the old engine has served throughout and keeps serving; the attempt's device memory went back as the exception unwound
        std::string msg = e.what();
        if (msg.find("out of memory") != std::string::npos) msg += ": the new engine does not fit beside the serving one — gsc_release_algorithm first, then InitAlgorithm";
        printf("%s\n", msg.c_str());
        return 0;
    }
}

uint64_t gsc_key_generation(GoUint8 algorithmID) { return algorithmID > 2 ? 0 : g_reg.generation(algorithmID); }

int gsc_memory_info(int device, uint64_t out[4]) {
    if (!out) return -1;
    try { return device_memory_info(device, out) ? 0 : -1; } catch (const std::exception& e) { printf("gsc_memory_info: %s\n", e.what()); return -1; }
}

void Free(void* pointer) { free(pointer); }

struct Prove_return Prove(GoSlice params) {
    return to_c(prove_one_json((const char*)params.data, params.len > 0 ? (size_t)params.len : 0, nullptr));
}

struct Prove_return ProveBatch(GoSlice params) {
    std::string out;
    try {
        JsonValue root;
        try { root = json_parse((const char*)params.data, params.len > 0 ? (size_t)params.len : 0); }
        catch (const JsonSyntaxError& e) { throw GoPanic{"{\"Offset\":" + std::to_string(e.offset) + "}"}; }
        if (root.kind != JsonValue::Array) throw GoPanic{json_quote("ProveBatch expects a JSON array")};
        const size_t n = root.items.size();
        std::vector<std::string> results(n);
        std::vector<Prepared> ok; std::vector<size_t> where;
        CallSnapshots snaps;      // one per cipher present, from prepare to the last result
        for (size_t i = 0; i < n; i++) {
            try { ok.push_back(prepare(root.items[i], snaps)); where.push_back(i); }
            catch (const GoPanic& g) { results[i] = g.json; }
        }
        // one device batch per algorithm; the algorithms have their own streams and buffers, so their batches run concurrently
        // (the solver levels and the commitment round trip of one hide under the MSMs of another)
        std::exception_ptr err; std::mutex err_mu;
        auto run = [&](int c) {
            try {
                std::vector<ProofRequest> reqs; std::vector<size_t> idx;
                for (size_t k = 0; k < ok.size(); k++) if (ok[k].cipher == c) { reqs.push_back(ok[k].req); idx.push_back(where[k]); }
                if (reqs.empty()) return;
                std::vector<ProofResult> res(reqs.size());
                ServedAlgo& served = *snaps.held[c];      // taken by prepare: a cipher is present only with an engine
                if (reqs.size() <= Batcher<Algorithm>::SMALL_CALL) { served.algo->forget_thread_stat(); served.batcher->submit_many(reqs.data(), reqs.size(), res.data()); }      // a small group shares device batches with concurrent callers
                else served.algo->prove_batch(reqs.data(), reqs.size(), res.data());
                for (size_t k = 0; k < reqs.size(); k++) results[idx[k]] = res[k].status ? std::string("{}") : success_json(res[k], reqs[k].ciphertext);
            } catch (...) { std::lock_guard<std::mutex> g(err_mu); if (!err) err = std::current_exception(); }
        };
        bool present[3] = {false, false, false};
        for (const Prepared& p : ok) present[p.cipher] = true;
        std::vector<std::thread> th;
        int first = -1;
        for (int c = 0; c < 3; c++) if (present[c]) { if (first < 0) first = c; else th.emplace_back(run, c); }
        if (first >= 0) run(first);
        for (auto& t : th) t.join();
        if (err) std::rethrow_exception(err);
        out = "[";
        for (size_t i = 0; i < n; i++) { if (i) out += ","; out += results[i]; }
        out += "]";
    } catch (const GoPanic& g) { out = g.json; }
    catch (const std::exception& e) { out = json_quote(e.what()); }
    return to_c(out);
}

long long gsc_prove_raw(GoUint8 cipher, const uint8_t* inputs, size_t n, uint8_t* proofs, uint32_t* proof_lens, uint8_t* ciphertexts) {
    if (cipher > 2) return -1;
    const Snapshot snap = snapshot(cipher); Algorithm* a = algo_of(snap);
    if (!a) return -1;
    try {
        static const bool trace = getenv("GSC_TRACE_HOST") != nullptr;      // read once
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<ProofRequest> reqs(n); std::vector<ProofResult> res(n);
        for (size_t i = 0; i < n; i++) {
            const uint8_t* rec = inputs + 112 * i; ProofRequest& q = reqs[i]; q = ProofRequest{};
            q.keylen = cipher == AES_128 ? 16 : 32; memcpy(q.key, rec, q.keylen); memcpy(q.nonce, rec + 32, 12);
            q.counter = (uint32_t)rec[44] | ((uint32_t)rec[45] << 8) | ((uint32_t)rec[46] << 16) | ((uint32_t)rec[47] << 24);
            memcpy(q.plaintext, rec + 48, 64);
            if (cipher == CHACHA20) chacha20_xor_stream(q.key, q.nonce, q.counter, q.plaintext, q.ciphertext, 64);
            else aes_ctr_xor_stream(q.key, q.keylen, q.nonce, q.counter, q.plaintext, q.ciphertext, 64);
            fill_randomness(q);
        }
        const auto t1 = std::chrono::steady_clock::now();
        if (n && n <= Batcher<Algorithm>::SMALL_CALL) { a->forget_thread_stat(); snap->batcher->submit_many(reqs.data(), n, res.data()); }      // a small call shares device batches with concurrent callers
        else a->prove_batch(reqs.data(), n, res.data());
        const auto t2 = std::chrono::steady_clock::now();
        if (trace) fprintf(stderr, "gsc_prove_raw: prepare %.2f ms, prove_batch %.2f ms\n", std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count());
        long long good = 0;
        for (size_t i = 0; i < n; i++) {
            if (ciphertexts) memcpy(ciphertexts + 64 * i, reqs[i].ciphertext, 64);
            proof_lens[i] = res[i].status ? 0u : (uint32_t)res[i].proof_len;
            memset(proofs + 196 * i, 0, 196);
            if (!res[i].status) { memcpy(proofs + 196 * i, res[i].proof, res[i].proof_len); good++; }
        }
        return good;
    } catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}

int gsc_prove_check_init(GoUint8 algorithmID, GoSlice verifyingKey) {
    if (algorithmID > 2) return -1;
    const Snapshot snap = snapshot(algorithmID); Algorithm* a = algo_of(snap);
    if (!a) return -1;
    try {
        if (!verifyingKey.data || verifyingKey.len <= 0) { a->prove_check_off(); return 1; }
        return a->prove_check_init((const uint8_t*)verifyingKey.data, (size_t)verifyingKey.len) ? 1 : 0;
    } catch (const std::exception& e) { printf("gsc_prove_check_init: %s\n", e.what()); return 0; }
}
int gsc_prove_check_stats(GoUint8 algorithmID, uint64_t out[4]) {
    if (algorithmID > 2 || !out) return -1;
    const Snapshot snap = snapshot(algorithmID); Algorithm* a = algo_of(snap);
    if (!a) return -1;
    a->prove_check_stats(out);
    return 0;
}
int gsc_debug_prove_corrupt(GoUint8 algorithmID, uint32_t index, int which, int mode) {
    if (hooks_refused("gsc_debug_prove_corrupt") || algorithmID > 2) return -1;
    const Snapshot snap = snapshot(algorithmID); Algorithm* a = algo_of(snap);
    if (!a) return -1;
    return a->debug_prove_corrupt(index, which, mode) ? 0 : -1;
}

int gsc_setup(GoSlice r1cs, const uint8_t* seed32, void** pk, size_t* pk_len, void** vk, size_t* vk_len) {
    if (!pk || !pk_len || !vk || !vk_len) return -1;
    *pk = *vk = nullptr; *pk_len = *vk_len = 0;
    if (seed32 && hooks_refused("gsc_setup with a caller-supplied seed")) return -1;      // deterministic toxic waste: test keys only
    try {
        if (!r1cs.data || r1cs.len <= 0) throw std::runtime_error("error reading r1cs: EOF");
        SetupKeys k = groth16_setup((const uint8_t*)r1cs.data, (size_t)r1cs.len, seed32, config_from_env().device);
        void* a = malloc(k.pk.size()); void* b = malloc(k.vk.size());
        if (!a || !b) { free(a); free(b); return -1; }
        memcpy(a, k.pk.data(), k.pk.size()); memcpy(b, k.vk.data(), k.vk.size());
        *pk = a; *pk_len = k.pk.size(); *vk = b; *vk_len = k.vk.size();
        return 0;
    } catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}

int gsc_setup_contribute(GoSlice pk, GoSlice vk, const uint8_t* seed32, void** pk_out, size_t* pk_len, void** vk_out, size_t* vk_len, uint8_t* record) {
    if (!pk_out || !pk_len || !vk_out || !vk_len || !record) return -2;
    *pk_out = *vk_out = nullptr; *pk_len = *vk_len = 0; memset(record, 0, GSC_CONTRIBUTION_BYTES);
    if (seed32 && hooks_refused("gsc_setup_contribute with a caller-supplied seed")) return -1;      // deterministic secrets: test keys only
    if (!pk.data || pk.len <= 0 || !vk.data || vk.len <= 0) { printf("gsc_setup_contribute: empty key\n"); return -2; }
    try {
        Phase2Step step;
        const int rc = phase2_contribute((const uint8_t*)pk.data, (size_t)pk.len, (const uint8_t*)vk.data, (size_t)vk.len, seed32, step);
        if (rc) return rc;
        void* a = malloc(step.pk.size()); void* b = malloc(step.vk.size());
        if (!a || !b) { free(a); free(b); return -3; }
        memcpy(a, step.pk.data(), step.pk.size()); memcpy(b, step.vk.data(), step.vk.size());
        *pk_out = a; *pk_len = step.pk.size(); *vk_out = b; *vk_len = step.vk.size();
        memcpy(record, step.record, GSC_CONTRIBUTION_BYTES);
        return 0;
    } catch (const std::exception& e) { printf("gsc_setup_contribute: %s\n", e.what()); return -3; }
}
int gsc_setup_verify_contribution(GoSlice pk_prev, GoSlice vk_prev, GoSlice pk_next, GoSlice vk_next, const uint8_t* record) {
    for (const GoSlice* k : {&pk_prev, &vk_prev, &pk_next, &vk_next}) if (!k->data || k->len <= 0) { printf("gsc_setup_verify_contribution: rule 1: empty key\n"); return 0; }
    if (!record) { printf("gsc_setup_verify_contribution: rule 4: no record\n"); return 0; }
    try {
        return phase2_verify((const uint8_t*)pk_prev.data, (size_t)pk_prev.len, (const uint8_t*)vk_prev.data, (size_t)vk_prev.len,
                             (const uint8_t*)pk_next.data, (size_t)pk_next.len, (const uint8_t*)vk_next.data, (size_t)vk_next.len, record);
    } catch (const std::exception& e) { printf("gsc_setup_verify_contribution: %s\n", e.what()); return -3; }
}
int gsc_debug_scale_points(int group, const uint8_t* pts, const uint8_t* inf, size_t n, const uint8_t* scalar_be32, uint8_t* out, uint8_t* out_inf) {
    if (hooks_refused("gsc_debug_scale_points") || !scalar_be32 || (n && (!pts || !inf || !out || !out_inf))) return -1;
    try { phase2_debug_scale(group, pts, inf, n, scalar_be32, out, out_inf); return 0; }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}

int gsc_srs_verify(GoSlice srs) {
    if (!srs.data || srs.len <= 0) { printf("gsc_srs_verify: rule 1: srs: empty file\n"); return 0; }
    try { return srs_verify((const uint8_t*)srs.data, (size_t)srs.len); }
    catch (const std::exception& e) { printf("gsc_srs_verify: %s\n", e.what()); return -3; }
}
int gsc_srs_initial(int L, void** srs, size_t* len) {
    if (!srs || !len) return -2;
    *srs = nullptr; *len = 0;
    try {
        std::vector<uint8_t> f;
        if (!srsc::initial(L, f)) { printf("gsc_srs_initial: L outside [1, 24]\n"); return -2; }
        return hand_over(f, srs, len) ? 0 : -2;
    } catch (const std::exception& e) { printf("gsc_srs_initial: %s\n", e.what()); return -2; }
}
int gsc_srs_contribute(GoSlice srs, const uint8_t* seed32, void** srs_out, size_t* len, uint8_t* record) {
    if (!srs_out || !len || !record) return -2;
    *srs_out = nullptr; *len = 0; memset(record, 0, GSC_SRS_CONTRIBUTION_BYTES);
    if (seed32 && hooks_refused("gsc_srs_contribute with a caller-supplied seed")) return -1;      // deterministic secrets: test files only
    if (!srs.data || srs.len <= 0) { printf("gsc_srs_contribute: srs: empty file\n"); return -2; }
    try {
        std::vector<uint8_t> f; uint8_t rec[GSC_SRS_CONTRIBUTION_BYTES];
        const int rc = srs_contribute((const uint8_t*)srs.data, (size_t)srs.len, seed32, f, rec);
        if (rc) return rc;
        if (!hand_over(f, srs_out, len)) return -3;
        memcpy(record, rec, GSC_SRS_CONTRIBUTION_BYTES);
        return 0;
    } catch (const std::exception& e) { printf("gsc_srs_contribute: %s\n", e.what()); return -3; }
}
int gsc_srs_verify_contribution(GoSlice prev, GoSlice next, const uint8_t* record) {
    if (!prev.data || prev.len <= 0 || !next.data || next.len <= 0) { printf("gsc_srs_verify_contribution: rule 1: srs: empty file\n"); return 0; }
    if (!record) { printf("gsc_srs_verify_contribution: rule 2: no record\n"); return 0; }
    try { return srs_verify_contribution((const uint8_t*)prev.data, (size_t)prev.len, (const uint8_t*)next.data, (size_t)next.len, record); }
    catch (const std::exception& e) { printf("gsc_srs_verify_contribution: %s\n", e.what()); return -3; }
}
int gsc_debug_scale_powers(int group, const uint8_t* pts, const uint8_t* inf, size_t n, const uint8_t* x_be32, const uint8_t* m_be32, uint64_t first, uint8_t* out, uint8_t* out_inf) {
    if (hooks_refused("gsc_debug_scale_powers") || !x_be32 || !m_be32 || (n && (!pts || !inf || !out || !out_inf))) return -1;
    try { srs_debug_scale_powers(group, pts, inf, n, x_be32, m_be32, first, out, out_inf); return 0; }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}
int gsc_setup_from_srs(GoSlice r1cs, GoSlice srs, const uint8_t* seed32, void** pk, size_t* pk_len, void** vk, size_t* vk_len) {
    if (!pk || !pk_len || !vk || !vk_len) return -2;
    *pk = *vk = nullptr; *pk_len = *vk_len = 0;
    if (seed32 && hooks_refused("gsc_setup_from_srs with a caller-supplied seed")) return -1;      // chosen gamma, delta, sigma: test keys only
    if (!r1cs.data || r1cs.len <= 0 || !srs.data || srs.len <= 0) { printf("gsc_setup_from_srs: empty r1cs or powers file\n"); return -2; }
    try {
        SetupKeys k = setup_from_srs((const uint8_t*)r1cs.data, (size_t)r1cs.len, (const uint8_t*)srs.data, (size_t)srs.len, seed32);
        void* a = malloc(k.pk.size()); void* b = malloc(k.vk.size());
        if (!a || !b) { free(a); free(b); return -3; }
        memcpy(a, k.pk.data(), k.pk.size()); memcpy(b, k.vk.data(), k.vk.size());
        *pk = a; *pk_len = k.pk.size(); *vk = b; *vk_len = k.vk.size();
        return 0;
    } catch (const SrsRefused& e) { printf("gsc_setup_from_srs: %s\n", e.what()); return -2; }
    catch (const std::exception& e) { printf("gsc_setup_from_srs: %s\n", e.what()); return -3; }
}
int gsc_pedersen_verify(GoSlice pk, GoSlice vk) {
    if (!pk.data || pk.len <= 0 || !vk.data || vk.len <= 0) { printf("gsc_pedersen_verify: rule 1: empty key\n"); return 0; }
    try { return pedersen_verify((const uint8_t*)pk.data, (size_t)pk.len, (const uint8_t*)vk.data, (size_t)vk.len); }
    catch (const std::exception& e) { printf("gsc_pedersen_verify: %s\n", e.what()); return -3; }
}
int gsc_setup_contribute_sigma(GoSlice pk, GoSlice vk, const uint8_t* seed32, void** pk_out, size_t* pk_len, void** vk_out, size_t* vk_len, uint8_t* record) {
    if (!pk_out || !pk_len || !vk_out || !vk_len || !record) return -2;
    *pk_out = *vk_out = nullptr; *pk_len = *vk_len = 0; memset(record, 0, GSC_SIGMA_CONTRIBUTION_BYTES);
    if (seed32 && hooks_refused("gsc_setup_contribute_sigma with a caller-supplied seed")) return -1;      // deterministic secrets: test keys only
    if (!pk.data || pk.len <= 0 || !vk.data || vk.len <= 0) { printf("gsc_setup_contribute_sigma: empty key\n"); return -2; }
    try {
        SigmaStep step;
        const int rc = sigma_contribute((const uint8_t*)pk.data, (size_t)pk.len, (const uint8_t*)vk.data, (size_t)vk.len, seed32, step);
        if (rc) return rc;
        void* a = malloc(step.pk.size()); void* b = malloc(step.vk.size());
        if (!a || !b) { free(a); free(b); return -3; }
        memcpy(a, step.pk.data(), step.pk.size()); memcpy(b, step.vk.data(), step.vk.size());
        *pk_out = a; *pk_len = step.pk.size(); *vk_out = b; *vk_len = step.vk.size();
        memcpy(record, step.record, GSC_SIGMA_CONTRIBUTION_BYTES);
        return 0;
    } catch (const std::exception& e) { printf("gsc_setup_contribute_sigma: %s\n", e.what()); return -3; }
}
int gsc_setup_verify_sigma_contribution(GoSlice pk_prev, GoSlice vk_prev, GoSlice pk_next, GoSlice vk_next, const uint8_t* record) {
    for (const GoSlice* k : {&pk_prev, &vk_prev, &pk_next, &vk_next}) if (!k->data || k->len <= 0) { printf("gsc_setup_verify_sigma_contribution: rule 1: empty key\n"); return 0; }
    if (!record) { printf("gsc_setup_verify_sigma_contribution: rule 3: no record\n"); return 0; }
    try {
        return sigma_verify((const uint8_t*)pk_prev.data, (size_t)pk_prev.len, (const uint8_t*)vk_prev.data, (size_t)vk_prev.len,
                            (const uint8_t*)pk_next.data, (size_t)pk_next.len, (const uint8_t*)vk_next.data, (size_t)vk_next.len, record);
    } catch (const std::exception& e) { printf("gsc_setup_verify_sigma_contribution: %s\n", e.what()); return -3; }
}
int gsc_setup_verify_from_srs(GoSlice r1cs, GoSlice srs, GoSlice pk, GoSlice vk) {
    if (!r1cs.data || r1cs.len <= 0 || !srs.data || srs.len <= 0) { printf("gsc_setup_verify_from_srs: empty r1cs or powers file\n"); return -2; }
    if (!pk.data || pk.len <= 0 || !vk.data || vk.len <= 0) { printf("gsc_setup_verify_from_srs: rule 1: empty key\n"); return 0; }
    try {
        return setup_verify_from_srs((const uint8_t*)r1cs.data, (size_t)r1cs.len, (const uint8_t*)srs.data, (size_t)srs.len, (const uint8_t*)pk.data, (size_t)pk.len,
                                     (const uint8_t*)vk.data, (size_t)vk.len);
    } catch (const SrsRefused& e) { printf("gsc_setup_verify_from_srs: %s\n", e.what()); return -2; }
    catch (const std::exception& e) { printf("gsc_setup_verify_from_srs: %s\n", e.what()); return -3; }
}
int gsc_debug_group_idft(int group, int L, const uint8_t* pts, uint8_t* out, uint8_t* out_inf) {
    if (hooks_refused("gsc_debug_group_idft") || !pts || !out || !out_inf) return -1;
    try { srs_debug_group_idft(group, L, pts, out, out_inf); return 0; }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}
int gsc_debug_column_sums(int group, uint32_t n_rows, const uint8_t* rows, uint32_t n_cols, const uint32_t* col_start, const uint32_t* term_row, const uint32_t* term_coeff,
                          uint32_t n_coeff, const uint8_t* coeff_be, uint8_t* out, uint8_t* out_inf) {
    if (hooks_refused("gsc_debug_column_sums") || !col_start || (n_rows && !rows) || (n_coeff && !coeff_be) || (n_cols && (!out || !out_inf))) return -1;
    if (col_start[n_cols] && (!term_row || !term_coeff)) return -1;
    try { srs_debug_column_sums(group, n_rows, rows, n_cols, col_start, term_row, term_coeff, n_coeff, coeff_be, out, out_inf); return 0; }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}
int gsc_debug_msm(const gsc_debug_msm_args* args) {
    if (hooks_refused("gsc_debug_msm") || !args) return -1;
    try { debug_msm(config_from_env().device, *args); return 0; }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}
int gsc_debug_solve(const gsc_debug_solve_args* args) {
    if (hooks_refused("gsc_debug_solve") || !args) return -1;
    try { return debug_solve(config_from_env().device, *args); }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}
int gsc_debug_assemble(const gsc_debug_assemble_args* args) {
    if (hooks_refused("gsc_debug_assemble") || !args) return -1;
    try { debug_assemble(config_from_env().device, *args); return 0; }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}
int gsc_debug_srs_generate(int L, const uint8_t* seed32, void** srs, size_t* len) {
    if (!srs || !len) return -1;
    *srs = nullptr; *len = 0;
    if (hooks_refused("gsc_debug_srs_generate") || !seed32) return -1;
    try {
        const std::vector<uint8_t> f = srs_debug_generate(L, seed32, config_from_env().device);
        void* a = malloc(f.size());
        if (!a) return -1;
        memcpy(a, f.data(), f.size());
        *srs = a; *len = f.size();
        return 0;
    } catch (const std::exception& e) { printf("gsc_debug_srs_generate: %s\n", e.what()); return -1; }
}

int gsc_set_deterministic_randomness(const uint8_t* r_be32, const uint8_t* s_be32, const uint8_t* mask_be32) {
    if (hooks_refused("gsc_set_deterministic_randomness")) return -1;
    std::lock_guard<std::mutex> l(g_mu);
    if (!r_be32 || !s_be32) { g_fixed_rand = false; return 0; }
    for (int i = 0; i < 32; i++) { g_r[i] = r_be32[31 - i]; g_s[i] = s_be32[31 - i]; g_mask[i] = mask_be32 ? mask_be32[31 - i] : 0; }
    g_fixed_rand = true;
    return 0;
}

long long gsc_debug_prove(GoSlice params) {
    if (hooks_refused("gsc_debug_prove")) return -1;
    g_debug = DebugVectors();
    std::string r = prove_one_json((const char*)params.data, params.len > 0 ? (size_t)params.len : 0, &g_debug);
    return r.find("\"proof\"") != std::string::npos ? 0 : -1;
}
long long gsc_debug_vector(int which, uint8_t* out, size_t cap) {
    if (hooks_refused("gsc_debug_vector")) return -1;
    const std::vector<uint8_t>* v = which == 0 ? &g_debug.W : which == 1 ? &g_debug.A : which == 2 ? &g_debug.B : which == 3 ? &g_debug.C : which == 4 ? &g_debug.H : nullptr;
    if (!v || v->empty()) return -1;
    if (out) memcpy(out, v->data(), cap < v->size() ? cap : v->size());
    return (long long)(v->size() / 32);
}

int gsc_debug_field_ops(int field, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n, int chain) {
    if (hooks_refused("gsc_debug_field_ops")) return -1;
    try { debug_field_ops(config_from_env().device, field, op, a, b, out, n, chain); return 0; }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}

int gsc_debug_limb_ops(int field, int op, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d, int32_t* out, size_t n) {
    if (hooks_refused("gsc_debug_limb_ops") || !a || !out) return -1;
    try { debug_limb_ops(config_from_env().device, field, op, a, b, c, d, out, n); return 0; }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}
int gsc_debug_curve_ops(int group, int op, const uint8_t* pts, const uint8_t* inf, const uint8_t* lam, size_t n, size_t k, uint8_t* out, uint8_t* flags) {
    if (hooks_refused("gsc_debug_curve_ops") || !pts || !inf || !lam || !out || !flags) return -1;
    try { debug_curve_ops(config_from_env().device, group, op, pts, inf, lam, n, k, out, flags); return 0; }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}

int gsc_debug_decode_points(int group, const uint8_t* bytes, size_t len, size_t n, uint8_t* out_xy, uint8_t* status) {
    if (hooks_refused("gsc_debug_decode_points") || (len && !bytes) || (n && (!out_xy || !status))) return -1;
    try { debug_decode_points(config_from_env().device, group, bytes, len, n, out_xy, status); return 0; }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}

int gsc_debug_tower_ops(int path, int op, const int32_t* in, size_t n, int32_t* out, uint8_t* flags) {
    if (hooks_refused("gsc_debug_tower_ops") || (n && (!in || !out || !flags))) return -1;
    try {
        if (debug_tower_ops(config_from_env().device, path, op, in, n, out, flags)) return 0;
        printf("gsc_debug_tower_ops: path %d has no op %d\n", path, op);
        return -1;
    } catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}

int gsc_debug_clock_trace(uint32_t n, uint32_t interval_us, unsigned long long* out) {
    if (hooks_refused("gsc_debug_clock_trace") || !out || !n) return -1;
    try { debug_clock_trace(config_from_env().device, n, interval_us, out); return 0; }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}

long long gsc_debug_pairing(const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* out) {
    if (hooks_refused("gsc_debug_pairing") || (n && (!g1 || !g2 || !out))) return -1;
    return gsc_verify_debug_pairing_impl(g1, g2, n, out, false);
}
long long gsc_debug_pairing_few(const uint8_t* g1, const uint8_t* g2, size_t n, uint8_t* out) {
    if (hooks_refused("gsc_debug_pairing_few") || (n && (!g1 || !g2 || !out))) return -1;
    return gsc_verify_debug_pairing_impl(g1, g2, n, out, true);
}
int gsc_debug_verify_path(int mode) {
    if (hooks_refused("gsc_debug_verify_path")) return -1;
    return gsc_verify_debug_path_impl(mode);
}
int gsc_debug_verify_randomizers(const uint8_t* seed32, int all_ones) {
    if (hooks_refused("gsc_debug_verify_randomizers")) return -1;
    return gsc_verify_debug_randomizers_impl(seed32, all_ones);
}
int gsc_debug_verify_g1(const gsc_debug_verify_g1_args* args) {
    if (hooks_refused("gsc_debug_verify_g1") || !args) return -1;
    return gsc_verify_debug_g1_impl(*args);
}
int gsc_debug_glv_split(const uint8_t* k, uint8_t* out) {
    if (hooks_refused("gsc_debug_glv_split") || !k || !out) return -1;
    uint32_t w[8]; memcpy(w, k, 32);
    GlvSplit s;
    if (!glv_split(w, s)) return -1;
    memcpy(out, s.k1, 20); memcpy(out + 20, s.k2, 20); memcpy(out + 40, &s.neg, 4);
    return 0;
}
long long gsc_debug_compute_h(GoUint8 algorithmID, const uint8_t* abc_be, size_t m, uint8_t* h_out, size_t cap) {
    if (hooks_refused("gsc_debug_compute_h") || algorithmID > 2) return -1;
    const Snapshot snap = snapshot(algorithmID); Algorithm* a = algo_of(snap); if (!a) return -1;
    if (!h_out) return (long long)a->domain_size();
    if (cap < a->domain_size() * 64 * 32) return -1;
    try { a->debug_compute_h(abc_be, m, h_out); return (long long)a->domain_size(); }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}

long long gsc_debug_secret_residue(GoUint8 algorithmID) {
    if (hooks_refused("gsc_debug_secret_residue") || algorithmID > 2) return -1;
    const Snapshot snap = snapshot(algorithmID); Algorithm* a = algo_of(snap); if (!a) return -1;
    try { return (long long)a->debug_secret_residue(); } catch (const std::exception& e) { fprintf(stderr, "gsc_debug_secret_residue: %s\n", e.what()); return -1; }
}
long long gsc_debug_secret_scan(GoUint8 algorithmID, char* out, size_t cap) {
    if (hooks_refused("gsc_debug_secret_scan") || algorithmID > 2) return -1;
    const Snapshot snap = snapshot(algorithmID); Algorithm* a = algo_of(snap); if (!a) return -1;
    try {
        std::string report;
        const long long total = (long long)a->debug_secret_scan(report);
        if (out && cap) { const size_t n = report.size() < cap - 1 ? report.size() : cap - 1; memcpy(out, report.data(), n); out[n] = 0; }
        return total;
    } catch (const std::exception& e) { fprintf(stderr, "gsc_debug_secret_scan: %s\n", e.what()); return -1; }
}
int gsc_debug_wipe(uint64_t bytes, int fill, const uint64_t* desc, size_t ndesc, const uint8_t* cls, size_t ncls, uint8_t* buf_out, const uint64_t* win, size_t nwin, uint64_t* counts, float* ms) {
    if (hooks_refused("gsc_debug_wipe") || (ndesc && !desc) || (nwin && (!win || !counts)) || (ncls && !cls) || ndesc > 4096 || nwin > 4096) return -1;
    try { const float t = debug_wipe(config_from_env().device, bytes, fill, desc, ndesc, cls, ncls, buf_out, win, nwin, counts); if (ms) *ms = t; return 0; }
    catch (const std::exception& e) { fprintf(stderr, "gsc_debug_wipe: %s\n", e.what()); return -1; }
}
long long gsc_debug_compute_d(GoUint8 algorithmID, const uint8_t* ab_be, size_t m, uint8_t* d_out, size_t cap) {
    if (hooks_refused("gsc_debug_compute_d") || algorithmID > 2) return -1;
    const Snapshot snap = snapshot(algorithmID); Algorithm* a = algo_of(snap); if (!a) return -1;
    if (!d_out) return (long long)a->domain_size();
    if (cap < a->domain_size() * 64 * 32) return -1;
    try { a->debug_compute_d(ab_be, m, d_out); return (long long)a->domain_size(); }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}
long long gsc_debug_quotient(const gsc_debug_quotient_args* args) {
    if (hooks_refused("gsc_debug_quotient") || !args || args->algorithm > 2) return -1;
    const Snapshot snap = snapshot((GoUint8)args->algorithm); Algorithm* a = algo_of(snap); if (!a) return -1;
    if (!args->out) return (long long)a->domain_size();
    try {
        a->debug_quotient_routes(args->mats_be, args->m, args->planes, args->plain, args->ncols, args->live, args->c, args->out, args->cap);
        return (long long)a->domain_size();
    } catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}
int gsc_debug_z_sum(GoUint8 algorithmID, const uint8_t* abc_be, size_t m, uint8_t* out, uint8_t* flags) {
    if (hooks_refused("gsc_debug_z_sum") || algorithmID > 2 || !abc_be || !out || !flags) return -1;
    const Snapshot snap = snapshot(algorithmID); Algorithm* a = algo_of(snap); if (!a) return -1;
    try { a->debug_z_sum(abc_be, m, out, flags); return 0; }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}

int gsc_debug_quot_fold_dft(int L, uint32_t m, const uint32_t* perm, const uint8_t* u_be, const uint8_t* u_inf, const uint8_t* v_be, const uint8_t* v_inf,
                            uint8_t* u2_be, uint8_t* u2_inf, uint8_t* v2_be, uint8_t* v2_inf) {
    if (hooks_refused("gsc_debug_quot_fold_dft") || L < 2 || L > 17 || m < 2 || m > (1u << L) || !u_be || !u_inf || !v_be || !v_inf || !u2_be || !u2_inf || !v2_be || !v2_inf) return -1;
    try { debug_quot_fold_dft(config_from_env().device, L, m, perm, u_be, u_inf, v_be, v_inf, u2_be, u2_inf, v2_be, v2_inf); return 0; }
    catch (const std::exception& e) { printf("%s\n", e.what()); return -1; }
}

size_t gsc_describe(GoUint8 algorithmID, char* out, size_t cap) {
    if (algorithmID > 2 || !cap) return 0;
    const Snapshot snap = snapshot(algorithmID); Algorithm* a = algo_of(snap);
    std::string s = a ? a->describe() + " key=" + snap->key_id + " gen=" + std::to_string(snap.generation()) : std::string("not initialised");
    size_t n = s.size() < cap - 1 ? s.size() : cap - 1; memcpy(out, s.data(), n); out[n] = 0; return n;
}
int gsc_last_dominant_kernel(GoUint8 algorithmID, char* name, size_t cap, float* ms, size_t* statements, size_t* columns, size_t* nbases) {
    if (algorithmID > 2) return -1;
    const Snapshot snap = snapshot(algorithmID); Algorithm* a = algo_of(snap); if (!a) return -1;
    const KernelStat st = a->last_kernel_stat();
    if (name && cap) { const size_t n = strlen(st.name) < cap - 1 ? strlen(st.name) : cap - 1; memcpy(name, st.name, n); name[n] = 0; }
    if (ms) *ms = st.ms;
    if (statements) *statements = st.statements;
    if (columns) *columns = st.columns;
    if (nbases) *nbases = st.nbases;
    return 0;
}
int gsc_last_kernel_clock(GoUint8 algorithmID, float* clock_mhz, int* windows) {
    if (algorithmID > 2) return -1;
    const Snapshot snap = snapshot(algorithmID); Algorithm* a = algo_of(snap); if (!a) return -1;
    const KernelStat st = a->last_kernel_stat();
    if (clock_mhz) *clock_mhz = st.clock_mhz;
    if (windows) *windows = st.nwin;
    return 0;
}
int gsc_last_stage_ms(GoUint8 algorithmID, float out[4]) {
    if (algorithmID > 2) return -1;
    const Snapshot snap = snapshot(algorithmID); Algorithm* a = algo_of(snap); if (!a) return -1;
    const KernelStat st = a->last_kernel_stat();
    for (int i = 0; i < 4; i++) out[i] = st.stage_ms[i];
    return 0;
}

}  // extern "C"
