// What the key ceremony's host code shares (phase2_gpu.cpp: contributions to a key pair; srs_gpu.cpp: the check of a powers file;
// srs_contrib_gpu.cpp: contributions to a powers file): device buffers and a stream that clean up behind themselves, the OS CSPRNG, the
// decoding of raw key points through the verifier's key-point kernel and their way back to bytes, one point times a public scalar, the
// generators, the refusal line.  Host code that calls HIP: include it from the *_gpu.cpp files only.
#pragma once
#include "phase2_kernels.hpp"
#include "verify_kernels.hpp"
#include "srs.hpp"
#include "phase2.hpp"
#include "host_field.hpp"
#include <sys/random.h>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

int gsc_verify_device_impl();                                                                                        // verify_gpu.cpp
void gsc_verify_draw_rho_impl(uint32_t* out, size_t n);                                                               // verify_gpu.cpp

namespace gsc {
namespace cer {

#define GSC_CER_HIP_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #expr); } while (0)

struct Buf {
    void* p = nullptr; size_t bytes = 0; bool secret = false;      // secret: zeroed before it is freed, also when an exception unwinds
    explicit Buf(size_t n, bool is_secret = false) : bytes(n ? n : 1), secret(is_secret) { GSC_CER_HIP_CHECK(hipMalloc(&p, bytes)); }
    Buf(const Buf&) = delete; Buf& operator=(const Buf&) = delete;
    ~Buf() { if (p) { if (secret) { (void)hipMemset(p, 0, bytes); (void)hipDeviceSynchronize(); } (void)hipFree(p); } }
    template <class T> T* as() const { return static_cast<T*>(p); }
};
struct Stream {
    hipStream_t s = nullptr;
    Stream() { GSC_CER_HIP_CHECK(hipSetDevice(gsc_verify_device_impl())); GSC_CER_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
};
inline void need_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw std::runtime_error("no HIP device available: the key ceremony computes on the GPU");
}
inline void os_random(void* out, size_t n) {      // OS CSPRNG bytes; a failure fails the call, never a fallback
    for (size_t got = 0; got < n;) {
        const ssize_t r = getrandom((uint8_t*)out + got, n - got, 0);
        if (r > 0) got += (size_t)r;
        else if (!(r < 0 && errno == EINTR)) throw std::runtime_error(std::string("getrandom failed: ") + strerror(errno));
    }
}
// a secret scalar: uniform in [1, r) by rejection; and its image for the device, little-endian canonical bytes
inline hostf::Fr random_nonzero_fr() {
    for (;;) {
        uint8_t be[32];
        os_random(be, 32);
        be[0] &= 0x3F;
        hostf::Fr v;
        const bool ok = hostf::Fr::from_be(be, v) && !v.is_zero();
        explicit_bzero(be, sizeof be);
        if (ok) return v;
    }
}
inline void fr_to_le(const hostf::Fr& v, uint8_t out[32]) { hostf::U256 c = v.canon(); memcpy(out, c.w, 32); explicit_bzero(&c, sizeof c); }
// n fresh non-zero 128-bit values, four little-endian words each: the factors of a verifier's random combination
inline std::vector<uint32_t> random_rho(size_t n) {
    std::vector<uint32_t> rho(4 * n);
    os_random(rho.data(), 16 * n);
    for (size_t i = 0; i < n; i++) while (!(rho[4 * i] | rho[4 * i + 1] | rho[4 * i + 2] | rho[4 * i + 3])) os_random(&rho[4 * i], 16);
    return rho;
}
// the same through the verifier's draw_randomizers: the OS CSPRNG unless gsc_debug_verify_randomizers (a test hook) says otherwise
inline std::vector<uint32_t> verifier_rho(size_t n) { std::vector<uint32_t> rho(4 * n); gsc_verify_draw_rho_impl(rho.data(), n); return rho; }

// Decodes n1 G1 slots (64 B) and n2 G2 slots (128 B) with the verifier's key-point kernel.  Returns the index of the first refused
// point (G1 slots count first, then G2), or -1 when every point is accepted.
inline long long decode_slots_first_bad(const std::vector<uint8_t>& s1, size_t n1, const std::vector<uint8_t>& s2, size_t n2, vfy::VP1* o1, vfy::VP2* o2, hipStream_t s) {
    if (!(n1 + n2)) return -1;
    Buf d1(s1.size()), d2(s2.size()), st(n1 + n2);
    if (n1) GSC_CER_HIP_CHECK(hipMemcpyAsync(d1.p, s1.data(), s1.size(), hipMemcpyHostToDevice, s));
    if (n2) GSC_CER_HIP_CHECK(hipMemcpyAsync(d2.p, s2.data(), s2.size(), hipMemcpyHostToDevice, s));
    launch_verify_key_points(d1.as<uint8_t>(), n1, d2.as<uint8_t>(), n2, o1, o2, st.as<int8_t>(), s);
    GSC_CER_HIP_CHECK(hipGetLastError());
    std::vector<int8_t> hs(n1 + n2);
    GSC_CER_HIP_CHECK(hipMemcpyAsync(hs.data(), st.p, hs.size(), hipMemcpyDeviceToHost, s));
    GSC_CER_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t i = 0; i < hs.size(); i++) if (hs[i] < 0) return (long long)i;
    return -1;
}
// false when a point is refused (st < 0)
inline bool decode_slots(const std::vector<uint8_t>& s1, size_t n1, const std::vector<uint8_t>& s2, size_t n2, vfy::VP1* o1, vfy::VP2* o2, hipStream_t s) {
    return decode_slots_first_bad(s1, n1, s2, n2, o1, o2, s) < 0;
}
// the decoded points of one key file on the device
struct DevKey {
    phase2::Walk w; size_t n1 = 0, n2 = 0;
    Buf g1, g2;
    DevKey(const phase2::Walk& walk) : w(walk), n1(walk.g1.size()), n2(walk.g2.size()), g1(sizeof(vfy::VP1) * walk.g1.size()), g2(sizeof(vfy::VP2) * walk.g2.size()) {}
    vfy::VP1* p1() const { return g1.as<vfy::VP1>(); }
    vfy::VP2* p2() const { return g2.as<vfy::VP2>(); }
};
inline bool decode_file(const uint8_t* b, DevKey& k, hipStream_t s) {
    std::vector<uint8_t> s1, s2;
    phase2::slots(b, k.w.g1, 32, s1); phase2::slots(b, k.w.g2, 64, s2);
    return decode_slots(s1, k.n1, s2, k.n2, k.p1(), k.p2(), s);
}
// raw big-endian bytes (and infinity flags) of n decoded points
template <class P> void download(const P* p, size_t n, uint8_t* out, uint8_t* inf, hipStream_t s) {
    constexpr size_t W = sizeof(P) == sizeof(vfy::VP1) ? 64 : 128;
    if (!n) return;
    Buf d(W * n), di(n);
    launch_points_be(p, n, d.as<uint8_t>(), di.as<uint8_t>(), s);
    GSC_CER_HIP_CHECK(hipGetLastError());
    GSC_CER_HIP_CHECK(hipMemcpyAsync(out, d.p, W * n, hipMemcpyDeviceToHost, s));
    GSC_CER_HIP_CHECK(hipMemcpyAsync(inf, di.p, n, hipMemcpyDeviceToHost, s));
    GSC_CER_HIP_CHECK(hipStreamSynchronize(s));
}

// one line on stdout; the caller returns rc (a refused step or file: 0; a refused contribution: -2)
inline int refuse(const char* who, const std::string& why, int rc = 0) { printf("%s: %s\n", who, why.c_str()); return rc; }

using srs::generators;      // raw big-endian G1 and G2 generators (srs.hpp: the host-only writer of gsc_srs_initial needs them too)

// k P for one decoded G1 point and a public scalar (big-endian, < r), as raw bytes (zeros for the point at infinity): a Schnorr equation's side
inline void scale_one(const vfy::VP1* p, const uint8_t k_be[32], uint8_t out[64], hipStream_t s) {
    uint8_t le[32]; for (int i = 0; i < 32; i++) le[i] = k_be[31 - i];
    Buf dk(32), o(sizeof(vfy::VP1));
    GSC_CER_HIP_CHECK(hipMemcpyAsync(dk.p, le, 32, hipMemcpyHostToDevice, s));
    launch_scale_points(p, 1, dk.as<uint32_t>(), o.as<vfy::VP1>(), s);
    GSC_CER_HIP_CHECK(hipGetLastError());
    uint8_t inf;
    download(o.as<vfy::VP1>(), 1, out, &inf, s);
}

}  // namespace cer
}  // namespace gsc
