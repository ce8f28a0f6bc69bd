/* libprove.h — C-ABI of the MI355X-native Groth16 prover for the gnark-symmetric-crypto circuits.
 *
 * Drop-in for the header cgo generates from the reference's libraries/prover/libprove.go
 * (`go build -buildmode=c-shared`, reference README.md:83-96): same symbol names, same argument
 * layout (GoSlice by value, GoUint8 for bool, struct Prove_return), same ownership rules.
 * Additions that the reference does not have are grouped at the end and prefixed gsc_ / named ProveBatch.
 */
#ifndef GSC_LIBPROVE_H
#define GSC_LIBPROVE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef unsigned char GoUint8;
typedef long long GoInt;
typedef struct { void *data; GoInt len; GoInt cap; } GoSlice;   /* passed BY VALUE */
struct Prove_return { void *r0; /* proofRes */ GoInt r1; /* resLen */ };

/* libprove.go:17-18 — no-op that forces the dynamic loader to bind the library. */
extern void enforce_binding(void);

/* libprove.go:20-23 -> impl.InitAlgorithm (prove_impl.go:65-114).
 * algorithmID: 0 chacha20, 1 aes-128-ctr, 2 aes-256-ctr (prove_impl.go:15-25).
 * provingKey / r1cs: the gnark v0.11.0 files written by keygen.go:341-352 (read only during the call).
 * Key points are read as gnark's ReadFrom reads them, element by element: the two top bits of an element's first byte say whether it is
 * compressed (10 / 11, 01 = infinity: what WriteTo writes) or raw (00: X | Y, what WriteRawTo writes; all-zero bytes = infinity), and one
 * key may mix the two.  Every point must have canonical coordinates and lie on its curve, and every G2 point (G2.B, beta, delta) must
 * lie in the subgroup of order r: a key gnark refuses with "subgroup check failed" is refused here.
 * Returns 1 on success or if the algorithm is already initialised, 0 on unknown id / parse failure / a refused key
 * (one line on stdout, as the reference prints it; nothing of the failed attempt stays allocated and a later call may succeed). */
extern GoUint8 InitAlgorithm(GoUint8 algorithmID, GoSlice provingKey, GoSlice r1cs);

/* libprove.go:25-28 — releases a buffer returned by Prove / ProveBatch (C free()). */
extern void Free(void *pointer);

/* libprove.go:30-47 -> impl.Prove (prove_impl.go:116-143).
 * params: JSON {"cipher","key","nonce","counter","input"} (provers.go:53-59).
 * Returns a malloc'd, NOT NUL-terminated JSON buffer and its length:
 *   success: {"proof":{"proofJson":"<base64>"},"publicSignals":"<base64 ciphertext>"}
 *   failure: the JSON encoding of the Go panic value (a quoted string for message panics, an object for
 *            decode errors); never unwinds across the ABI. */
extern struct Prove_return Prove(GoSlice params);

/* ---- additions (not in the reference) ---- */

/* Proves many independent statements in one device batch.  params: JSON array of Prove inputs (ciphers may be
 * mixed).  Returns a JSON array whose i-th element is exactly what Prove would have returned for element i. */
extern struct Prove_return ProveBatch(GoSlice params);

/* Binary batch entry used by bench.py / tests (no JSON on the timed path).
 * cipher: algorithm id.  inputs: n records of 112 bytes {key[32] (AES-128: first 16 used), nonce[12],
 * counter u32 little-endian, input[64]}.  proofs: n x 196 bytes, proof_lens: n (0 on failure),
 * ciphertexts: n x 64 bytes.  Returns the number of proofs produced, or -1 if the algorithm is not initialised.
 * A call of up to 32 statements (here and in ProveBatch) shares device batches with concurrent callers, like single Prove calls do. */
extern long long gsc_prove_raw(GoUint8 cipher, const uint8_t *inputs, size_t n, uint8_t *proofs, uint32_t *proof_lens, uint8_t *ciphertexts);

/* Groth16 Setup for one of the reference's circuits (stands in for groth16.Setup, keygen.go:345,384,423; needed because the
 * reference ships no pk.aes128 / pk.aes256).  r1cs: the gnark v0.11.0 constraint system file.  On success (0) *pk / *vk are malloc'd
 * buffers in groth16.ProvingKey.WriteTo / VerifyingKey.WriteTo layout (what InitAlgorithm and the verifier read); release both
 * with Free.  The group elements are computed on the GPU.  seed32 == NULL: toxic waste from the OS CSPRNG, discarded before the
 * call returns.  A non-NULL 32-byte seed makes the keys a deterministic function of (r1cs, seed) — TEST keys — and is refused (-1)
 * unless test hooks are enabled (below). */
extern int gsc_setup(GoSlice r1cs, const uint8_t *seed32, void **pk, size_t *pk_len, void **vk, size_t *vk_len);

/* TEST HOOKS.  gsc_set_deterministic_randomness and every gsc_debug_* function below refuse to work (return -1, message on
 * stdout) unless the process was started with GSC_ENABLE_TEST_HOOKS=1 in its environment; the variable is read once, when the
 * library is loaded.  A production host never sets it: fixed prover randomness voids zero-knowledge for the whole process. */

/* TEST HOOK: fixes the prover randomness (r, s, AES commitment mask; 32-byte big-endian, < Fr modulus) for every
 * subsequent proof of this process; pass NULLs to return to the OS CSPRNG (the default).  With it fixed the proof is a
 * deterministic function of the inputs, which is what byte-level parity with gnark is defined on.
 * Returns 0, or -1 when test hooks are disabled. */
extern int gsc_set_deterministic_randomness(const uint8_t *r_be32, const uint8_t *s_be32, const uint8_t *mask_be32);

/* TEST HOOK: runs one proof and copies the intermediate vectors of the device pipeline for parity tests.
 * which: 0 W (n_wires), 1 A, 2 B, 3 C (n_constraints), 4 h (domain size; element k = h_{bitrev(k)}).
 * Elements are 32 bytes, little-endian 32-bit limbs; W/A/B/C are in Montgomery form (x*2^256 mod r), h is canonical.
 * Call gsc_debug_prove first; gsc_debug_vector returns the element count (or -1) and copies min(cap, size) bytes. */
extern long long gsc_debug_prove(GoSlice params);
extern long long gsc_debug_vector(int which, uint8_t *out, size_t cap);

/* TEST HOOK: element-wise operations of the device's field arithmetic, for unit tests against big integers.
 * field: 0 = Fp, 1 = Fr in radix 2^29 (plain-C products); 2 = Fp in radix 2^29 with the carry-chained multiply-add products that every
 *        G1 kernel uses; 3 = Fp, 4 = Fr in the saturated 8 x 32-bit form (decompression, Setup, the generic solver).
 * op: 0 mul, 1 add, 2 sub, 3 sqr, 4 inverse, 5 r*b - b*a (fused), 6 neg, 7 (r-b)*(a+b); fields 3 and 4 have no ops 5 and 7; field 1 alone
 *     has op 8, the solver's inversion of 64 values at once.  The op is applied `chain` times to a running value r that starts at a.
 * a, b, out: n canonical 32-byte little-endian values.  0 on success; -1 for a field / op that does not exist (nothing runs then). */
extern int gsc_debug_field_ops(int field, int op, const uint8_t *a, const uint8_t *b, uint8_t *out, size_t n, int chain);

/* TEST HOOK: one radix-2^29 operation on RAW limbs: every operand and the result are n x 9 int32 limbs (value = sum l[i] 2^(29 i)), used
 * exactly as given, in the 2^261 Montgomery domain, without conversion, freeze or pack; this is how operands of every class the field code
 * admits (tight, signed-tight, loose) reach its instructions.  field: 0, 1, 2 as above.  op: 0 mul(a, b), 1 sqr(a), 2 fmms(a, b, c, d) =
 * a*b - c*d, 3 norm(a), 4 freeze(a), 5 freeze_near(a); operands an op does not read may be NULL.  The caller keeps the operands inside the
 * domains bn254_fp29.hpp documents.  0 on success, -1 on error. */
extern int gsc_debug_limb_ops(int field, int op, const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d, int32_t *out, size_t n);

/* TEST HOOK: the XYZZ group law of the device (Curve9), one operation or accumulation per element.  group: 0 = G1 (over field 2 above),
 * 1 = G2 (over Fp2).  A coordinate is one (G1) or two (G2: real, imaginary) canonical 32-byte little-endian values.
 * pts: n x k affine points (x, y); inf: n x k flags, non-zero = the point at infinity (coordinates ignored); lam: n x 2 non-zero field
 * elements, the scales under which points 0 and 1 enter where they are XYZZ operands: (x l^2, y l^3, l^2, l^3).
 * op: 0 dbl(P0), k = 1;  1 P0 + P1 + ... with madd<true> (exact), k >= 2;  2 the same with madd<false> (no equality tests), k >= 2;
 *     3 add(P0, P1), k = 2;  4 to_aff(P0), k = 1;  5 k >= 1 points into four partial sums with madd<true>, the sums joined with add.
 *     Points that enter as affine operands (ops 1, 2: all but P0; op 5: all) must not be infinity.
 * out: n affine results (zeros when there is none); flags: n bytes, bit 0 the result is infinity, bit 1 (op 2) ZZ was 0 mod p after the
 * first addition, bit 2 (op 2) ZZ was 0 mod p after the last one: then there is no result.  0 on success, -1 on error. */
extern int gsc_debug_curve_ops(int group, int op, const uint8_t *pts, const uint8_t *inf, const uint8_t *lam, size_t n, size_t k, uint8_t *out, uint8_t *flags);

/* TEST HOOK: decodes a slice of encoded key points exactly as InitAlgorithm does: the host walk over the elements (each compressed or
 * raw by the flag bits of its first byte, see InitAlgorithm above) and the decode kernels, for G2 with the subgroup test [r]Q = O.
 * Needs a device, no key.  group: 0 = G1, 1 = G2.  bytes / len: n encoded elements and nothing else (a slice that ends inside an
 * element, or bytes left over: -1).  out_xy: n x 64 (G1: X | Y) or n x 128 (G2: X.A1 | X.A0 | Y.A1 | Y.A0) canonical big-endian bytes,
 * zeros unless the status is 0.  status: n bytes, 0 a point of the group, 1 refused (a coordinate >= p, off the curve, a malformed
 * infinity, G2: outside the subgroup), 2 the point at infinity.  0 on success, -1 on error. */
extern int gsc_debug_decode_points(int group, const uint8_t *bytes, size_t len, size_t n, uint8_t *out_xy, uint8_t *status);

/* TEST HOOK: one operation of the GPU verifier's arithmetic per element on RAW limbs: the Fp / Fp2 helpers, the Fp12 tower, the Miller steps
 * and the final exponentiation of csrc/verify_dev.hpp (path 0: one element per thread) and the Fp12 operations of its lane-sliced twin
 * csrc/verify_few_dev.hpp (path 1: one element per group of 8 lanes; a group without an element computes on the identity, as in
 * production).  An Fp value is 9 int32 limbs in the 2^261 Montgomery domain, used exactly as given; Fp2 = (real, imaginary) = 18 words;
 * Fp12 = the coefficients of w^0..w^5 = 108 words; a line = (a, b, c) = 54 words; k, ka, kb are one int32 each.  The caller keeps the
 * operands inside the discipline verify_dev.hpp documents (tight limbs, |value| < 5p).  in / out: n elements, the words of one element:
 *   op  0 red(a)  1 lin(a, b, ka, kb) = ka a + kb b               in 9 / 20, out 9
 *       2 add2(a, b)  3 sub2(a, b)  6 mul2(a, b)                  in 36, out 18
 *       4 neg2  5 conj2  7 sqr2  9 mulxi  12 inv2                 in 18, out 18
 *       8 scale2(a, k in Fp)  10 small2(a, k)                     in 27 / 19, out 18
 *       11 inv1  13 sqrt1 (flag: a root exists; out: a root, else zeros)       in 9, out 9
 *       14 sqrt2 (flag and out likewise)  15 lex_large2 (flag)    in 18, out 18 / 0
 *       16 mul12(a, b)  17 sqr12  18 mul_line(f, c0, c1, c3)      in 216 / 108 / 162, out 108
 *       19 conj12  20 frob12  21 frob12_2  22 inv12  23 pow_x  24 final_exp  25 is_one12 (flag, out 0)       in 108, out 108
 *       26 dbl_step(X, Y, Z)  27 add_step(X, Y, Z, xQ, yQ): T' (X, Y, Z) and the line      in 54 / 90, out 108
 *       28 frob_points(xQ, yQ): pi(Q), -pi^2(Q)  29 lines_of(xQ, yQ): the 102 lines of the Miller loop      in 36, out 72 / 5508
 * Path 1 has ops 16..25 only and returns 144 words per Fp12 value: the slice of each of the 8 lanes (lanes 6 and 7 hold zero).
 * flags: n bytes, 0 for an op without a flag.  0 on success; -1 for a path / op that does not exist (nothing is launched then) and on error. */
extern int gsc_debug_tower_ops(int path, int op, const int32_t *in, size_t n, int32_t *out, uint8_t *flags);

/* TEST HOOK: the quotient-polynomial kernels (computeH) alone, on caller-supplied vectors, 64 independent columns at once.
 * abc_be: a, b, c one after the other, each [m][64] canonical big-endian 32-byte values (m <= constraints of the algorithm).
 * h_out (cap bytes, at least domain*64*32): [domain][64] canonical little-endian values, row k = coefficient bitrev(k).
 * Returns the domain size (also when h_out is NULL: size query), -1 on error. */
extern long long gsc_debug_compute_h(GoUint8 algorithmID, const uint8_t *abc_be, size_t m, uint8_t *h_out, size_t cap);
/* TEST HOOK: the quotient kernels of the EVALUATION form alone (what batch calls run: four transforms instead of six; see
 * csrc/k_quot_bases.hip).  ab_be: a, then b, each [m][64] canonical big-endian values.  d_out: [domain][64] canonical little-endian
 * values, row i = A(zeta w^i) * B(zeta w^i) * 2^261 mod r in natural order (zeta: the primitive 2n-th root of unity, w = zeta^2 the
 * domain generator; A, B the interpolation polynomials of a, b).  Returns the domain size (also for d_out == NULL), -1 on error. */
extern long long gsc_debug_compute_d(GoUint8 algorithmID, const uint8_t *ab_be, size_t m, uint8_t *d_out, size_t cap);
/* TEST HOOK: n samples {100 MHz clock, shader clock}, interval_us apart, taken by a one-wave kernel that stays resident beside whatever the
 * device runs meanwhile (call it from a thread of its own around a Prove): the shader clock each kernel of a call is granted.  Blocks. */
extern int gsc_debug_clock_trace(uint32_t n, uint32_t interval_us, unsigned long long *out);
/* TEST HOOK: bytes of a finished call's secrets (key wires of the witness, r, s, -rs, the raw input records, commitment masks) that are still
 * non-zero in the algorithm's device buffers — the engine clears them behind the last kernel of every call, so 0; -1 on error / hooks disabled. */
extern long long gsc_debug_secret_residue(GoUint8 algorithmID);
// TEST HOOK: the evaluation-form quotient sum (sum c_i U_i + sum d_i V_i) of 64 columns through the batch kernels and whatever sets InitAlgorithm built.
// abc_be: a, b, c = a b row by row, [m][64] canonical big-endian values; out: 64 x 64 B big-endian X | Y; flags[i] = 1: the point at infinity.  0 on success.
extern int gsc_debug_z_sum(GoUint8 algorithmID, const uint8_t *abc_be, size_t m, uint8_t *out, uint8_t *flags);
/* TEST HOOK: every key-derived device buffer of the algorithm against its idle image.  Synchronises every lane, then counts on the device, over the whole
 * allocation of every region classed secret (every device allocation of a lane but the public ones: results, verdicts, timing words), the bytes that differ from
 * the idle image: zero, or 0x80 in the rows of the byte planes that are marked wide for good.  out (cap bytes, NUL-terminated): "lane<i>.<name>=<bytes> " for every
 * region that is not clean, then "registered=<bytes> allocated=<bytes> public=<comma-separated names>" (registered: the bytes of the lanes' region tables; allocated:
 * the bytes their allocations took: equal unless a buffer is missing from the table).  Returns the total — 0 after InitAlgorithm and after any call, however it left —
 * or -1 on error / hooks disabled. */
extern long long gsc_debug_secret_scan(GoUint8 algorithmID, char *out, size_t cap);
/* TEST HOOK: the kernels behind that, k_wipe and k_scan_idle, on a buffer of their own (needs a device, no key).  Allocates `bytes` bytes of device memory, fills them
 * with the byte `fill`, and applies ndesc descriptors {offset, rows, pitch, width, image} (five uint64 each: `rows` rows of `width` bytes, `pitch` apart, from `offset`;
 * image != 0: instead of zero, row i gets 0x80 where cls[i mod ncls] != 0) with ONE launch sequence of k_wipe.  buf_out (may be NULL; `bytes` bytes): the buffer
 * afterwards.  win: nwin scan windows in the same five-word format, counts[i] = bytes of window i that differ from its idle image (k_scan_idle), so that large
 * buffers need no host copy.  *ms (may be NULL): device time of the k_wipe launch.  Descriptors and windows must lie inside the buffer.  0 on success, -1 on error. */
extern int gsc_debug_wipe(uint64_t bytes, int fill, const uint64_t *desc, size_t ndesc, const uint8_t *cls, size_t ncls, uint8_t *buf_out,
                          const uint64_t *win, size_t nwin, uint64_t *counts, float *ms);
// TEST HOOK: the fold of the Z bases that the domain's zero padding makes redundant, by three group transforms, on caller-supplied bases (needs a device, no
// InitAlgorithm).  n = 2^L, 2 <= L <= 17, 2 <= m <= n; perm: n entries, table position -> coset index (NULL: the identity); u_be (m points) and v_be (n points,
// table order): 64 B big-endian X | Y each, *_inf[i] = 1: the point at infinity.  Out: U' (m) and V' (m - 1) in the same format.  0 on success, -1 on error.
extern int gsc_debug_quot_fold_dft(int L, uint32_t m, const uint32_t *perm, const uint8_t *u_be, const uint8_t *u_inf, const uint8_t *v_be, const uint8_t *v_inf,
                                   uint8_t *u2_be, uint8_t *u2_inf, uint8_t *v2_be, uint8_t *v2_inf);
/* TEST HOOK (host arithmetic only, no GPU): the GLV split the latency path feeds to its scalar multiplications
 * (csrc/glv.hpp).  k: canonical scalar < r, 32 bytes little-endian.  out: 20 bytes |k1|, 20 bytes |k2| (little-endian), 4 bytes
 * flags (bit 0: k1 < 0, bit 1: k2 < 0) with k = k1 + k2 * lambda (mod r).  Returns 0, -1 on error. */
extern int gsc_debug_glv_split(const uint8_t *k, uint8_t *out);

/* Human-readable description of an initialised algorithm (sizes, table memory, and per engine replica of GSC_DEVICES the calls /
 * statements it has served so far: "served(calls/statements)=a/b,c/d"); returns bytes written. */
extern size_t gsc_describe(GoUint8 algorithmID, char *out, size_t cap);
/* Device milliseconds of the four stages (witness, quotient, msm, assembly) of the batch of that algorithm that finished last. */
extern int gsc_last_stage_ms(GoUint8 algorithmID, float out[4]);
/* The dominant kernel of the batch of that algorithm that finished last, timed with HIP events on the kernel's own stream (bench.py's
 * roofline object).  Batch calls: "k_msm_win<Fp29f>", the Z-table gather-accumulate.  Calls of a handful of statements (the latency
 * path): the resident witness kernel "k_solver_few".  name: NUL-terminated kernel name (cap bytes); *ms: milliseconds; *statements:
 * statements the call proved; *columns: the 64-padded batch the kernels ran on; *nbases: fixed bases per proof of the Z set.
 * Any out pointer may be NULL.  Returns 0, -1 when the algorithm is not initialised. */
extern int gsc_last_dominant_kernel(GoUint8 algorithmID, char *name, size_t cap, float *ms, size_t *statements, size_t *columns, size_t *nbases);
/* For the same batch: *clock_mhz = the shader clock the Z-table kernel ran at (clock stamps of one wave in the middle of the launch; 0 when
 * the call took the latency path), *windows = the digit windows of its Z set.  bench.py prices the kernel's VALU-issue roofline with them.
 * The three gsc_last_* functions report the calling thread's own last gsc_prove_raw / ProveBatch call of more than 32 statements; on a thread
 * that made none, the chunk that finished last on any replica. */
extern int gsc_last_kernel_clock(GoUint8 algorithmID, float *clock_mhz, int *windows);

/* ---- GPU verifier (k_verify.hip): verdicts identical to libverify.so's Verify, computed on the device ---- */
/* Loads a verifying key (gnark VerifyingKey.WriteTo bytes, as InitVerifier takes) for the GPU verifier.  algorithmID: 0 chacha20,
 * 1 aes-128-ctr, 2 aes-256-ctr.  Needs no InitAlgorithm.  1 on success, 0 on a bad key (a point that does not decode, a beta / gamma /
 * delta outside G2, as libverify refuses it).  Each point of the key may be compressed or raw (WriteRawTo's X | Y, flag bits 00), as for
 * InitAlgorithm; proofs stay compressed in their 196-byte slots.  Loading again replaces the key.  Without a call, keys load on first use from
 * GSC_VK_DIR (vk.chacha20, vk.aes128, vk.aes256), as libverify does.  Device: GSC_DEVICE, or the first of GSC_DEVICES. */
extern int gsc_verify_init(GoUint8 algorithmID, GoSlice verifyingKey);
/* n proofs of one algorithm.  proofs: n x 196-byte slots (gsc_prove_raw's layout), proof_lens[i] the length of proof i; signals:
 * n x 144 bytes (ct | nonce | counter | pt, as Verify's publicSignals).  verdicts[i] = 1 iff Verify would accept item i.  Returns the
 * number accepted, -1 if no key is loaded for the algorithm, -2 on a device error (then every verdict is 0).  Thread-safe; calls on
 * one key run one after the other on the verifier's own stream, beside any proving. */
extern long long gsc_verify_raw(GoUint8 algorithmID, const uint8_t *proofs, const uint32_t *proof_lens, const uint8_t *signals, size_t n,
                                uint8_t *verdicts);
/* JSON array of Verify inputs ({"cipher","proof","publicSignals"}; ciphers may be mixed) -> malloc'd JSON array of true/false,
 * element i == Verify(element i).  A top-level syntax error gives {"Offset":n}, a non-array the quoted string
 * "VerifyBatch expects a JSON array" (ProveBatch's shapes).  Release with Free. */
extern struct Prove_return VerifyBatch(GoSlice params);
/* TEST HOOK: n reduced pairings e(P_i, Q_i) = f^((p^12-1)/r) on the device.  P: 64 bytes x | y, Q: 128 bytes x.A1 | x.A0 | y.A1 | y.A0,
 * big-endian canonical; all zero = infinity; points must lie on their curves.  out: 12 x 32 big-endian bytes per result, coefficient
 * 2i + j = component j (of 1, u) of the w^i coefficient in Fp12 = Fp2[w]/(w^6 - (9+u)), Fp2 = Fp[u]/(u^2+1).  Returns n, -1 when hooks
 * are off or on error. */
extern long long gsc_debug_pairing(const uint8_t *g1_uncompressed, const uint8_t *g2_uncompressed, size_t n, uint8_t *out);
/* Batched check (k_verify_batch.hip): per chunk of 65 536 items, with fresh random nonzero 128-bit rho_i (and t_i for the AES
 * keys' proof of knowledge) from the OS CSPRNG, one final exponentiation decides
 *   prod_i e(rho_i A_i, B_i) e(-(sum rho_i) alpha, beta) e(-sum rho_i L_i, gamma) e(-sum rho_i C_i, delta)
 *   (* e(sum t_i D_i, ped_gsn) e(sum t_i PoK_i, ped_g)) == 1.
 * Same arguments, return values and verdicts as gsc_verify_raw.  A chunk whose check fails is verified again proof by proof, so the
 * verdicts are gsc_verify_raw's; when it holds, every item that decodes is accepted (wrong with probability about 2^-128). */
extern long long gsc_verify_raw_batched(GoUint8 algorithmID, const uint8_t *proofs, const uint32_t *proof_lens, const uint8_t *signals,
                                        size_t n, uint8_t *verdicts);
/* The same check as a yes / no answer for a whole set: 1 iff Verify would accept every item (n = 0: 1), 0 otherwise (no
 * proof-by-proof pass: it stops at the first failing chunk), -1 if no key is loaded for the algorithm, -2 on a device error. */
extern int gsc_verify_all(GoUint8 algorithmID, const uint8_t *proofs, const uint32_t *proof_lens, const uint8_t *signals, size_t n);
/* JSON array of Verify inputs (VerifyBatch's; ciphers may be mixed, each cipher checked with gsc_verify_all) -> 1 iff Verify would
 * accept every element.  Malformed JSON, a non-array, an empty array, an element that does not parse or a cipher without a key: 0. */
extern GoUint8 VerifyAll(GoSlice params);
/* Claim-wise batched check (k_verify_claims.hip): the equation above with the claim as its unit.
 * m claims over n items of one algorithm; claim j is the contiguous run of items [claim_ends[j-1], claim_ends[j]) (claim_ends[-1] = 0).
 * verdicts[j] = 1 iff Verify would accept every item of claim j (an empty claim: 1).  Each claim is decided by a batched check of its
 * own (fresh random rho_i, t_i per item, as gsc_verify_raw_batched draws them): no claim's verdict depends on another claim's items, and
 * there is no proof-by-proof pass.  A claim holding a bad proof is accepted with probability about 2^-128.
 * Returns the number of claims accepted; -1 no key loaded; -2 device error (every verdict 0); -3 when claim_ends is not non-decreasing
 * or claim_ends[m-1] != n (m == 0 requires n == 0) - nothing runs and verdicts is not written.
 * proofs, proof_lens and signals as in gsc_verify_raw; routing and chunks (8192 / 65 536 items) as in every entry point above.  A claim
 * that crosses a chunk boundary is cut there into parts, each an equation of its own: the claim holds iff all of them do. */
extern long long gsc_verify_claims(GoUint8 algorithmID, const uint8_t *proofs, const uint32_t *proof_lens, const uint8_t *signals, size_t n,
                                   const uint64_t *claim_ends, size_t m, uint8_t *verdicts);
/* JSON array of claims, each a JSON array of Verify inputs (ciphers may be mixed inside a claim) -> malloc'd JSON array of true/false,
 * one per claim.  A claim that is not an array, is empty, holds an element that does not parse or names a cipher without a key is
 * false and leaves the others alone.  Each cipher's share of all claims goes through gsc_verify_claims once; a claim's verdict is the
 * AND of its shares.  A top-level syntax error gives {"Offset":n}, a non-array the quoted string "VerifyClaims expects a JSON array".
 * Release with Free. */
extern struct Prove_return VerifyClaims(GoSlice params);
/* TEST HOOK: the randomizers of the batched checks (gsc_verify_claims included).  seed32 (32 bytes): a fixed function of the seed from now on; all_ones != 0:
 * every rho_i = t_i = 1 (the naive sum, which swapped public inputs of two proofs pass; it takes precedence over a seed); NULL
 * seed and all_ones == 0: the OS CSPRNG again (the default).  Returns 0, -1 when hooks are off. */
extern int gsc_debug_verify_randomizers(const uint8_t *seed32, int all_ones);
/* Few-proof path (k_verify_few.hip): a call of at most GSC_VERIFY_FEW_MAX items of one algorithm (read once, when the key loads; 0
 * switches the path off) is verified by groups of 8 lanes sharing one proof's pairing instead of one thread per proof.  Every entry
 * point above routes by itself (such a call is processed in chunks of 8192, the batched check included); verdicts do not depend on
 * the path.  The batched check's final exponentiation always runs there.  Default: 8192, the measured crossover. */
/* One Verify input ({"cipher","proof","publicSignals"}) answered on the GPU: 1 iff Verify would accept it; anything malformed, an
 * unknown cipher or a cipher without a key: 0.  Shares VerifyBatch's parser. */
extern GoUint8 gsc_verify_json(GoSlice params);
/* Which kernels the last verifier call on this key took: 1 one thread per proof, 2 the few-proof groups, 0 no call yet, -1 no key
 * loaded (or algorithmID > 2). */
extern int gsc_verify_last_path(GoUint8 algorithmID);
/* TEST HOOK: the routing of every later verifier call.  0 automatic (by GSC_VERIFY_FEW_MAX), 1 always one thread per proof, 2 always
 * the few-proof groups (any n, in chunks of 8192).  Returns 0, -1 when hooks are off or mode is none of these. */
extern int gsc_debug_verify_path(int mode);
/* TEST HOOK: gsc_debug_pairing's arguments and output, computed by the few-proof kernels (the lines of Q_i, the Miller loop over
 * them and the lane-sliced final exponentiation). */
extern long long gsc_debug_pairing_few(const uint8_t *g1_uncompressed, const uint8_t *g2_uncompressed, size_t n, uint8_t *out);

/* ---- the prover's self-check (an addition; off unless asked for) ----
 * With the check on for an algorithm, a proof leaves Prove / ProveBatch / gsc_prove_raw only if Verify (libverify.so, gsc_verify_raw) would
 * accept the released bytes under the loaded verifying key and the public signals ct | nonce | counter | pt, which the host builds from the
 * request and its own ciphertext.  Every chunk is decided on the device before anything is downloaded: the verifier's batch check over the
 * chunk's points as they lie in the prover's output buffers (coordinates < p, the curve equations exactly, [r]B = infinity, then one final
 * exponentiation), and the per-proof pairings when that fails.  A proof that fails is refused exactly as a prover error is: "{}" from Prove /
 * ProveBatch, proof_lens[i] = 0 and a zeroed slot from gsc_prove_raw; every other proof of the chunk is released unchanged, byte for byte what
 * the call gives with the check off.  Statements the prover refuses anyway (solver status, degenerate points) take no part.
 *
 * gsc_prove_check_init: verifyingKey = gnark VerifyingKey.WriteTo bytes (the decoder and the refusals of gsc_verify_init, raw points
 * included).  Builds one check context per engine replica on that replica's device.  1 = on; 0 = the key was refused (a line on stdout; the
 * state stays as it was); -1 = the algorithm is not initialised.  An empty slice turns the check off and frees the contexts (1).  Safe beside
 * running Prove calls: a chunk is checked under the key that was loaded when it started, or not at all.
 * GSC_PROVE_CHECK=1 in the environment makes InitAlgorithm do this itself with vk.chacha20 / vk.aes128 / vk.aes256 from GSC_VK_DIR; a missing
 * or refused file makes InitAlgorithm return 0 with one line on stdout. */
extern int gsc_prove_check_init(GoUint8 algorithmID, GoSlice verifyingKey);
/* out: chunks checked, proofs checked, proofs refused by the check, chunks that needed the proof-by-proof pass — summed over the replicas,
 * since the key was loaded; all 0 while the check is off.  Returns 0, -1 when the algorithm is not initialised.  gsc_describe reports
 * check=off or check=on(<bytes of device memory of the contexts>). */
extern int gsc_prove_check_stats(GoUint8 algorithmID, uint64_t out[4]);
/* TEST HOOK: arms a one-shot change to statement `index` of the algorithm's next chunk, applied on the device behind the assembly and in
 * front of the check and the download, inside that proof's own output slot.  which: 0 A, 1 B, 2 C, 3 D, 4 PoK (3, 4: AES only).  mode 0: the
 * same point of statement (index + 1) mod n — a valid group element in the wrong equation; mode 1: bit 0 of the point's y flipped — off the
 * curve.  An index past the chunk changes nothing.  Returns 0; -1 when hooks are off, the algorithm is not initialised or which / mode is none. */
extern int gsc_debug_prove_corrupt(GoUint8 algorithmID, uint32_t index, int which, int mode);

/* ---- key lifecycle (an addition): give an algorithm's tables back, or put another key in its place, without restarting the host ----
 * A call — Prove, ProveBatch, gsc_prove_raw, every query — is served whole by the engine it found when it entered.  The calls below may run
 * beside any number of such calls; those of one id serialise among themselves (and with InitAlgorithm of that id), and callers of the other
 * ids are never held up.  InitAlgorithm on an initialised id still returns 1 and drops its key.
 *
 * gsc_release_algorithm: takes the algorithm out: from that instant Prove / ProveBatch answer "proving params are not initialized for cipher:
 * ..." and gsc_prove_raw -1.  Then waits until every call that had entered is through (callers parked in the micro-batcher are served), checks
 * that the idle engine's secret regions are at their idle image, and frees the engine, its lanes, its self-check contexts: all its device
 * memory is back when the call returns, and InitAlgorithm works as in a fresh process.  1 = released; 0 = not initialised or unknown id. */
extern GoUint8 gsc_release_algorithm(GoUint8 algorithmID);
/* gsc_replace_algorithm: builds a complete new engine beside the serving one (all replicas of GSC_DEVICES; the environment as InitAlgorithm
 * reads it), swaps, waits until the last call under the old key has left and frees the old engine.  1 = swapped: every call that enters from
 * now on is served by the new key and the old key's memory is back.  0 = refused, with one line on stdout (a key that does not parse, a refused
 * key point, a wrong circuit, a refused verifying key, device memory that does not hold both engines — release first, then InitAlgorithm): the
 * old engine has served throughout and keeps serving, nothing of the attempt stays allocated, the generation does not move.  -1 = the id is not
 * initialised (use InitAlgorithm).  The new engine takes the digit widths a fresh InitAlgorithm would choose once the old engine is gone.
 * Self-check: a non-empty verifyingKey turns it on for the new engine under that key (refused key = refused replacement); an empty one leaves
 * it off, or, with GSC_PROVE_CHECK=1, on under GSC_VK_DIR's file.  The old verifying key never checks a new key's proofs. */
extern int gsc_replace_algorithm(GoUint8 algorithmID, GoSlice provingKey, GoSlice r1cs, GoSlice verifyingKey);
/* out: free and total device memory (hipMemGetInfo), bytes held on that device by the provers (key tables and lane buffers of every complete
 * engine replica), bytes held there by verifier keys and self-check contexts.  Returns 0; -1 for a device that does not exist. */
extern int gsc_memory_info(int device, uint64_t out[4]);
/* 0 while not initialised; 1 after InitAlgorithm; +1 per successful gsc_replace_algorithm; 0 again after a release.  gsc_describe ends in
 * key=<first 16 hex digits of SHA-256 of the proving key's bytes> gen=<n>.  A caller who must know which key made a proof reads the
 * generation before and after the call: equal values name it. */
extern uint64_t gsc_key_generation(GoUint8 algorithmID);

/* ---- key ceremony, second phase (an addition): several parties each re-randomise delta of a key pair, so that forging
 * proofs under the final key needs every one of them to collude (or to have kept their secret).  tau, alpha, beta and gamma are NOT
 * re-randomised: that is the first phase (gsc_srs_initial / gsc_srs_contribute below, then gsc_setup_from_srs).
 * A contribution draws a secret x in [1, r) and makes, from (pk, vk) in gnark's layouts (points compressed or raw, as InitAlgorithm takes them),
 * G1.Delta' = x G1.Delta and G2.Delta' = x G2.Delta in pk and vk, G1.Z'[k] = (1/x) G1.Z[k] and G1.K'[i] = (1/x) G1.K[i] in pk; every other byte
 * of both files is copied; the rewritten points are written compressed.  The result is an ordinary key pair for InitAlgorithm,
 * gsc_replace_algorithm, gsc_verify_init, libverify.so and gnark.
 * The record (GSC_CONTRIBUTION_BYTES, this project's own format, NOT gnark's mpcsetup transcript): SHA-256(pk_prev) | SHA-256(pk_next) |
 * G1.Delta' raw X | Y | T = k G1.Delta_prev raw | z = k + c x mod r, big-endian; c = the first 31 bytes, as a big-endian integer, of
 * SHA-256("gsc-phase2-v1" | SHA-256(pk_prev) | Delta_prev raw | Delta' raw | T raw): a Schnorr proof that the contributor knows x.
 * x and k come from the OS CSPRNG; with seed32 (TEST HOOKS only) x = SHA-256("gsc-phase2-x" | seed32) mod r, k = SHA-256("gsc-phase2-k" | seed32) mod r.
 * Neither call needs an initialised algorithm or an R1CS; both run on GSC_DEVICE, or the first of GSC_DEVICES, and are thread-safe. */
#define GSC_CONTRIBUTION_BYTES 224
/* 0 on success: *pk_out / *vk_out malloc'd (release with Free), record filled.  -1: seed given without test hooks;
 * -2: a key that does not parse / a refused point / pk and vk that disagree on delta; -3: device error.  On failure
 * the outputs are NULL / 0, the record is zeroed, nothing stays allocated. */
extern int gsc_setup_contribute(GoSlice pk, GoSlice vk, const uint8_t *seed32,
                                void **pk_out, size_t *pk_len, void **vk_out, size_t *vk_len,
                                uint8_t record[GSC_CONTRIBUTION_BYTES]);
/* One step (prev, next, record) is accepted iff (1) both pairs parse and every point decodes as for InitAlgorithm / gsc_verify_init, neither delta
 * at infinity; (2) outside delta, Z and K next equals prev BYTE FOR BYTE (a re-encoded key — raw for compressed — is refused); (3) pk and vk of each
 * pair carry the same deltas; (4) the record's hashes and Delta' match the files; (5) z Delta_prev == T + c Delta'; (6) e(Delta'_1, G_2) =
 * e(G_1, Delta'_2); (7) with fresh non-zero 128-bit rho_i from the OS CSPRNG, e(sum rho_i P'_i, Delta'_2) = e(sum rho_i P_i, Delta_prev_2) over Z and K.
 * A wrong step is accepted with probability about 2^-128.
 * 1 accepted, 0 refused (one line on stdout naming the first rule that failed), -3 device error. */
extern int gsc_setup_verify_contribution(GoSlice pk_prev, GoSlice vk_prev, GoSlice pk_next, GoSlice vk_next,
                                         const uint8_t record[GSC_CONTRIBUTION_BYTES]);
/* TEST HOOK: out[i] = scalar * pts[i].  group 0 G1 (64 B X|Y), 1 G2 (128 B X.A1|X.A0|Y.A1|Y.A0), big-endian canonical;
 * inf[i] != 0: infinity in, infinity out (flag in out_inf); scalar_be32 < r.  0 on success, -1 on error / hooks disabled. */
extern int gsc_debug_scale_points(int group, const uint8_t *pts, const uint8_t *inf, size_t n,
                                  const uint8_t *scalar_be32, uint8_t *out, uint8_t *out_inf);

/* ---- key ceremony, first phase: the check of a powers file (an addition).  The result of a phase-1 ceremony is a file of
 * group elements in which nobody needs to know tau, alpha or beta.  THIS PROJECT'S OWN FORMAT, version 1 — NOT snarkjs' .ptau and NOT gnark's
 * mpcsetup format (neither can be pinned without those tools; a converter is not part of the library):
 *   "gscsrs01" (8 B) | u32 big-endian L | tauG1[0 .. 2N-2] | tauG2[0 .. N-1] | alphaG1[0 .. N-1] | betaG1[0 .. N-1] | betaG2        N = 2^L
 * tauG1[i] = tau^i G1, tauG2[i] = tau^i G2, alphaG1[i] = alpha tau^i G1, betaG1[i] = beta tau^i G1, betaG2 = beta G2; every element raw (flag
 * bits 00; G1 64 B X | Y, G2 128 B X.A1 | X.A0 | Y.A1 | Y.A0, big-endian), none compressed, none at infinity; 1 <= L <= 24; the length is
 * the one L gives, exactly.
 * gsc_srs_verify accepts a file iff (1) magic, L and length are right and every element is raw, finite, canonical (< p), on the curve and, in
 * G2, in the subgroup; (2) tauG1[0] and tauG2[0] are the generators; with fresh non-zero 128-bit rho_i from the OS CSPRNG, drawn anew for each
 * rule, (3) e(sum rho_i tauG1[i+1], G_2) = e(sum rho_i tauG1[i], tauG2[1]) over i < 2N-2; (4) e(G_1, sum rho_i tauG2[i+1]) = e(tauG1[1],
 * sum rho_i tauG2[i]) over i < N-1; (5) and (6) rule 3's equation over alphaG1 and over betaG1, i < N-1; (7) e(betaG1[0], G_2) = e(G_1, betaG2).
 * A wrong file is accepted with probability about 2^-128.  The check shows that the file is the powers of SOME tau, alpha, beta; it does not
 * show who made the file or that anybody discarded those scalars: that is what a ceremony's contribution records are for
 * (gsc_srs_contribute / gsc_srs_verify_contribution below).
 * 1 accepted, 0 refused (one line on stdout naming the first rule that failed), -3 device error.  Needs no initialised algorithm; runs on
 * GSC_DEVICE, or the first of GSC_DEVICES, and is thread-safe. */
extern int gsc_srs_verify(GoSlice srs);
/* ---- key ceremony, first phase: making a powers file (an addition).  The ceremony starts from the file of tau = alpha =
 * beta = 1 and every party multiplies the scalars by secrets of its own; the final tau, alpha, beta are products that nobody knows unless
 * every party colludes (or kept its secrets).  The full chain to a proving key, with no test hook on the way: gsc_srs_initial ->
 * gsc_srs_contribute (each party; everybody checks every link with gsc_srs_verify_contribution) -> gsc_setup_from_srs ->
 * gsc_setup_contribute (each party; gsc_setup_verify_contribution) and, for a key with a commitment (AES-V2), gsc_setup_contribute_sigma
 * (each party; gsc_setup_verify_sigma_contribution), from the pair everybody checked with gsc_setup_verify_from_srs.
 * The starting file for N = 2^L, 1 <= L <= 24, in the layout above: every G1 element the G1 generator, every G2 element the G2 generator,
 * raw.  Host only (no device, no test hooks) and deterministic: a verifier of a chain makes the start itself and compares the published one
 * byte for byte.  0 on success: *srs malloc'd (release with Free); -2: L out of range, the outputs NULL / 0. */
extern int gsc_srs_initial(int L, void **srs, size_t *len);
/* One contribution.  Draws tau', alpha', beta' in [1, r) and three Schnorr nonces from the OS CSPRNG and writes a file of the same L with
 * tauG1'[i] = tau'^i tauG1[i] (i <= 2N-2), tauG2'[i] = tau'^i tauG2[i], alphaG1'[i] = alpha' tau'^i alphaG1[i], betaG1'[i] = beta' tau'^i betaG1[i]
 * (i < N), betaG2' = beta' betaG2, every element raw.  The input gets rule 1 of gsc_srs_verify (the walk, and every element decoded on the
 * device); the powers are computed on the device and every element is multiplied by its own in a ladder that does not branch on the scalar.
 * The record (GSC_SRS_CONTRIBUTION_BYTES, this project's own format, like the phase-2 record): SHA-256(prev) | SHA-256(next) | then for
 * s = tau, alpha, beta: new_s raw (64; next's tauG1[1] / alphaG1[0] / betaG1[0]) | T_s = k_s base_s raw (64; base_s: prev's element) |
 * z_s = k_s + c_s s' mod r, big-endian (32); c_s = the first 31 bytes, as a big-endian integer, of SHA-256("gsc-phase1-v1" | one byte 0 / 1 / 2
 * for tau / alpha / beta | SHA-256(prev) | base_s raw | new_s raw | T_s raw): three Schnorr proofs that the contributor knows its secrets.
 * With seed32 (TEST HOOKS only) s' = SHA-256("gsc-phase1-tau" | seed32) mod r (and "-alpha", "-beta"), k_s = SHA-256("gsc-phase1-k-tau" |
 * seed32) mod r (likewise).
 * 0 on success: *srs_out malloc'd (release with Free), record filled.  -1: a seed given without test hooks (before a device is asked for);
 * -2: a refused file (one line on stdout names the element) or a seed that gives a zero scalar; -3: device error.  On failure the outputs
 * are NULL / 0, the record is zeroed, nothing stays allocated. */
#define GSC_SRS_CONTRIBUTION_BYTES 544
extern int gsc_srs_contribute(GoSlice srs, const uint8_t *seed32, void **srs_out, size_t *len, uint8_t record[GSC_SRS_CONTRIBUTION_BYTES]);
/* One link (prev, next, record) is accepted iff (1) both files pass the host walk (magic, L, length, raw finite elements) with the same L, and
 * prev's tauG1[1], alphaG1[0], betaG1[0] decode; (2) SHA-256(prev) and SHA-256(next) are the record's; (3) the record's three new elements are
 * next's tauG1[1], alphaG1[0], betaG1[0]; (4) for s = tau, alpha, beta: z_s < r, T_s a finite raw G1 point, z_s base_s == T_s + c_s new_s (the
 * line names s); (5) next passes all of gsc_srs_verify, rules 1-7 (the line carries the inner rule: "rule 5: next: rule 3: ...").  Rules 4
 * and 5 together: next holds the powers of (tau tau', alpha alpha', beta beta') with tau', alpha', beta' known to the contributor.
 * PREV IS DELIBERATELY NOT CHECKED IN FULL: a chain is verified from the bytes of gsc_srs_initial(L), link by link, and each prev is the next
 * of the link before it (which rule 5 checked); a verifier who starts in the middle runs gsc_srs_verify on its first prev itself.
 * 1 accepted, 0 refused (one line on stdout, "gsc_srs_verify_contribution: rule k: ...", naming the first rule that failed), -3 device error. */
extern int gsc_srs_verify_contribution(GoSlice prev, GoSlice next, const uint8_t record[GSC_SRS_CONTRIBUTION_BYTES]);
/* TEST HOOK: out[i] = m x^(first + i) pts[i] through the kernels and the launcher a contribution uses (k_fr_powers, the per-point ladder).
 * Conventions and refusals as gsc_debug_scale_points; x_be32, m_be32 < r.  0 on success, -1 on error / hooks disabled. */
extern int gsc_debug_scale_powers(int group, const uint8_t *pts, const uint8_t *inf, size_t n, const uint8_t *x_be32, const uint8_t *m_be32,
                                  uint64_t first, uint8_t *out, uint8_t *out_inf);
/* Groth16 Setup from a powers file: an ordinary gnark pk / vk (compressed points) for the R1CS, made from the file's group elements alone — no
 * tau, alpha or beta is known to this call.  The Lagrange bases at tau, the column sums A_i(tau), B_i(tau), K_i and the Z_k are computed in the
 * groups, on the device.  The call first runs gsc_srs_verify's whole check on the file.  A larger file serves a smaller circuit: with
 * L > log2 n (n: the circuit's domain size, as gsc_setup computes it) the first 2n-1 / n elements are used.
 * seed32 == NULL (the only mode a production host reaches): gamma = delta = 1, i.e. G1.Delta, G2.Delta and G2.Gamma are the generators.
 * A KEY WITH DELTA = 1 IS FORGEABLE BY ANYONE.  It becomes usable only after at least one gsc_setup_contribute; a deployment verifies the file
 * (gsc_srs_verify) and every link of the chain (gsc_setup_verify_contribution).  Without a commitment (ChaCha20-V3) the key is a deterministic
 * function of (r1cs, file).  With one (AES-V2) the Pedersen sigma and g come from the OS CSPRNG and are wiped before the call returns:
 * whoever runs this call held sigma for that moment, so sigma is re-randomised like delta: gsc_setup_contribute_sigma (each party;
 * gsc_setup_verify_sigma_contribution), from a pair that gsc_setup_verify_from_srs accepts.  Public committed wires are refused, as by gsc_setup.
 * seed32 != NULL (TEST HOOKS only): gamma, delta, sigma, g = gsc_setup's seeded scalars, applied to the unscaled points, so that the result
 * equals gsc_setup(r1cs, seed32) byte for byte when the file holds the same seed's tau, alpha, beta (gsc_debug_srs_generate).
 * 0 on success: *pk / *vk malloc'd (release with Free).  -1: a seed given without test hooks; -2: malformed r1cs, a file that gsc_srs_verify
 * refuses, or L < log2 n (one line on stdout); -3: device error.  On failure the outputs are NULL / 0 and nothing stays allocated. */
extern int gsc_setup_from_srs(GoSlice r1cs, GoSlice srs, const uint8_t *seed32, void **pk, size_t *pk_len, void **vk, size_t *vk_len);
/* ---- key ceremony: the Pedersen sigma of a commitment key, distributed (an addition).  A key with a BSB22 commitment
 * (AES-128-V2, AES-256-V2) carries pk.Basis_j = K_j / gamma over the committed wires, pk.BasisExpSigma_j = sigma Basis_j, vk.G = g G_2,
 * vk.GSigmaNeg = -sigma g G_2.  Whoever knows sigma forges the proof of knowledge PoK = sigma D of a commitment D it cannot open: sigma is
 * toxic waste like delta.  The PEDERSEN RELATION of a pair: e(BasisExpSigma_j, G) e(Basis_j, GSigmaNeg) = 1 for every j.
 * A sigma contribution draws a secret x in [1, r) and makes BasisExpSigma'_j = x BasisExpSigma_j (pk) and GSigmaNeg' = x GSigmaNeg (vk): the
 * key of sigma x.  Every other byte of both files is copied (G too: the relation is homogeneous in g, and g's discrete logarithm opens
 * nothing); the rewritten points are written compressed, infinity stays infinity.  A delta contribution copies the commitment key and a
 * sigma contribution copies delta, Z and K: THE TWO KINDS OF LINK MAY INTERLEAVE IN ONE CHAIN.
 * The record (GSC_SIGMA_CONTRIBUTION_BYTES, this project's own format, the phase-2 record's layout): SHA-256(pk_prev) | SHA-256(pk_next) |
 * new raw X | Y (next's BasisExpSigma[j0]; j0: the lowest index whose element is finite) | T = k base raw (base: prev's BasisExpSigma[j0]) |
 * z = k + c x mod r, big-endian; c = the first 31 bytes, as a big-endian integer, of SHA-256("gsc-sigma-v1" | SHA-256(pk_prev) | base raw |
 * new raw | T raw).  The tag is not phase 2's: a delta record never passes as a sigma record.
 * x and k come from the OS CSPRNG; with seed32 (TEST HOOKS only) x = SHA-256("gsc-sigma-x" | seed32) mod r, k = SHA-256("gsc-sigma-k" | seed32) mod r.
 * None of the four calls needs an initialised algorithm; all run on GSC_DEVICE, or the first of GSC_DEVICES, and are thread-safe; every
 * refusal prints one line, "<function>: rule k: ...", on stdout. */
#define GSC_SIGMA_CONTRIBUTION_BYTES 224
/* Does the pair hold the Pedersen relation?  (1) both files parse, each holds exactly one commitment key ("no commitment key" otherwise), every
 * point of both decodes as for InitAlgorithm / gsc_verify_init (canonical, on the curve, G2 in the subgroup), G and GSigmaNeg are finite, Basis
 * and BasisExpSigma have the same length and their infinities at the same positions, at least one element is finite; (2) with fresh non-zero
 * 128-bit rho_j from the OS CSPRNG, e(sum rho_j BasisExpSigma_j, G) = e(-sum rho_j Basis_j, GSigmaNeg).  A wrong pair is accepted with
 * probability about 2^-128.  1 accepted, 0 refused, -3 device error. */
extern int gsc_pedersen_verify(GoSlice pk, GoSlice vk);
/* One sigma contribution.  0 on success: *pk_out / *vk_out malloc'd (release with Free), record filled.  -1: seed given without test hooks
 * (before the keys are looked at or a device is asked for); -2: a key that does not parse, has no commitment key or fails rule 1 of
 * gsc_pedersen_verify, or a seed that gives a zero scalar; -3: device error.  On failure the outputs are NULL / 0, the record is zeroed,
 * nothing stays allocated. */
extern int gsc_setup_contribute_sigma(GoSlice pk, GoSlice vk, const uint8_t *seed32,
                                      void **pk_out, size_t *pk_len, void **vk_out, size_t *vk_len,
                                      uint8_t record[GSC_SIGMA_CONTRIBUTION_BYTES]);
/* One link (prev, next, record) is accepted iff (1) rule 1 of gsc_pedersen_verify holds on both pairs; (2) outside pk's BasisExpSigma and vk's
 * GSigmaNeg next equals prev BYTE FOR BYTE with the same counts (Basis, G, delta, Z, K untouched; a re-encoded key is refused); (3) the
 * record's hashes are the files', BasisExpSigma has its infinities at the same positions in prev and next (for next this is rule 1's clause
 * on the infinities, reported here), new is next's element at j0; (4) z < r, T is a finite raw point of the curve, z base == T + c new;
 * (5) rule 2 of gsc_pedersen_verify holds on NEXT.  Rule 5 makes next the key of some sigma''; rule 4 makes BasisExpSigma'[j0] a multiple x,
 * known to the contributor, of prev's; given the relation on prev, sigma'' = x sigma.
 * PREV'S RELATION IS DELIBERATELY NOT RE-CHECKED: a chain is verified from a start pair that passed gsc_pedersen_verify or
 * gsc_setup_verify_from_srs, link by link, and each prev is the next of the link before it (which rule 5 checked); a verifier who starts in
 * the middle runs gsc_pedersen_verify on its first prev itself.
 * 1 accepted, 0 refused (the line names the first rule that failed), -3 device error. */
extern int gsc_setup_verify_sigma_contribution(GoSlice pk_prev, GoSlice vk_prev, GoSlice pk_next, GoSlice vk_next,
                                               const uint8_t record[GSC_SIGMA_CONTRIBUTION_BYTES]);
/* Is (pk, vk) what gsc_setup_from_srs makes of (r1cs, srs)?  Runs that call's production path (no seed) and accepts iff (1) the given pair
 * equals the recomputed one byte for byte outside pk's BasisExpSigma and vk's G and GSigmaNeg (every run draws sigma and g afresh; for a circuit
 * without a commitment that is the whole of both files); (2) with a commitment, rules 1 and 2 of gsc_pedersen_verify hold on the given pair.
 * The start of a verified chain for every algorithm.  1 accepted, 0 refused (with the rule), -2 malformed r1cs, a file gsc_srs_verify
 * refuses, or L < log2 n; -3 device error. */
extern int gsc_setup_verify_from_srs(GoSlice r1cs, GoSlice srs, GoSlice pk, GoSlice vk);
/* TEST HOOK: the powers file for tau, alpha, beta = gsc_setup's seeded toxic(seed32, "tau" | "alpha" | "beta"), 1 <= L <= 20: whoever holds
 * the seed holds the scalars.  0 on success: *srs malloc'd (release with Free); -1 on error / hooks disabled, outputs NULL / 0. */
extern int gsc_debug_srs_generate(int L, const uint8_t *seed32, void **srs, size_t *len);
/* TEST HOOK: the group transform that turns powers of tau into the Lagrange basis at tau, out[j] = (1/n) sum_k w^(-jk) pts[k] over n = 2^L raw
 * finite points (group 0: G1, 64 B; 1: G2, 128 B), w the generator of gsc_setup's domain of size n; natural order in and out; out_inf[j] = 1
 * (and zeros) for the point at infinity.  1 <= L <= 17.  0 on success, -1 on error / hooks disabled. */
extern int gsc_debug_group_idft(int group, int L, const uint8_t *pts, uint8_t *out, uint8_t *out_inf);
/* TEST HOOK: the column sums of a sparse matrix over group elements, out[w] = sum over the terms t in [col_start[w], col_start[w+1]) of
 * coeff[term_coeff[t]] * rows[term_row[t]], with the kernel's cut of long columns into segments.  rows: n_rows raw finite points of the group;
 * col_start: n_cols + 1 offsets; coeff_be: n_coeff scalars below r, 32 big-endian bytes each; out_inf[w] = 1 for the point at infinity (an
 * empty column, terms that cancel).  0 on success, -1 on error (a row that is not a finite point, an index out of range) / hooks disabled. */
extern int gsc_debug_column_sums(int group, uint32_t n_rows, const uint8_t *rows, uint32_t n_cols, const uint32_t *col_start,
                                 const uint32_t *term_row, const uint32_t *term_coeff, uint32_t n_coeff, const uint8_t *coeff_be,
                                 uint8_t *out, uint8_t *out_inf);
/* TEST HOOK: the MSM kernels alone, on a caller's bases and scalars: no key, no circuit, no witness.  The bases are laid out by the planner the
 * engine uses for a key's sets (csrc/msm_layout.hpp) from the caller's per-base description, the tables are built, and one sum per column runs
 * through the launch sequence of a prover's MSM, the function the engine calls (msm_run, csrc/msm_set.hpp): recoding, gather-accumulate (flat and
 * windowed part), slice reductions, Horner.
 *   group 0: G1 (64 B per point), 1: G2 (128 B, A1 before A0); points: nbases raw finite points, big-endian X | Y;
 *   kind[k]: 0 bit, 1 narrow with rowlen[k] table entries (1 .. 32768), 2 wide; rows[k] < n_rows: the scalar row of base k; zero_row: a row of zeros
 *   (padding slots);  c in [4, 17]: digit width of the windowed part;  cv: 0 = wide bases take the windowed kernel, 4 .. 15 = every wide base becomes
 *   window octets of the flat part at that width;  mont: the kernels get Montgomery images (wire values, sign-normalised) or canonical integers —
 *   canonical ones only where the engine passes them: no bit and no narrow bases;
 *   batch: 64 or 128 columns;  nproofs: 0 = batch kernels, 1 .. 32 = latency kernels on the first nproofs columns;
 *   per_flat / per_win: bases per slice (multiples of 8, flat at most 512), 0 = the engine's own choice (per_flat is not read by the latency kernels);
 *   digit_bases: 0, or more than the wide bases: the windowed digits are laid out for digit_bases bases with the scalar rows digit_rows[0 .. digit_bases)
 *   (its first entries the wide bases' own rows), of which the kernel walks the wide bases only;
 *   scalars_be: n_rows x batch canonical values below r, 32 big-endian bytes each, [row][column];
 *   plane (optional): byte plane [(column / 64 * plane_stride + row) * 64 + column % 64] for the rows below plane_rows <= plane_stride: 0, 1, -1, or
 *   -128 = read the row's 32-byte scalar after all.
 * Outputs: out / out_inf: per column (batch, or nproofs) the affine sum as canonical little-endian values (G1 x, y; G2 x.a0, x.a1, y.a0, y.a1) and 1
 * (with zeros) for the point at infinity;  flat_digits, win_digits (16-byte words as the kernels store them), gok, group_ok: copies of the recoders'
 * output, each with its capacity in bytes (a buffer may be NULL with capacity 0: not copied; too small a buffer is refused);
 * info[64]: 0 nflat, 1 nbit, 2 nexpanded, 3 nwide, 4 nwin, 5 / 6 slices and bases per slice of the flat part, 7 / 8 of the windowed part,
 * 9 reduction levels of the flat part, 10 + 2 i / 11 + 2 i slices entering level i and 1 when it took the by-proof kernel (i < 8), 26 and 27 .. 42 the
 * same for the windowed part, 43: Horner had an addend, 44 columns returned, 45 flat octets, 46 octets per window of the windowed digits, 47 cv,
 * 48 .. 51 bytes written to flat_digits, win_digits, gok, group_ok.
 * 0 on success; -1 (one line on stdout) for hooks disabled, an unknown group, c / cv / batch / nproofs / per outside the above, a scalar not below r,
 * a point that is not raw, finite and in the group, canonical scalars with bit or narrow bases, more than 2^16 bases or 2^28 table entries. */
struct gsc_debug_msm_args {
    int32_t group; uint32_t nbases;
    const uint8_t *points; const uint8_t *kind; const uint32_t *rowlen; const uint32_t *rows;
    uint32_t n_rows, zero_row;
    int32_t c, cv, mont;
    uint32_t batch, nproofs, per_flat, per_win, digit_bases;
    const uint32_t *digit_rows;
    const uint8_t *scalars_be;
    const int8_t *plane; uint32_t plane_rows, plane_stride;
    uint8_t *out, *out_inf;
    uint8_t *flat_digits; size_t flat_digits_cap;
    uint8_t *win_digits; size_t win_digits_cap;
    uint8_t *gok; size_t gok_cap;
    uint8_t *group_ok; size_t group_ok_cap;
    uint32_t *info;
};
extern int gsc_debug_msm(const struct gsc_debug_msm_args *args);
/* TEST HOOK: the proof assembly kernels alone, on a caller's MSM sums and scalars: no key, no circuit, no InitAlgorithm.  Every sum is given as an
 * affine point, an infinity byte and a scale l != 0 per column and reaches the kernels as the XYZZ image (x l^2, y l^3, l^2, l^3), four zeros for the
 * point at infinity.  The production launchers then run in the prover's order: flags zeroed over their padded words; launch_prep_rs; with a
 * commitment launch_points_to_affine_be (D, bit 8) and launch_challenge_from_point; launch_fin_scalarmul, or launch_fin_scalarmul_few on the halves
 * glv_split returns on the host; launch_points_to_affine_be (Pok, bit 16); launch_fin_combine.
 *   batch: 1 .. 256 columns;  nproofs: 0 = the batch kernel, 1 .. 32 (<= batch) = the latency kernel on the first nproofs columns (tmp keeps the stride
 *   batch; k_fin_combine runs over the whole batch either way, with tmp = infinity in the columns the latency kernel left alone);
 *   n_wires (<= 4096): k_prep_rs writes its four rows behind that many rows of W;  fill: the byte out, W, mask_out, commit and cpts hold before the
 *   first kernel;
 *   x_pts: batch raw points, big-endian X | Y (64 B; B2: 128 B, X.A1 | X.A0 | Y.A1 | Y.A0), not read where x_inf[column] != 0;  x_lam: batch scales,
 *   32 B big-endian (B2: 64 B, A1 | A0), non-zero and below p.  A, B1, K, Z in G1 and B2 in G2 are required;  C: all three NULL = the launcher gets
 *   no sumC (the coefficient route);  D and Pok: both given = the commitment part runs, both NULL = it does not;
 *   rs: batch x 64 bytes, r then s, eight little-endian words each, below r;  mask: NULL, or batch x 32 bytes little-endian, below r;
 *   glv_in: NULL = the latency kernel gets glv_split's halves of rs, as a prover's call does.  Otherwise (nproofs != 0) 2 x nproofs records laid out
 *   like the output glv, which the kernel gets INSTEAD: any magnitudes below 2^130 and any neg, the kernel's own contract, of which glv_split's
 *   results are a part (its k1 is never negative and its magnitudes stay below 2^128).  k_prep_rs still reads rs.
 * Outputs: out: batch x 256 bytes (Ar x | y, Bs x.a0 | x.a1 | y.a0 | y.a1, Krs x | y: canonical, eight little-endian words each);  flags: one byte per
 * column (1 Ar, 2 Bs, 4 Krs, 8 D, 16 Pok at infinity);  tmp: 2 x batch x 64 bytes, tmp[0] = s A then tmp[1] = r B1 as canonical little-endian x | y, with
 * tmp_inf[2 x batch] = 1 (and zeros) for the point at infinity;  cpts: D at column x 64, Pok at (batch + column) x 64, as stored;  commit, mask_out: one
 * value per column as stored (eight little-endian Montgomery words);  W: the four rows r, s, -r s, 0 as stored, [row][column];  glv: 2 x nproofs
 * records of 44 bytes (k1[5], k2[5], neg; [column][s, r]) as the kernel got them.
 * 0 on success; -1 (one line on stdout): hooks disabled, batch / nproofs / n_wires / fill outside the above, a scalar or mask not below r, a scale
 * that is zero or not below p, a missing buffer, glv_in without nproofs or with a magnitude of 2^130 or more or neg above 3, a point that is not raw, finite, on the curve and in the group. */
struct gsc_debug_assemble_args {
    uint32_t batch, nproofs, n_wires, fill;
    const uint8_t *a_pts, *a_inf, *a_lam;
    const uint8_t *b1_pts, *b1_inf, *b1_lam;
    const uint8_t *k_pts, *k_inf, *k_lam;
    const uint8_t *z_pts, *z_inf, *z_lam;
    const uint8_t *b2_pts, *b2_inf, *b2_lam;
    const uint8_t *c_pts, *c_inf, *c_lam;
    const uint8_t *d_pts, *d_inf, *d_lam;
    const uint8_t *pok_pts, *pok_inf, *pok_lam;
    const uint8_t *rs; const uint8_t *mask; const uint8_t *glv_in;
    uint8_t *out, *flags, *tmp, *tmp_inf, *cpts, *commit, *W, *mask_out, *glv;
};
extern int gsc_debug_assemble(const struct gsc_debug_assemble_args *args);
/* TEST HOOK: the evaluation-form quotient kernels alone on the routes a batch call takes (csrc/k_ntt.hip: byte planes with and without the
 * plain-integer first stages, the digits recoded inside the last kernel, a few columns, live tiles), 64 independent columns, on the first lane of
 * a loaded algorithm and with that algorithm's own transform tables, the plain-integer ones included.
 *   algorithm: 0 .. 2, initialised;  mats_be: a, then b, each [m][64] canonical big-endian 32-byte values;  m: rows, up to the DOMAIN size n (rows
 *   m .. n-1 count as zero: the hook fills them with 0xFF bytes, the kernels must not read them);
 *   planes: NULL, or the byte planes of a and then b, [n][64] each: an entry 0, 1 or -1 stands for that value, -128 says the row's value is the
 *   one in mats_be; rows >= m may hold anything.  Where an entry is not -128 the value in mats_be is not read;
 *   plain: 0 or 1, handed to the launcher as NttNarrow::plain unchanged, with planes or (null plane pointers) without: launch_quotient itself clears
 *   it where its rule says so, e.g. without both planes, and the call then takes the generic route;
 *   ncols: 0 = every column, else only the first ncols columns (rounded up to 4) are transformed, c = 0 only;
 *   live: 0 = every table position, else only the positions below live are produced (kernels.hpp quot_live_tiles), the rest of out is leftovers
 *   (c = 0) or zero (c > 0);
 *   c: 0 = launch_compute_d, out = [n][64] canonical little-endian values, row i = A(zeta w^i) B(zeta w^i) 2^261 mod r;
 *      4 .. 17 = launch_compute_d_digits with msm_windows(c) windows into a buffer of the hook's own, out = that buffer as the kernel wrote it:
 *      16-byte words, word (j * n/8 + octet) * 64 + column (c = 17: two words, at twice that index) holds the digits of window j of the table
 *      positions 8 octet .. 8 octet + 7 (position t = index quot_digit_index(L, t)) as int16 (c = 17: int32);
 *   out / cap: the output and its capacity in bytes: n * 64 * 32 for c = 0, windows * n/8 * 64 * 16 (c = 17: * 32) otherwise.
 * Returns the domain size n (also with out == NULL: size query); -1 (one line on stdout) for hooks disabled, an algorithm that is not loaded,
 * m or live above n, ncols above 64 or with c > 0, c or plain outside the above, a plane entry below row m that is none of the four, too small a cap. */
struct gsc_debug_quotient_args {
    uint32_t algorithm; int32_t plain, c;
    const uint8_t *mats_be; size_t m;
    const int8_t *planes;
    size_t ncols, live;
    uint8_t *out; size_t cap;
};
extern long long gsc_debug_quotient(const struct gsc_debug_quotient_args *args);
/* TEST HOOK: the witness solver kernels alone, on a caller's constraint system: a device, but no key and no InitAlgorithm.  The description is an
 * R1CS file given field by field, exactly what the parser would have produced; the tables are built and uploaded by the functions InitAlgorithm
 * uses (csrc/solver_tables.hpp: build_solver_program, build_few_program, the count tables' device check, coeff / coeff_inv, build_small_program) and
 * the levels run through the engine's own loops (solver_run_levels, solver_run_small).
 *   n_public (wire 0 included), n_secret, n_internal, n_constraints;
 *   calldata: n_calldata words, every instruction's first word its own length (the boundaries are derived from it); blueprint / constraint_off /
 *   wire_off: one word per instruction (n_instr of them);  bp_kind[b]: 0 hint, 1 r1c, 2 lookup;  bp_entries: the EntriesCalldata words of the
 *   blueprints one after the other, bp_entries_len[b] of them for blueprint b (256 x 3 for a lookup, 0 otherwise);
 *   coeff: n_coeff x 8 little-endian 32-bit limbs, Montgomery, ids 0..4 being 0, 1, 2, -1, -2;  has_commitment, commit_wire, commit_private;
 *   in_W: the rows of the public and secret wires, [wire][column], 8 Montgomery limbs each, used as given (the caller sets wire 0);
 *   mask / commit: one Montgomery value per column for the Randomize / commitment hints, or NULL (zero);
 *   batch: columns, a multiple of 64 up to 4096;  nproofs: 0 = the batch kernels on every column, 1 .. 32 = the resident kernels on the first
 *   nproofs columns (batch = 64);  workgroups: the resident grid, 0 = the engine's choice, always clamped to the device's compute units;
 *   mode: 0 = generic solver, 1 = small-integer path (nproofs = 0) from the class predictions class_w[n_wires], class_a / class_b / class_c
 *   [n_constraints] (0 = bit, 1 = also -1, more = wide);  fill: the byte W (but its input rows), A, B and C hold before the first kernel.
 * Outputs: W (n_wires rows), A, B, C (n_constraints rows) as stored: [row][column], 8 Montgomery limbs, with their capacities in bytes; status[batch]
 * (0xFFFFFFFF: satisfied); flag: the small path's misprediction word; why[128]: SmallProgram::why or the refusing builder's text;
 * info[32]: 0 levels, 1 commit_level, 2 has_div, 3 ops, 4 WPB of the batch launches (0: none), 5 resident workgroups used, 6 resident launches,
 * 7 a resident launch gave up at a barrier (the call still returns 0 with what it has), 8 the small program qualified, 9 levels with long ops,
 * 10 count levels, 11 the largest level_long, 12 / 13 the small chain's levels and the bundles of its widest level (16 waves share them),
 * 14 + l for l < 18: level l as kind | level_long << 1 | width << 12.
 * 0 on success; -1 (one line on stdout): hooks disabled, a description the builders refuse, an index out of range, a buffer too small, a batch or
 * nproofs outside the above; -2: mode 1 and the circuit does not qualify (why says why); -3: a device error. */
struct gsc_debug_solve_args {
    uint32_t n_public, n_secret, n_internal, n_constraints;
    const uint32_t *calldata; uint32_t n_calldata;
    const uint32_t *blueprint, *constraint_off, *wire_off; uint32_t n_instr;
    const uint8_t *bp_kind; const uint32_t *bp_entries; const uint32_t *bp_entries_len; uint32_t n_blueprints;
    const uint32_t *coeff; uint32_t n_coeff;
    int32_t has_commitment; uint32_t commit_wire; const uint32_t *commit_private; uint32_t n_commit_private;
    const uint32_t *in_W; const uint32_t *mask; const uint32_t *commit;
    uint32_t batch, nproofs, workgroups; int32_t mode;
    const uint8_t *class_w, *class_a, *class_b, *class_c;
    uint32_t fill;
    uint32_t *W; size_t W_cap;
    uint32_t *A; size_t A_cap;
    uint32_t *B; size_t B_cap;
    uint32_t *C; size_t C_cap;
    uint32_t *status; uint32_t *flag; uint32_t *info; char *why;
};
extern int gsc_debug_solve(const struct gsc_debug_solve_args *args);
/* TEST HOOK: the verifier's G1 stage alone, everything between a proof's bytes and the first Miller loop, on a caller's key, proofs and
 * randomizers.  The hook builds a key of its own with the verifier's build_key (chunk buffers for n proofs; the loaded keys are not touched),
 * runs prep_chunk (the host pre-check, the public-input windows, k_verify_prep), then launch_verify_batch on the caller's randomizers and, with
 * parts, launch_verify_claims, and reads back what they left behind.  The randomizer mode of gsc_debug_verify_randomizers is neither read nor
 * changed.
 *   algorithm: 0 .. 2;  vk / vk_len: the key's bytes, either point encoding;  n: 1 .. 8192 proofs in 196-byte slots with lens[n] and
 *   n x 144 signal bytes;  rnd: n x 8 words, rho (four little-endian words) then t, used as given;  np / ends: 0, or np part ends, strictly
 *   increasing, the last one n (part j = proofs [ends[j-1], ends[j]));  path: 1 the per-thread Miller kernels, 2 the few-proof ones;
 *   fill: the byte every output holds before the first kernel.
 * A G1 point is 65 bytes, canonical big-endian X | Y and an infinity byte (1: infinity, coordinates zero); a G2 point 129 bytes, X.A1 | X.A0 | Y.A1 |
 * Y.A0 and the byte.  Outputs (each may be NULL):
 *   key_status: one int8 per key point as k_verify_key_points left it (0 finite, 1 infinity), alpha, beta1, delta1, K ..., then beta, gamma, delta
 *   (ped_g, ped_gsn) in G2: key_status_cap entries at most;
 *   table: 144 x 256 G1 points, the public-input window tables;  ctable: 32 x 256 (a key with a commitment; else left alone);
 *   ok: n bytes, ProofDev::ok;  g1: n x 6 G1 points A, C, L, D, PoK, rho A (the first five left alone for a proof without ok, D also for a key
 *   without a commitment);  g2: n G2 points B (left alone without ok);  okv: n bytes, the batched check's;
 *   fixed: 5 G1 points, the chunk's fixed pairs;  flag: the chunk's byte;
 *   pfixed: np x 5 G1 points (the Pedersen pairs left alone for a key without a commitment);  prho: np x 5 words, the part's sum of rho;
 *   pflag: np bytes.
 * 0 on success; -1 (one line on stdout): hooks disabled, an argument outside the above, a device error; -2: the key is refused (it does not
 * parse, or a point of it does not decode); -3: the key is not one of the algorithm's circuit.  Nothing is written unless 0 is returned. */
struct gsc_debug_verify_g1_args {
    uint32_t algorithm, path, fill;
    const uint8_t *vk; size_t vk_len;
    size_t n; const uint8_t *proofs; const uint32_t *lens; const uint8_t *signals; const uint32_t *rnd;
    size_t np; const uint64_t *ends;
    int8_t *key_status; size_t key_status_cap;
    uint8_t *table, *ctable, *ok, *g1, *g2, *okv, *fixed, *flag, *pfixed; uint32_t *prho; uint8_t *pflag;
};
extern int gsc_debug_verify_g1(const struct gsc_debug_verify_g1_args *args);

#ifdef __cplusplus
}
#endif
#endif
