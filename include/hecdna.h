/*
 * hecdna.h — C-ABI of the MI355X-native CKKS homomorphic linear-algebra engine.
 *
 * This is the drop-in boundary for the reference's hot path
 * (isteiakakis/Homomorphic-Encryption-Algorithms-Diploma-Thesis):
 * every arithmetic step of he::linalg / he::operators goes through a seal::Evaluator member call;
 * each entry point below replaces one of those calls (reference file:line cited per function) and
 * keeps its argument meaning, data layout and error behaviour:
 *
 *   - data layout = SEAL layout: a ciphertext is u64[size][level][N] in NTT form, a plaintext
 *     u64[level][N] in NTT form, a key-switching key (one RelinKeys / GaloisKeys entry, i.e. SEAL's
 *     vector<PublicKey>) u64[L][2][K][N], where K = #coeff_modulus, L = K-1 data primes and
 *     "level" = number of data primes a ciphertext currently has (SEAL chain index + 1);
 *   - all residues canonical in [0, q); every result is bit-identical to this repository's CPU
 *     restatement of SEAL 4.1's Evaluator (oracle/).  Against SEAL itself parity is unpinned:
 *     SEAL is absent here and the reference ships no test vectors;
 *   - errors: SEAL throws std::invalid_argument / std::logic_error; here every call returns a
 *     status (HEC_OK, HEC_EINVAL for invalid_argument, HEC_ELOGIC for logic_error, HEC_EDEVICE for a
 *     HIP failure) and hec_last_error() returns SEAL's message text ("scale mismatch",
 *     "Galois key not present", "end of modulus switching chain reached", ...).
 *
 * Objects are device-resident on the context's GPU; every call is ordered on the context's HIP
 * stream (hec_context_set_stream), downloads synchronise.  One context per device, one host
 * thread per context.  A matvec runs its whole batch on the context's stream by default (one lane); the
 * option "lanes" > 1 (HEC_LANES) splits a batch of >= 32 vectors into concurrent lanes on engine-owned threads
 * and streams, joined before it returns (opt-in).  No torch types cross this boundary.
 */
#ifndef HECDNA_H
#define HECDNA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HEC_OK 0
#define HEC_EINVAL 1
#define HEC_ELOGIC 2
#define HEC_EDEVICE 3

typedef struct hec_context hec_context;
typedef struct hec_ciphertext hec_ciphertext;
typedef struct hec_plaintext hec_plaintext;
typedef struct hec_kswitch_key hec_kswitch_key; /* one KSwitchKeys entry: RelinKeys[0] */
typedef struct hec_galois_keys hec_galois_keys; /* GaloisKeys: galois_elt -> key */
typedef struct hec_secret_key hec_secret_key;   /* seal::SecretKey: u64[K][N], NTT form, key level */

const char *hec_last_error(void);
int hec_version(void);

/* ---------------------------------------------------------------- parameters / context ---- */
/* seal::CoeffModulus::Create(N, bit_sizes) — used at reference matrix_operations.cpp:1050 */
int hec_create_coeff_modulus(uint64_t poly_modulus_degree, const int *bit_sizes, uint64_t count, uint64_t *out);
/* seal::SEALContext(EncryptionParameters{ckks, N, coeff_modulus}) — matrix_operations.cpp:1047-1051.
 * coeff_modulus[K-1] is the special (key) prime.  device = HIP device ordinal. */
int hec_context_create(uint64_t poly_modulus_degree, const uint64_t *coeff_modulus, uint64_t K, int device,
                       hec_context **out);
/* Objects (ciphertexts, plaintexts, keys) may be destroyed before or after their context, in any order, as SEAL's
 * objects holding their context by shared_ptr allow: an object destroyed after its context frees its own device
 * memory and touches nothing else.  The destroys (of objects and of contexts) may run on any thread, concurrently
 * with each other, as a garbage collector's finalisers do; every other call on a context and its objects comes from
 * one host thread at a time.  A call on an object whose context is gone fails with HEC_EINVAL and the object kind's
 * "... is not valid for encryption parameters" message.  A handle is never valid for a later context, even one
 * created at the destroyed context's address: such a call fails the same way. */
int hec_context_destroy(hec_context *ctx);
int hec_context_set_stream(hec_context *ctx, void *hip_stream); /* NULL = context-owned stream */
int hec_context_synchronize(hec_context *ctx);
/* Engine knobs at run time (no SEAL counterpart; the HEC_* environment switches of DESIGN.md §4.1 set the
 * same knobs at context creation): "lanes", "lane_min_batch", "hoist", "hoist_min", "hmac", "hmac_odd3",
 * "hoist_scan", "fan", "fuse_galois", "fused_modup_mac", "tensor_defer", "tensor_bufs", "tensor_xcd",
 * "split_bfly", "bmac_split", "nttb_shfl" (the forward pass B at 128 points with its exchanges as DPP lane moves
 * instead of LDS: 1, 16 outputs per lane; 2, swapped back for coalesced stores), "nttb_shfl_dr" (the same for the
 * divide-and-round pass B), "moddown1" (the single-pass mod-down at N = 2^15), "hmac_int" (0: the 60-bit hoisted MAC
 * targets on the round-5 loop), "nt_e" (0: the hoisted digits stored with the default cache policy instead of
 * non-temporally), "mac_divround" (1: the per-rotation key switch accumulates the special-prime target first and the
 * data targets' fused MAC kernel divides-and-rounds its own accumulators; 0: the separate divide-and-round pass B;
 * HEC_MAC_DIVROUND at context creation, HEC_EINVAL when out of range), "hmac_divround" (1: the same order for the
 * children of a hoisted node, a sibling group at a time: the hoisted MAC kernel's data targets divide-and-round their
 * accumulators into the children's rotation buffers; 0: the separate pass B; HEC_HMAC_DIVROUND at context creation,
 * HEC_EINVAL when out of range; applies with "hmac" 2, "hmac_int" 1 and "fan" 1), "kernel_memops" (0: workspace fills and
 * device copies through the runtime's hipMemsetAsync / hipMemcpyAsync instead of engine kernels; A/B only,
 * DESIGN.md §4.8), "prng_group" (0..16: PRNG buffers per wavefront of the key generator's BLAKE2Xb kernel, 0 = chosen per
 * launch; every value draws the same words), and three debug switches:
 * "poison" (every workspace carve and fresh output buffer is filled with 0xFF bytes before use, so a read of
 * memory the call never wrote becomes a deterministic wrong result), "lane_serial" (batch lanes run one after
 * another) and "debug_lanes" (per-call zero-list and key-table reports on stderr).  Every schedule is
 * bit-identical.  Applies to the context and its batch lanes; HEC_EINVAL for an unknown name, and for a value
 * outside an enumerated knob's range ("split_bfly" 0..4, "hmac" 0..2, "hmac_odd3" 0..1, "hoist_scan" 0..1,
 * "nttb_shfl" 0..2, "nttb_shfl_dr" 0..1, "moddown1" 0..1, "hmac_int" 0..1, "nt_e" 0..1,
 * "mac_divround" 0..1, "hmac_divround" 0..1, "prng_group" 0..16, "rot_add" 0..1).  "math_chunk" (0..65535) caps the ciphertexts per pass
 * of the he::math calls and of hec_multiply_relin_rescale_many / hec_sum_elems_many below; 0 is automatic, a negative
 * value HEC_EINVAL.  "rot_add": 1 the rotate-and-accumulate steps of hec_sum_elems_many add the accumulator in the
 * key switch's last stage (k_bmac's divide-and-round epilogue, k_moddown1), 0 in a k_ew_add launch after it. */
int hec_context_set_option(hec_context *ctx, const char *name, int64_t value);
uint64_t hec_context_poly_degree(const hec_context *ctx);
uint64_t hec_context_key_moduli(const hec_context *ctx); /* K */
/* seal::GaloisTool::get_elt_from_step (rotation step -> Galois element); 0 on error */
uint32_t hec_galois_elt_from_step(const hec_context *ctx, int step);
/* seal::GaloisTool::get_elts_all — the set KeyGenerator::create_galois_keys() makes
 * (matrix_operations.cpp:1063-1064).  Returns the count; writes it when out != NULL. */
uint64_t hec_default_galois_elts(const hec_context *ctx, uint32_t *out);

/* ---------------------------------------------------------------- ciphertext / plaintext -- */
int hec_ciphertext_create(hec_context *ctx, hec_ciphertext **out);
int hec_ciphertext_destroy(hec_ciphertext *ct);
/* host SEAL-layout buffer u64[size][level][N] -> device */
int hec_ciphertext_upload(hec_ciphertext *ct, const uint64_t *host, uint64_t size, uint64_t level, double scale);
/* device -> host (synchronises); host must hold size*level*N words */
int hec_ciphertext_download(const hec_ciphertext *ct, uint64_t *host);
int hec_ciphertext_info(const hec_ciphertext *ct, uint64_t *size, uint64_t *level, double *scale);
int hec_ciphertext_copy(hec_ciphertext *dst, const hec_ciphertext *src); /* value semantics, deep copy */
/* device-to-device import/export of the raw u64 words (for RCCL exchanges done by the caller) */
int hec_ciphertext_export_device(const hec_ciphertext *ct, void *dev_dst);
int hec_ciphertext_import_device(hec_ciphertext *ct, const void *dev_src, uint64_t size, uint64_t level,
                                 double scale);
/* canonicalise every word mod its prime (after an integer sum of partial accumulators) */
int hec_ciphertext_reduce(hec_context *ctx, hec_ciphertext *ct);
/* synthetic input: uniformly random residues (RLWE ciphertexts are pseudo-uniform) */
int hec_ciphertext_fill_uniform(hec_ciphertext *ct, uint64_t size, uint64_t level, double scale, uint64_t seed);

int hec_plaintext_create(hec_context *ctx, hec_plaintext **out);
int hec_plaintext_destroy(hec_plaintext *pt);
int hec_plaintext_upload(hec_plaintext *pt, const uint64_t *host, uint64_t level, double scale);
/* synthetic NTT-form plaintext: uniform residues mod q_i from a seeded device generator (benchmarks) */
int hec_plaintext_fill_uniform(hec_plaintext *pt, uint64_t level, double scale, uint64_t seed);
int hec_plaintext_download(const hec_plaintext *pt, uint64_t *host); /* u64[level][N], synchronises */
int hec_plaintext_info(const hec_plaintext *pt, uint64_t *level, double *scale);
/* seal::CKKSEncoder::encode(values, [parms_id,] scale, destination) on the GPU, for `count` slot vectors at
 * once — the reference encodes every matrix column / diagonal this way before encryption
 * (src/demos/matrix_operations.cpp:1106-1108, client.cpp:228-230, he_math.cpp:32-53 through
 * he_util.h:33-36).  re / im: host doubles, count rows of n_values (n_values <= N/2; missing slots are
 * zero); im = NULL encodes real values (SEAL's vector<double> overload).  out[v] receives an NTT-form
 * plaintext at `level` with `scale`.  Errors as SEAL: "values has invalid size", "scale out of bounds",
 * "encoded values are too large". */
int hec_encode(hec_context *ctx, const double *re, const double *im, uint64_t n_values, uint64_t count, double scale,
               uint64_t level, hec_plaintext *const *out);
/* seal::CKKSEncoder::encode(double value, parms_id, scale, destination) (SEAL 4.1 encode_internal(double, ...)), the
 * scalar form he::util::drop_chain_levels and he::math use (include/he_util.h:33, src/core/he_math.cpp:32,40,53):
 * round(value * scale) as an exact integer, its residue mod every prime of `level` (negated for a negative value),
 * written to every word of that limb (the NTT form of a constant polynomial); no transform runs.  Errors as SEAL:
 * "parms_id is not valid for encryption parameters", "scale out of bounds", "encoded value is too large" (also for a
 * non-finite value). */
int hec_encode_scalar(hec_context *ctx, double value, double scale, uint64_t level, hec_plaintext *out);

/* ---------------------------------------------------------------- client half: decrypt / decode */
/* The last two calls of every reference demo (src/demos/matrix_operations.cpp:107,126-127,1153-1156; client.cpp,
 * fft.cpp, math_operations.cpp): Decryptor::decrypt then CKKSEncoder::decode, for batches.  Decryption is bit-exact;
 * the decoder follows SEAL 4.1's decode_internal (inverse NTT, exact CRT composition, centring on Q, the words summed
 * into a double times 1 / scale, DWTHandler::transform_to_rev over root_powers_, slot i read at
 * matrix_reps_index_map_[i]) as far as it can be restated without SEAL at hand: it is checked to a derived
 * floating-point tolerance against this repository's CPU restatement, not to SEAL's bits.
 * A batch may mix ciphertext sizes (>= 2) and levels (1 .. L); the engine groups it by (size, level).  Everything is
 * ordered on the context's stream; calls with host outputs synchronise.  Nothing is written on an error. */
/* seal::SecretKey (KeyGenerator::secret_key(), matrix_operations.cpp:1059-1060): host u64[K][N], NTT form at the key
 * level.  Like every object it may be destroyed before or after its context; its device memory is zero-filled
 * before it is freed, as SEAL wipes secret keys. */
int hec_secret_key_upload(hec_context *ctx, const uint64_t *host, hec_secret_key **out);
int hec_secret_key_download(const hec_secret_key *sk, uint64_t *host); /* u64[K][N], synchronises */
int hec_secret_key_destroy(hec_secret_key *sk);
/* Decryptor::decrypt (matrix_operations.cpp:126,1154; CKKS: dot_product_ct_sk_array): out[i] = sum_k cts[i][k] s^k
 * per limb, NTT form; out[i] receives the ciphertext's level and scale.  Errors as SEAL: "encrypted is not valid for
 * encryption parameters" (an empty handle, one of another context, size < 2), "secret key is not valid for
 * encryption parameters", "plain is not valid for encryption parameters" (an output handle of another context). */
int hec_decrypt(hec_context *ctx, const hec_secret_key *sk, const hec_ciphertext *const *cts, uint64_t count,
                hec_plaintext *const *out);
/* CKKSEncoder::decode (matrix_operations.cpp:127,1155) for `count` plaintexts: row v of re / im (host doubles,
 * n_values each, n_values <= N/2) receives the first n_values slots; im == NULL keeps the real parts (SEAL's
 * vector<double> overload).  Errors as SEAL: "plain is not valid for encryption parameters", "scale out of bounds"
 * (scale <= 0 or int(log2 scale) >= the level's total coefficient-modulus bits, the encoder's rule), "values has
 * invalid size" (n_values > N/2). */
int hec_decode(hec_context *ctx, const hec_plaintext *const *pts, uint64_t count, uint64_t n_values, double *re,
               double *im);
/* both in one pass, with no plaintext objects in between; the doubles are those of hec_decode(hec_decrypt()) */
int hec_decrypt_decode(hec_context *ctx, const hec_secret_key *sk, const hec_ciphertext *const *cts, uint64_t count,
                       uint64_t n_values, double *re, double *im);

/* ---------------------------------------------------------------- KeyGenerator / Encryptor -- */
/* The first lines of every reference demo (matrix_operations.cpp:1057-1065, client.cpp:87-115): KeyGenerator's
 * secret_key / create_public_key / create_relin_keys / create_galois_keys and Encryptor's encrypt /
 * encrypt_symmetric, generated on the GPU.
 *
 * Randomness.  Every generating call takes `seed`, a 64-byte SEAL prng_seed_type.  NULL draws 64 bytes from
 * getrandom(2) (HEC_ELOGIC when that fails; there is no time or pid fallback).  With a given seed the call's output
 * is a pure function of its arguments.  A SEED MUST NEVER BE REUSED ACROSS CALLS: two calls with one seed share their
 * sub-streams (the same `a` and the same noise), which reveals the difference of their plaintexts or keys.  Derive a
 * fresh seed per call (hecdna/seal_compat.hpp hashes a master seed with a call counter).
 * Sub-stream (call, role, i, j) is SEAL's Blake2xbPRNG on the 64-byte value BLAKE2Xb(input = the four values as
 * little-endian u64, key = seed, 64 bytes) = hec_seal_blake2xb; call 1 secret, 2 public key, 3 relin, 4 galois,
 * 5 encrypt_symmetric, 6 encrypt; role 1 the uniform `a`, 2 the noise `e`, 3 a ternary polynomial; (i, j) = relin
 * (digit, 0), galois (digit, galois_elt), encrypt_symmetric (batch index, 0), encrypt (batch index, 0) for u and e_0
 * and (batch index, 1) for e_1.  `a` is SEAL's sample_poly_uniform over the stream (what a seeded ciphertext's
 * receiver expands); a ternary polynomial is the same routine with the modulus 3 over N words, coefficient
 * (v mod 3) - 1; the noise is the centred binomial of SEAL 4.1's sample_poly_cbd (6 bytes per coefficient, in
 * [-21, 21]).  SEAL's own ternary stream and noise stream cannot be observed by any caller and are not reproduced.
 *
 * An RLWE sample over the primes S is c1 = a (used as drawn, NTT form), c0 = -(a s + NTT(e)).  Nothing is written on
 * an error.  Errors as SEAL: "secret key is not valid for encryption parameters", "public key is not valid for
 * encryption parameters", "plain is not valid for encryption parameters", "Galois element is not valid". */
typedef struct hec_public_key hec_public_key; /* seal::PublicKey: u64[2][K][N], NTT form, key level */
/* KeyGenerator::secret_key(): a ternary s, its residues on all K primes, NTT form */
int hec_keygen_secret(hec_context *ctx, const uint64_t seed[8], hec_secret_key **out);
/* KeyGenerator::create_public_key: one RLWE sample over all K primes */
int hec_keygen_public(hec_context *ctx, const hec_secret_key *sk, const uint64_t seed[8], hec_public_key **out);
int hec_public_key_upload(hec_context *ctx, const uint64_t *host, hec_public_key **out); /* u64[2][K][N] */
int hec_public_key_download(const hec_public_key *pk, uint64_t *host);                  /* synchronises */
int hec_public_key_destroy(hec_public_key *pk);
/* KeyGenerator::create_relin_keys (generate_one_kswitch_key): digit J is an RLWE sample over all K primes with
 * (P mod q_J) (s (*) s) added to limb J of c0; layout u64[L][2][K][N] */
int hec_keygen_relin(hec_context *ctx, const hec_secret_key *sk, const uint64_t seed[8], hec_kswitch_key **out);
/* KeyGenerator::create_galois_keys(elts): the same with apply_galois_ntt(s, elt) in place of s (*) s, for n
 * elements (n == 0: the set of hec_default_galois_elts); a key's words do not depend on the other elements asked
 * for.  The keys land as hec_galois_keys_add leaves them. */
int hec_keygen_galois(hec_galois_keys *gk, const hec_secret_key *sk, const uint32_t *elts, uint64_t n,
                      const uint64_t seed[8]);
/* Encryptor::encrypt_symmetric for `count` plaintexts (levels may differ): out[v] = an RLWE sample over the
 * plaintext's primes with the plaintext added to c0, at the plaintext's level and scale.  public_seeds (count * 8
 * words, or NULL) receives the sub-seed of every `a`, what hec_seal_ciphertext_save_seeded writes. */
int hec_encrypt_symmetric(hec_context *ctx, const hec_secret_key *sk, const hec_plaintext *const *pts, uint64_t count,
                          const uint64_t seed[8], hec_ciphertext *const *out, uint64_t *public_seeds);
/* Encryptor::encrypt (encrypt_zero_internal, asymmetric) for a plaintext at level l: over the l + 1 primes of the
 * level above (l = L: all K primes), t_j = u (*) pk_j + NTT(e_j) with u ternary, each t_j divided and rounded by the
 * last of these primes (the arithmetic of hec_rescale_to_next_inplace; the scale is left alone), then c0 += plain. */
int hec_encrypt(hec_context *ctx, const hec_public_key *pk, const hec_plaintext *const *pts, uint64_t count,
                const uint64_t seed[8], hec_ciphertext *const *out);

/* ---------------------------------------------------------------- keys -------------------- */
/* RelinKeys (KeyGenerator::create_relin_keys, matrix_operations.cpp:1061-1062): data u64[L][2][K][N] */
int hec_kswitch_key_upload(hec_context *ctx, const uint64_t *host, hec_kswitch_key **out);
/* device -> host in the layout of hec_kswitch_key_upload (synchronises) */
int hec_kswitch_key_download(const hec_kswitch_key *key, uint64_t *host);
int hec_kswitch_key_fill_uniform(hec_context *ctx, uint64_t seed, hec_kswitch_key **out);
int hec_kswitch_key_destroy(hec_kswitch_key *key);
/* GaloisKeys (KeyGenerator::create_galois_keys, matrix_operations.cpp:1063-1064) */
int hec_galois_keys_create(hec_context *ctx, hec_galois_keys **out);
int hec_galois_keys_add(hec_galois_keys *gk, uint32_t galois_elt, const uint64_t *host);
/* one Galois key, device -> host in the layout of hec_galois_keys_add (synchronises); HEC_EINVAL "Galois key not
 * present" when the set has no key for galois_elt */
int hec_galois_keys_download(const hec_galois_keys *gk, uint32_t galois_elt, uint64_t *host);
int hec_galois_keys_add_uniform(hec_galois_keys *gk, uint32_t galois_elt, uint64_t seed);
int hec_galois_keys_has(const hec_galois_keys *gk, uint32_t galois_elt);
int hec_galois_keys_destroy(hec_galois_keys *gk);

/* ---------------------------------------------------------------- evaluator --------------- */
/* Each replaces the seal::Evaluator call behind one he::operators operator
 * (reference include/he_operators.h:44-159, src/core/he_operators.cpp:14-237). */
int hec_negate_inplace(hec_context *ctx, hec_ciphertext *a);                                  /* op -= eval     */
int hec_add_inplace(hec_context *ctx, hec_ciphertext *a, const hec_ciphertext *b);           /* a += eval % b  */
int hec_sub_inplace(hec_context *ctx, hec_ciphertext *a, const hec_ciphertext *b);           /* a -= eval % b  */
int hec_add_plain_inplace(hec_context *ctx, hec_ciphertext *a, const hec_plaintext *p);      /* a += eval % pt */
int hec_sub_plain_inplace(hec_context *ctx, hec_ciphertext *a, const hec_plaintext *p);      /* a -= eval % pt */
int hec_multiply_inplace(hec_context *ctx, hec_ciphertext *a, const hec_ciphertext *b);      /* a *= eval % b  */
int hec_multiply_plain_inplace(hec_context *ctx, hec_ciphertext *a, const hec_plaintext *p); /* a *= eval % pt */
int hec_square_inplace(hec_context *ctx, hec_ciphertext *a);                                  /* he_linalg.cpp:647 */
int hec_relinearize_inplace(hec_context *ctx, hec_ciphertext *a, const hec_kswitch_key *rk); /* a &= eval % rk */
int hec_rescale_to_next_inplace(hec_context *ctx, hec_ciphertext *a);                         /* a ^= eval      */
int hec_mod_switch_to_next_inplace(hec_context *ctx, hec_ciphertext *a);                      /* a |= eval      */
/* a <<= eval % gk % steps (left); right rotation = negative steps (he_operators.cpp:204-235) */
int hec_rotate_vector_inplace(hec_context *ctx, hec_ciphertext *a, int steps, const hec_galois_keys *gk);
int hec_apply_galois_inplace(hec_context *ctx, hec_ciphertext *a, uint32_t galois_elt, const hec_galois_keys *gk);

/* ---------------------------------------------------------------- he::linalg hot path ----- */
/* BatchedMatrix::matmul(eval, rk, gk, other), diag(this) x col(other) (he_linalg.cpp:943-1006):
 *   out[i] = rescale(relin( sum_{j<n} rot(cols[i], j) (*) diags[j] )),  i < p
 * n diagonal ciphertexts, p column ciphertexts (the p independent input vectors of a matvec batch).
 * out[i] may be fresh ciphertexts; they receive level = input level - 1. */
int hec_matmul_diag_col(hec_context *ctx, const hec_ciphertext *const *diags, uint64_t n,
                        const hec_ciphertext *const *cols, uint64_t p, const hec_kswitch_key *rk,
                        const hec_galois_keys *gk, hec_ciphertext *const *out);
/* Sharded form: size-3 partial sums over diagonals [j_begin, j_end) (no relin / rescale). */
int hec_matmul_diag_col_partial(hec_context *ctx, const hec_ciphertext *const *diags, uint64_t n,
                                uint64_t j_begin, uint64_t j_end, const hec_ciphertext *const *cols, uint64_t p,
                                const hec_galois_keys *gk, hec_ciphertext *const *acc_out);
/* Sharded form over an arbitrary set of diagonal indices j_idx[0..nj) (any order, no duplicates): the
 * multi-GPU planner hands each rank whole subtrees of the rotation prefix trie so that no key switch
 * is repeated across ranks.  Summing the partials of a partition of [0, n) mod q gives exactly the
 * accumulator of hec_matmul_diag_col. */
int hec_matmul_diag_col_partial_set(hec_context *ctx, const hec_ciphertext *const *diags, uint64_t n,
                                    const uint64_t *j_idx, uint64_t nj, const hec_ciphertext *const *cols, uint64_t p,
                                    const hec_galois_keys *gk, hec_ciphertext *const *acc_out);
/* ct x pt matvec (the plaintext-diagonal form of BatchedMatrix::matmul diag x col,
 * he_linalg.cpp:943-1006, with `*= eval % plain` = multiply_plain_inplace, he_operators.cpp:128-142):
 *   out[i] = rescale_to_next( sum_j diags[j] (x) rot(cols[i], j) )
 * diags: n NTT-form plaintexts at the columns' level (SEAL CKKSEncoder output layout u64[level][N]).
 * The products stay size 2, so there is no relinearization; rotations as in hec_matmul_diag_col. */
int hec_matmul_diagpt_col(hec_context *ctx, const hec_plaintext *const *diags, uint64_t n,
                          const hec_ciphertext *const *cols, uint64_t p, const hec_galois_keys *gk,
                          hec_ciphertext *const *out);
/* The rotation steps of the baby-step giant-step ct x pt matvec below (host only, no context): the babies
 * 1 .. bs_eff - 1, then the giants g bs_eff for 1 <= g < ceil(n / bs_eff), with bs_eff = min(bs, n); bs = 0 picks the
 * smallest power of two >= sqrt(n).  A caller with a key for exactly these steps (hec_keygen_galois over their
 * elements) pays one key switch per step: (bs_eff - 1) + (ceil(n / bs_eff) - 1) against the n - 1 rotations, each
 * a NAF chain, of BatchedMatrix::matmul's loop (he_linalg.cpp:943-1006; `*= eval % plain` is multiply_plain_inplace,
 * he_operators.cpp:128-142).  The schedule is not the reference's, so its ciphertext bits are not either.
 * *count = the number of steps, min(cap, *count) of them written to steps; *bs_eff (optional) = bs_eff.
 * HEC_EINVAL for n = 0, n >= 2^30 and bs_eff > 1024. */
int hec_bsgs_plan(uint64_t n, uint64_t bs, int *steps, uint64_t cap, uint64_t *count, uint64_t *bs_eff);
/* ct x pt matvec on the baby-step giant-step schedule: the product of hec_matmul_diagpt_col (he_linalg.cpp:943-1006
 * with multiply_plain, he_operators.cpp:128-142) from (bs_eff - 1) + (G - 1) rotations, G = ceil(n / bs_eff):
 *   inner_g = sum_{i < bs_eff, g bs_eff + i < n} multiply_plain(rotate_vector(cols[c], i), pdiags[g bs_eff + i])
 *   out[c]  = rescale_to_next( inner_0 + sum_{1 <= g < G} rotate_vector(inner_g, g bs_eff) )
 * pdiags are in BSGS form: pdiags[j] encodes diagonal j's slot vector rotated right by (j / bs_eff) bs_eff slots.
 * NOT bit-identical to hec_matmul_diagpt_col unless bs_eff = n (it decrypts to the same product); it IS word for
 * word, with level and scale, what the per-operation calls above give when composed in this order, rotate_vector by
 * SEAL's rule (the step's own key, else its NAF chain).  Every check (objects, sizes, levels, scales, "end of
 * modulus switching chain reached", "Galois key not present" over every step of hec_bsgs_plan) comes before the
 * first write.  out[c] may be cols[c]; an output that is another entry's input, or listed twice, is HEC_EINVAL.
 * A pass of Bc input vectors holds (nodes + GG + 2) Bc ciphertexts of workspace beside the key switch's own: nodes =
 * the nodes of the baby rotations' prefix trie (bs_eff with a key per step, more on a sparser key set such as the
 * default one, whose NAF chains pass through steps outside 0 .. bs_eff - 1), GG = "bsgs_gg".  Bc is halved until that
 * fits the free device memory; when not even one vector fits, the call fails with HEC_EDEVICE (an allocation error).
 * Runs on the context's stream in passes of at most "bsgs_chunk" input vectors (option, 0..65535, 0 = automatic);
 * the outputs do not depend on it, nor on "bsgs_bg" (1, 2, 4), "bsgs_gg" (2, 4, 8, 16) and "bsgs_order" (0..1), the
 * inner-sum kernel's tile and grid order.  Batch lanes and the sharded path do not take this route. */
int hec_matmul_diagpt_col_bsgs(hec_context *ctx, const hec_plaintext *const *pdiags, uint64_t n, uint64_t bs,
                               const hec_ciphertext *const *cols, uint64_t p, const hec_galois_keys *gk,
                               hec_ciphertext *const *out);
/* ct x ct matvec on the baby-step giant-step schedule: the product of hec_matmul_diag_col (BatchedMatrix::matmul
 * diag x col, he_linalg.cpp:943-1006) from (bs_eff - 1) baby rotations, G relinearisations and (G - 1) giant
 * rotations, G = ceil(n / bs_eff), bs_eff = min(bs, n), bs = 0 hec_bsgs_plan's choice:
 *   inner_g = sum_{i < bs_eff, g bs_eff + i < n} multiply(rotate_vector(cols[c], i), diags[g bs_eff + i])   (size 3)
 *   r_g     = relinearize(inner_g, rk)
 *   out[c]  = rescale_to_next( r_0 + sum_{1 <= g < G} rotate_vector(r_g, g bs_eff) )
 * diags are in BSGS form: diags[j] encrypts diagonal j's slot vector rotated right by (j / bs_eff) bs_eff slots (the
 * client rolls the slot vector before encrypting it, which costs nothing and adds no noise).  The rotation steps are
 * those of hec_bsgs_plan.  NOT bit-identical to hec_matmul_diag_col unless bs_eff = n, where G = 1 and the two
 * definitions coincide (it decrypts to the same product; every giant group's relinearisation adds its own noise); it
 * IS word for word, with level and scale, what the per-operation calls above give when composed in this order,
 * rotate_vector by SEAL's rule (the step's own key, else its NAF chain).
 * bs_eff > 512 is HEC_EINVAL "bs must be at most 512": the inner-sum kernel adds two exact FP64 products per term,
 * which stays below 2^52 for 966 terms at most; the ct x pt call keeps its 1024.
 * Every check comes before the first write, in this order: objects and the Galois keys of this context, sizes 2,
 * one level, "scale out of bounds" and "scale mismatch" over every product, "end of modulus switching chain
 * reached", rk of this context, "Galois key not present" over every step of hec_bsgs_plan, the aliasing rule: out[c]
 * may be cols[c]; an output that is another entry's input or a diagonal, or listed twice, is HEC_EINVAL.
 * A pass of Bc input vectors holds (nodes + 2 + 1.5 GG) Bc ciphertexts of workspace beside the key switch's own,
 * which covers GG Bc entries when the tile's relinearisations run as one key switch (GG Bc (l + 1) l <= 65,535):
 * nodes = the nodes of the baby rotations' prefix trie (as for hec_matmul_diagpt_col_bsgs), GG = "bsgs_ct_gg" size-3
 * slots.  Bc is halved until that fits the free device memory; when not even one vector fits, the call fails with
 * HEC_EDEVICE.  Runs on the context's stream in passes of at most "bsgs_chunk" input vectors; the outputs do not
 * depend on it, nor on "bsgs_ct_bg" (1, 2), "bsgs_ct_gg" (2, 4, 8) and "bsgs_order" (0..1), the inner-sum kernel's
 * tile and grid order.  Batch lanes and the sharded path do not take this route. */
int hec_matmul_diag_col_bsgs(hec_context *ctx, const hec_ciphertext *const *diags, uint64_t n, uint64_t bs,
                             const hec_ciphertext *const *cols, uint64_t p, const hec_kswitch_key *rk,
                             const hec_galois_keys *gk, hec_ciphertext *const *out);
/* relinearize + rescale a batch of size-3 accumulators (he_linalg.cpp:999-1002) */
int hec_matmul_finish(hec_context *ctx, hec_ciphertext *const *acc, uint64_t p, const hec_kswitch_key *rk,
                      hec_ciphertext *const *out);
/* BatchedMatrix::matmul, col(this) x col(other)^T -> diag output:
 *   out[i] = rescale(relin( sum_{j<n} rot(B[j], i) (*) A[j] )), i < p */
int hec_matmul_col_colT(hec_context *ctx, const hec_ciphertext *const *A, uint64_t n,
                        const hec_ciphertext *const *B, uint64_t p, const hec_kswitch_key *rk,
                        const hec_galois_keys *gk, hec_ciphertext *const *out);
/* The form of a matrix's ciphertext diagonals: natural (diagonal i as it is), or the BSGS form for a block size bs
 * (diagonal i rotated right by (i / bs_eff) bs_eff slots, what hec_matmul_diag_col_bsgs takes). */
#define HEC_DIAG_NATURAL 0
#define HEC_DIAG_BSGS 1
/* The rotation steps of hec_matmul_col_colT_bsgs below (host only, no context), with bs_eff = min(bs, p), G =
 * ceil(p / bs_eff) and bs = 0 the smallest power of two >= sqrt(p) (hec_bsgs_plan's rule applied to p): the babies
 * 1 .. bs_eff - 1, then the negative giants -g bs_eff for 1 <= g < G, then, for form HEC_DIAG_NATURAL only, the
 * positive giants g bs_eff for 1 <= g < G.  A key set with exactly these steps' elements makes every rotation one
 * key switch.  *count = the number of steps, min(cap, *count) of them written to steps; *bs_eff (optional) = bs_eff.
 * HEC_EINVAL for p = 0, p >= 2^30 and a form outside {0, 1}. */
int hec_colcolT_bsgs_plan(uint64_t p, uint64_t bs, int form, int *steps, uint64_t cap, uint64_t *count,
                          uint64_t *bs_eff);
/* col x col^T -> diag product on the baby-step giant-step schedule: the product of hec_matmul_col_colT from
 * n (bs_eff - 1) baby rotations of B and n (G - 1) giant rotations of A in place of its n (p - 1) rotations of B.
 * With output i = g bs_eff + b (b < bs_eff, g < G, i < p):
 *   Bb[j][b] = rotate_vector(B[j], b)               (b = 0: B[j] itself)
 *   Ag[j][g] = rotate_vector(A[j], -g bs_eff)       (g = 0: A[j] itself)
 *   acc_i    = sum_{j < n} multiply(Bb[j][b], Ag[j][g])                                        (size 3)
 *   r_i      = rescale_to_next(relinearize(acc_i, rk))
 *   out[i]   = r_i                                  form HEC_DIAG_BSGS
 *   out[i]   = rotate_vector(r_i, g bs_eff)         form HEC_DIAG_NATURAL (g = 0: r_i)
 * since rot(B[j], i) (.) A[j] = rot( rot(B[j], b) (.) rot(A[j], -g bs_eff), g bs_eff ).  The result IS word for word,
 * with level and scale, what the per-operation calls above give when composed in this order, rotate_vector by SEAL's
 * rule (the step's own key, else its NAF chain).  It is NOT the bits of hec_matmul_col_colT unless G = 1 (bs_eff = p),
 * where the two definitions coincide and both forms are equal (it decrypts to the same product).  Form HEC_DIAG_BSGS
 * with block size bs is the input form of hec_matmul_diag_col_bsgs with the same bs and n = p: r_i is diagonal i
 * rotated right by g bs_eff slots, so the output needs no rotation at all and feeds that matvec directly (no
 * bsgs_rotate_diagonals pass).  Outputs have level l - 1 and scale sc / q_{l-1}, sc = B[j]->scale A[j]->scale.
 * Every check comes before the first write, in this order: null arguments and n, p >= 1; the form; the Galois keys
 * of this context; every A[j] and B[j] (object, size 2, one level); "scale out of bounds" and "scale mismatch" over
 * B[j]->scale A[j]->scale; "end of modulus switching chain reached" for l < 2; rk of this context; "Galois key not
 * present" over every step of hec_colcolT_bsgs_plan (a key holds every level, so one found at level l serves the
 * positive giants at l - 1 too); the aliasing rule: an output handle that is any input, or that is listed twice, is
 * HEC_EINVAL.  Nothing is written on an error.
 * Runs on the context's stream in passes of Jc columns: Jc <= 512 (the inner-sum kernel adds two exact FP64 products
 * per column, which stays below 2^52 for 966 columns at most), Jc <= 65,535 / ((l + 1) l), at most
 * "cct_jchunk" (option, 0..512, 0 = automatic).  The workspace holds the p size-3 accumulators, the p outputs,
 * (nodes_B + nodes_A + 2) Jc ciphertexts for the two rotation tries (their nodes beside the roots: bs_eff - 1 and
 * G - 1 with a key per step, more on a sparser key set) and the key switch's own; Jc is halved until that fits the
 * free device memory, and when not even one column fits the call fails with HEC_EDEVICE.  The outputs do not depend
 * on the pass size, nor on "cct_tb" (1, 2, 4), "cct_tg" (1, 2, 4) and "bsgs_order" (0..1), the inner-sum kernel's
 * tile and grid order.  Batch lanes and the sharded path do not take this route. */
int hec_matmul_col_colT_bsgs(hec_context *ctx, const hec_ciphertext *const *A, uint64_t n,
                             const hec_ciphertext *const *B, uint64_t p, uint64_t bs, int form,
                             const hec_kswitch_key *rk, const hec_galois_keys *gk, hec_ciphertext *const *out);
/* Matrix::matmul (he_linalg.cpp:202-236): column-major element-wise ciphertext matrices
 * (index i + rows*j, swapped when *_transposed); out has r1*c2 entries, column-major. */
int hec_matrix_matmul(hec_context *ctx, const hec_ciphertext *const *A, uint64_t a_rows, uint64_t a_cols,
                      int a_transposed, const hec_ciphertext *const *B, uint64_t b_rows, uint64_t b_cols,
                      int b_transposed, const hec_kswitch_key *rk, hec_ciphertext *const *out);

/* ---------------------------------------------------------------- he::fft ------------------ */
/* The doubles he::fft encodes (reference src/core/he_fft.cpp:40,55 and :92-149), host only, no device: the one
 * source of these values for the engine, the C++ drop-in and the tests (libstdc++'s std::exp and
 * std::pow(complex<double>, size_t), which is not the repeated product; entry 0 is (1, -0)).
 * hec_fft_twiddles: re/im[k] = pow(exp(i s (-2 pi) / m), k) for k < m / 2, s = +1 forward, -1 inverse; m a power of
 * two >= 2.  hec_bfft_diagonal: the n values of diag_D<s>(d, k, n) before it is tiled over slot_count, d in {0, 1, 2}
 * (d = 2 needs k > 2), k = 2^i <= n.  HEC_EINVAL for arguments outside these ranges (no message is recorded). */
int hec_fft_twiddles(uint64_t m, int inverse, double *re, double *im);
int hec_bfft_diagonal(int d, uint64_t k, uint64_t n, int inverse, double *re, double *im);
/* he::fft::fft / ifft (he_fft.cpp:13-87): the radix-2 FFT over n ciphertexts, out[j] = sum_i in[i] w_n^(i j).
 * Every butterfly of block size m is E = rescale(e (*) encode(1 + 0i)), T = rescale(o (*) encode(w_m^k)), E + T and
 * E - T, the plaintexts complex-scalar encodes at the operands' level and scale; ifft multiplies every output by
 * the scalar encode of 1.0 / n and rescales once more.  A stage runs over all n ciphertexts at once.  n a power
 * of two ("n must be a power of two"; the reference does not check); every in[i] of size 2 ("encrypted size must be
 * 2"), at one level ("encrypted1 and encrypted2 parameter mismatch") with bitwise-equal scales ("scale mismatch");
 * level >= log2 n + 1, one more for the inverse ("end of modulus switching chain reached"); "scale out of bounds"
 * where a multiply_plain of the chain would throw it.  Nothing is written on an error.  out[i] may be a fresh
 * handle or in[i]; n = 1 forward copies.  n * 2 * (level - 1) <= 65535. */
int hec_fft(hec_context *ctx, const hec_ciphertext *const *in, uint64_t n, int inverse, hec_ciphertext *const *out);
/* he::fft::bfft / ibfft (he_fft.cpp:166-223) on B independent ciphertexts whose slot vectors are n-periodic (B = 1
 * is the reference's call): for i = 1 .. log2 n, k = 2^i, steps = n / k,
 *   y = rescale(y (*) D0) + rescale(rot(y, +steps) (*) D1) [+ rescale(rot(y, -steps) (*) D2) for i > 1],
 * the diagonals hec_bfft_diagonal's values tiled over slot_count; ibfft adds the 1.0 / n step.  Each n-block of
 * the result is its DFT in bit-reversed order.  Rotations as hec_rotate_vector_inplace (one key for +-steps, else the
 * NAF terms; "Galois key not present").  Errors as hec_fft, and n <= slot_count ("n must be at most slot_count"). */
int hec_bfft(hec_context *ctx, const hec_ciphertext *const *in, uint64_t B, uint64_t n, int inverse,
             const hec_galois_keys *gk, hec_ciphertext *const *out);

/* ---------------------------------------------------------------- he::math ----------------- */
/* The reference's he::math (src/core/he_math.cpp:22-269) on B ciphertexts at once.  out[i] is, bit for bit with its
 * level and scale, what the per-operation schedule (scalar encodes at the ciphertext's parms_id and scale,
 * multiply_plain, multiply / square, relinearize, rescale_to_next, add_plain / sub_plain, sub) gives for x[i] alone;
 * every stage of that schedule runs once over the whole batch.  B >= 1; every x[i] of size 2 ("encrypted size must be
 * 2"), at one level ("encrypted1 and encrypted2 parameter mismatch"), with bitwise-equal scales ("scale mismatch");
 * iter_num >= 1 ("iter_num must be positive"; the reference asserts); rk of this context ("relin_keys is not valid
 * for encryption parameters").  The host checks of the whole schedule run first, in the schedule's order, and the
 * first that fails is the call's status and message ("scale out of bounds", "end of modulus switching chain
 * reached", "encoded value is too large", "scale mismatch"); nothing is written on an error.  out[i] may be a fresh
 * handle or x[i].  Ordered on the context's stream; a batch larger than one pass allows (65,535 blocks per NTT
 * launch, or the option "math_chunk") runs in several passes. */
#define HEC_MATH_SIGNED_INV 0
#define HEC_MATH_INV_SQRT_TWICE 1
#define HEC_MATH_SQRT 2
#define HEC_MATH_ABS 3
/* host only, no device: the level and scale the call below would return for inputs at (level, scale), or the status
 * and message of the first check that the per-operation sequence would fail.  coeff_modulus: the K key moduli */
int hec_math_plan(const uint64_t *coeff_modulus, uint64_t K, int fn, double a, uint64_t iter_num, uint64_t level,
                  double scale, uint64_t *out_level, double *out_scale);
/* signed_inv (he_math.cpp:22-90): 1/x = a prod_k (1 + (1 - a x)^(2^k)) from 2a - a^2 x; |a x - 1| < 1 */
int hec_math_signed_inv(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, double a, uint64_t iter_num,
                        const hec_kswitch_key *rk, hec_ciphertext *const *out);
/* inv_sqrt_twice (he_math.cpp:95-164, the `#if 1` form): Newton for 1/sqrt(2x), y' = 3/2 y - x y^3 from y0 = a */
int hec_math_inv_sqrt_twice(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, double a, uint64_t iter_num,
                            const hec_kswitch_key *rk, hec_ciphertext *const *out);
/* sqrt (he_math.cpp:211-232): inv_sqrt_twice(x, 1 / a / sqrt 2) times sqrt(2) x dropped to its level */
int hec_math_sqrt(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, double a, uint64_t iter_num,
                  const hec_kswitch_key *rk, hec_ciphertext *const *out);
/* abs (he_math.cpp:237-269): inv_sqrt_twice(x^2, 1 / a / sqrt 2) times sqrt(2) x^2 dropped to its level */
int hec_math_abs(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, double a, uint64_t iter_num,
                 const hec_kswitch_key *rk, hec_ciphertext *const *out);
/* Polynomial evaluation, an extension (the reference has none): out[i] = sum_j coeffs[j] x[i]^j, j = 0 .. degree, by
 * Paterson-Stockmeyer with block size bs (a power of two in [2, 16]; 0 chooses 2^m, m = min(4, max(1, ceil(ceil(log2(
 * d + 1)) / 2)))), on B ciphertexts at once.  out[i] is, bit for bit with its level and scale, what the per-operation
 * schedule of DESIGN.md 2.9 gives for x[i] alone: x^j = rescale(relin(x^ceil(j/2) x^floor(j/2))) after
 * mod_switch_to_next to the lower level, each power once; a leaf (degree below bs) is the sum of multiply_plain by
 * scalar encodes whose scales land every term on one assigned scale, rescaled once, plus add_plain of the constant; a
 * node is Eval(quotient) x^g + Eval(remainder), g = bs 2^k <= degree.  The output scale is the input scale bitwise and
 * the output level is the one hec_math_poly_plan reports (a dense polynomial of degree 7 or 8 takes four levels, of
 * degree 63 seven).  Real finite coefficients
 * ("coefficients must be finite"); trailing zeros are trimmed and what remains must not be constant ("polynomial
 * must not be constant"); degree < 2^16 ("degree must be below 2^16"); "bs must be a power of two in [2, 16]".  A
 * coefficient that is exactly 0.0 issues no step.  Inputs, rk, passes, the order of the host checks and their messages
 * as the calls above; nothing is written on an error.  out[i] may be a fresh handle or x[i]. */
int hec_math_poly(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, const double *coeffs, uint64_t degree,
                  uint64_t bs, const hec_kswitch_key *rk, hec_ciphertext *const *out);
/* host only, no device: the level and scale hec_math_poly would return for inputs at (level, scale), the block size
 * it uses, its products (relinearised multiplications, the powers included) and its leaves (linear-combination
 * stages); or the status and message of the first check that fails.  coeff_modulus: the K key moduli */
int hec_math_poly_plan(const uint64_t *coeff_modulus, uint64_t K, const double *coeffs, uint64_t degree, uint64_t bs,
                       uint64_t level, double scale, uint64_t *out_level, double *out_scale, uint64_t *bs_eff,
                       uint64_t *products, uint64_t *leaves);
/* he::util::drop_chain_levels (he_util.h:27-48) on B ciphertexts in place: per level, every ciphertext times the
 * scalar encode of 1 at the first one's level and scale, rescaled.  Inputs and errors as above; levels = 0 is a no-op */
int hec_drop_chain_levels(hec_context *ctx, hec_ciphertext *const *cts, uint64_t B, uint64_t levels);

/* ---------------------------------------------------------------- he::linalg element-wise products and sums */
/* The members of he::linalg that touch many ciphertexts element by element (Matrix::operator*=, BatchedMatrix::
 * operator*=, square_inplace and sum_bvec_elems_inplace) as single calls over B ciphertexts: out[i] is, word for word
 * and with the same level and scale, what the per-operation calls give for entry i alone.  Entries may sit at
 * different levels and scales: they are grouped by level on the host, each group runs its stages over the whole group
 * (in passes of at most 65,535 / ((l + 1) l) ciphertexts, or the option "math_chunk"), and the outputs keep the
 * caller's order.  Every check runs before anything is written, in entry order, and the status and message are those
 * of the per-operation call on the lowest failing entry: inputs of size 2 ("encrypted size must be 2"), "encrypted1
 * and encrypted2 parameter mismatch" for a pair at two levels, "scale out of bounds", "end of modulus switching chain
 * reached", "Galois key not present", the messages of a key or ciphertext of another context.  out[i] may be a fresh
 * handle or entry i's own input; an output handle that is another entry's input, or that appears twice, is
 * HEC_EINVAL ("an output may alias only its own entry's inputs").  B = 0 succeeds and does nothing.  Ordered on the
 * context's stream. */
/* out[i] = rescale_to_next(relinearize(a[i] * b[i], rk)); b[i] == a[i] (the same handle) is square. */
int hec_multiply_relin_rescale_many(hec_context *ctx, const hec_ciphertext *const *a,
                                    const hec_ciphertext *const *b, uint64_t B,
                                    const hec_kswitch_key *rk, hec_ciphertext *const *out);
/* out[i] = BatchedVector::sum_elems_inplace on x[i] with this dim (he_linalg.cpp:667-713): slot 0 of every block of
 * dim slots holds the block's sum.  gk must hold the key of every step of hec_sum_elems_plan(dim); dim = 0 is
 * HEC_EINVAL ("dim must be positive").  With the option "rot_add" = 1 every accumulate step acc + rotate(src, step)
 * is one key switch whose last stage also adds acc; with 0 the add is a launch of its own.  Same words either way. */
int hec_sum_elems_many(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, uint64_t dim,
                       const hec_galois_keys *gk, hec_ciphertext *const *out);
/* host only: the rotation steps that schedule issues for dim, in order, including the ones whose
 * result the reference discards (e.g. dim = 1 rotates once and keeps the input).  *count is their number; at most
 * cap of them are written to steps (steps may be null when cap is 0). */
int hec_sum_elems_plan(uint64_t dim, int *steps, uint64_t cap, uint64_t *count);

/* ---------------------------------------------------------------- multi-GPU (SURVEY 8(b),(e)) */
/* One process per GPU.  The reference is single-threaded (no collective anywhere); the sharded matvec splits
 * the diagonal loop of BatchedMatrix::matmul (he_linalg.cpp:977-997) over the ranks and exchanges the size-3
 * partial sums once over RCCL (xGMI), so a C++ caller of the he_linalg.h drop-in shards through this ABI alone.
 *
 * Planner (host only, no GPU): rank_of_diag[j] = the rank that owns diagonal j < n: whole subtrees of the
 * rotation prefix trie (SEAL's key-switch sequences over the key set key_elts), balanced by key switches. */
int hec_plan_diagonal_shards(uint64_t poly_modulus_degree, uint64_t n, int world, const uint32_t *key_elts,
                             uint64_t nkeys, int32_t *rank_of_diag);
/* ncclGetUniqueId: 128 bytes that rank 0 creates and every rank passes to hec_comm_init (RCCL is loaded on
 * first use from librccl.so.1; HEC_ELOGIC when it is absent). */
int hec_comm_unique_id(void *unique_id);
/* ncclCommInitRank on the context's device; world == 1 needs no id; 1 <= world <= 8 (the partial-sum exchange
 * adds world canonical 60-bit residues in u64).  The communicator lives until hec_context_destroy. */
int hec_comm_init(hec_context *ctx, int rank, int world, const void *unique_id);
/* A host communicator: the caller's own collectives (MPI, a gloo process group, ...) for the sharded
 * matvec, in place of RCCL.  Both callbacks are all-reduces over the world, in place, on host memory, and return
 * 0 on success.  allreduce_f64: op HEC_REDUCE_MIN or HEC_REDUCE_MAX.  allreduce_u64_sum: exact (world <= 8
 * residues < 2^60).  The engine calls them from the thread that called hec_matmul_diag_col_sharded. */
#define HEC_REDUCE_MIN 0
#define HEC_REDUCE_MAX 1
typedef struct hec_comm_ops {
    void *user;
    int (*allreduce_f64)(void *user, double *buf, uint64_t count, int op);
    int (*allreduce_u64_sum)(void *user, uint64_t *buf, uint64_t count);
} hec_comm_ops;
/* hec_comm_init with the caller's collectives (*ops is copied); same world bound. */
int hec_comm_init_ops(hec_context *ctx, int rank, int world, const hec_comm_ops *ops);
/* The agreement step hec_matmul_diag_col_sharded runs before any data moves (host only, no device needed): each
 * rank passes its own check result (status HEC_OK / HEC_EINVAL / HEC_ELOGIC and SEAL's message) and its p output
 * product scales; after two allreduce_f64 calls a failing rank returns its own status and message, every other rank
 * the status of the failing rank with the larger (status << 8 | rank + 1) and "... failed SEAL's checks on rank r";
 * when no rank failed, every rank returns HEC_EINVAL "scale mismatch" if the ranks' scales of one output are not
 * SEAL-close (add_inplace over the whole sum), else HEC_OK.  No rank is left waiting in the exchange.  msg (cap bytes,
 * may be NULL) receives the message.  HEC_EDEVICE / HEC_ELOGIC when a callback fails. */
int hec_shard_agree(const hec_comm_ops *ops, int rank, int status, const char *reason, const double *scales,
                    uint64_t p, char *msg, uint64_t msg_cap);
/* 1 when the context has a communicator (then *rank, *world are set), 0 when not, HEC_EINVAL on NULL */
int hec_context_comm(const hec_context *ctx, int *rank, int *world);
/* BatchedMatrix::matmul diag x col over the world (every rank calls it with the same arguments): rank r
 * computes the partial sums over its planned diagonals (hec_plan_diagonal_shards with the keys of gk): only those
 * diags[j] are read and checked, every other entry is never dereferenced and may be NULL or any handle.  The
 * ranks then agree on the argument checks (hec_shard_agree's protocol: two all-reduces of p + 1 doubles, min and
 * max, over the RCCL or the host communicator, so an error on one rank is returned on all ranks instead of leaving
 * the others in the exchange), run one all-reduce of the partials (RCCL,
 * or the host communicator of hec_comm_init_ops; u64 sum, exact
 * for world <= 8 and 60-bit primes) + reduction mod q, and every rank relinearizes and rescales all p outputs:
 * out[i] is bit-identical to hec_matmul_diag_col on one GPU. */
int hec_matmul_diag_col_sharded(hec_context *ctx, const hec_ciphertext *const *diags, uint64_t n,
                                const hec_ciphertext *const *cols, uint64_t p, const hec_kswitch_key *rk,
                                const hec_galois_keys *gk, hec_ciphertext *const *out);

/* ---------------------------------------------------------------- SEAL wire format */
/* seal::Serialization::Save / Load byte layouts of the objects the reference's socket layer exchanges
 * (src/demos/client.cpp:113-115,238-240 saves, src/demos/server.cpp:110-122,140-152 loads): SEALHeader (16 B:
 * magic 0xA15E, header size, version 4.1, compr_mode, size) + members, compr_mode HEC_COMPR_NONE / ZLIB / ZSTD
 * (zlib, zstd loaded on first use).  Host-only functions return HEC_EINVAL with SEAL's wording for malformed
 * input ("loaded SEALHeader is invalid", ...); hec_seal_last_error() holds the message.  Seeded ciphertexts
 * (encrypt_symmetric().save(), client.cpp:113-114) are expanded by hec_seal_ciphertext_load_ex and by the device
 * loader hec_ciphertext_load_seal (Ciphertext::expand_seed); hec_seal_ciphertext_load, which has no moduli,
 * rejects them (HEC_EINVAL).  Decompressed objects are bounded, since the bytes come from a client socket
 * (server.cpp:110-122): 2 GiB per ciphertext; a key object (with every compressed member nested in it) by the
 * caller's max_bytes in the *_ex forms, by 16 GiB in the others, and by a fixed count of key lists in the device
 * loaders (hec_galois_keys_load_seal_ex; it does not depend on the device's free memory).  A payload over its limit is HEC_EINVAL ("decompressed SEAL object exceeds the
 * size limit"); a payload must also hold the words it announces. */
#define HEC_COMPR_NONE 0
#define HEC_COMPR_ZLIB 1
#define HEC_COMPR_ZSTD 2
const char *hec_seal_last_error(void);
/* BLAKE2b (util::HashFunction behind parms_id), outlen <= 64 bytes */
int hec_seal_blake2b(const void *in, uint64_t nbytes, uint64_t outlen, void *out);
/* EncryptionParameters::parms_id() of CKKS {N, coeff_modulus[0..count)} (a ciphertext at level l: its l primes) */
int hec_seal_parms_id(uint64_t poly_modulus_degree, const uint64_t *coeff_modulus, uint64_t count, uint64_t out[4]);
/* Ciphertext::load / save on host buffers: data u64[size][level][N]; *consumed / *written = object bytes
 * (out == NULL: size query) */
int hec_seal_ciphertext_load(const void *bytes, uint64_t nbytes, uint64_t *size, uint64_t *level,
                             uint64_t *poly_modulus_degree, double *scale, uint64_t parms_id[4], uint64_t *data,
                             uint64_t data_words, uint64_t *consumed);
/* Ciphertext::load(context, ...) including a seeded object (c0 + UniformRandomGeneratorInfo, as
 * Encryptor::encrypt_symmetric(...).save writes it: src/demos/client.cpp:113-114): c1 is expanded with SEAL 4.1's
 * Ciphertext::expand_seed (Blake2xbPRNG + sample_poly_uniform) over coeff_modulus[0..level); the parms_id must
 * match; prng_type blake2xb (SEAL's default) or shake256.  coeff_modulus = NULL behaves as hec_seal_ciphertext_load (a seeded object is an error). */
int hec_seal_ciphertext_load_ex(const void *bytes, uint64_t nbytes, const uint64_t *coeff_modulus, uint64_t count,
                                uint64_t *size, uint64_t *level, uint64_t *poly_modulus_degree, double *scale,
                                uint64_t parms_id[4], uint64_t *data, uint64_t data_words, uint64_t *consumed);
/* BLAKE2Xb XOF (SEAL util/blake2xb.c, behind Blake2xbPRNG): outlen bytes of BLAKE2Xb(in) keyed with key */
int hec_seal_blake2xb(const void *in, uint64_t nbytes, const void *key, uint64_t keylen, uint64_t outlen, void *out);
/* SHAKE256 XOF (behind SEAL's Shake256PRNG) */
int hec_seal_shake256(const void *in, uint64_t nbytes, uint64_t outlen, void *out);
int hec_seal_ciphertext_save(const uint64_t *data, uint64_t size, uint64_t level, uint64_t poly_modulus_degree,
                             double scale, const uint64_t *coeff_modulus, int compr_mode, void *out, uint64_t cap,
                             uint64_t *written);
/* Serializable<Ciphertext>::save of Encryptor::encrypt_symmetric(plain) (client.cpp:113-114), host only: c0
 * (u64[level][N]) and the UniformRandomGeneratorInfo {prng_type 1 (blake2xb), prng_seed} that Ciphertext::expand_seed
 * and hec_seal_ciphertext_load_ex expand into c1; prng_seed = the public_seeds entry of hec_encrypt_symmetric. */
int hec_seal_ciphertext_save_seeded(const uint64_t *c0, uint64_t level, uint64_t poly_modulus_degree, double scale,
                                    const uint64_t *coeff_modulus, const uint64_t prng_seed[8], int compr_mode,
                                    void *out, uint64_t cap, uint64_t *written);
/* EncryptionParameters::load / save (CKKS) */
int hec_seal_parms_load(const void *bytes, uint64_t nbytes, uint64_t *poly_modulus_degree, uint64_t *coeff_modulus,
                        uint64_t cap, uint64_t *count, uint64_t *consumed);
int hec_seal_parms_save(uint64_t poly_modulus_degree, const uint64_t *coeff_modulus, uint64_t count, int compr_mode,
                        void *out, uint64_t cap, uint64_t *written);
/* the decompressed-size limit of the context-free key loaders below: 16 GiB (SEAL's default GaloisKeys at
 * N = 2^16 with 17 primes take 8.84 GB), bounded by half the host's available memory (the object is inflated in host
 * memory), at least 1 GiB */
uint64_t hec_seal_kswitch_keys_default_limit(void);
/* KSwitchKeys (RelinKeys, GaloisKeys) load of key list `index` (RelinKeys 0, GaloisKeys (galois_elt - 1) / 2)
 * in the engine's key layout u64[L][2][K][N]; *lists = the object's list count, *words = that list's words */
int hec_seal_kswitch_keys_load(const void *bytes, uint64_t nbytes, uint64_t index, uint64_t *lists, uint64_t *out,
                               uint64_t cap_words, uint64_t *words, uint64_t *consumed);
/* ... with at most max_bytes decompressed (0: hec_seal_kswitch_keys_default_limit) */
int hec_seal_kswitch_keys_load_ex(const void *bytes, uint64_t nbytes, uint64_t index, uint64_t max_bytes,
                                  uint64_t *lists, uint64_t *out, uint64_t cap_words, uint64_t *words,
                                  uint64_t *consumed);
/* The same object in ONE pass: visit(user, index, words, nwords) is called for every non-empty key list in order
 * (GaloisKeys hold N lists, almost all empty, so a per-index hec_seal_kswitch_keys_load would reparse the object N
 * times).  A non-zero return from visit stops the walk, and the function returns that status unchanged (with
 * hec_seal_last_error() = "key list rejected by the caller").  *lists = the object's list count. */
int hec_seal_kswitch_keys_foreach(const void *bytes, uint64_t nbytes,
                                  int (*visit)(void *user, uint64_t index, const uint64_t *words, uint64_t nwords),
                                  void *user, uint64_t *lists, uint64_t *consumed);
/* ... with at most max_bytes decompressed (0: hec_seal_kswitch_keys_default_limit) */
int hec_seal_kswitch_keys_foreach_ex(const void *bytes, uint64_t nbytes, uint64_t max_bytes,
                                     int (*visit)(void *user, uint64_t index, const uint64_t *words, uint64_t nwords),
                                     void *user, uint64_t *lists, uint64_t *consumed);
int hec_seal_kswitch_keys_save(uint64_t poly_modulus_degree, const uint64_t *coeff_modulus, uint64_t K,
                               const uint64_t *const *keys, const uint64_t *digits, uint64_t nlists, int compr_mode,
                               void *out, uint64_t cap, uint64_t *written);
/* device objects: Ciphertext::load(context, ...) (checks N and the parms_id of its level against the context)
 * and Ciphertext::save(stream, compr_mode); RelinKeys::load; GaloisKeys::load (every non-empty key list) */
int hec_ciphertext_load_seal(hec_ciphertext *ct, const void *bytes, uint64_t nbytes, uint64_t *consumed);
int hec_ciphertext_save_seal(const hec_ciphertext *ct, int compr_mode, void *out, uint64_t cap, uint64_t *written);
int hec_kswitch_key_load_seal(hec_context *ctx, const void *bytes, uint64_t nbytes, hec_kswitch_key **out,
                              uint64_t *consumed);
int hec_galois_keys_load_seal(hec_galois_keys *gk, const void *bytes, uint64_t nbytes, uint64_t *consumed);
/* ... with at most max_lists non-empty key lists (0: the default, hec_galois_keys_load_seal_default_lists: four times
 * SEAL's default set of 2 log2(N) - 1, at least 64, at most N, bounded by half the host's available memory; it does
 * not depend on the device).  More lists, or a compressed object that inflates beyond them, is invalid_argument
 * "decompressed SEAL object exceeds the size limit" (the object is inflated in host memory before it is parsed). */
int hec_galois_keys_load_seal_ex(hec_galois_keys *gk, const void *bytes, uint64_t nbytes, uint64_t max_lists,
                                 uint64_t *consumed);
uint64_t hec_galois_keys_load_seal_default_lists(const hec_context *ctx);

/* ---------------------------------------------------------------- primitives (cfg2) ------- */
/* In-place batched negacyclic NTT over device data u64[npolys][nlimbs][N]; limb j uses prime
 * limb0 + j (SEAL ntt_negacyclic_harvey / inverse_ntt_negacyclic_harvey, canonical in/out). */
int hec_ntt_forward(hec_context *ctx, uint64_t *dev_data, uint64_t limb0, uint64_t nlimbs, uint64_t npolys);
int hec_ntt_inverse(hec_context *ctx, uint64_t *dev_data, uint64_t limb0, uint64_t nlimbs, uint64_t npolys);
/* out = a (*) b (dyadic_product_coeffmod), same layout */
int hec_dyadic_multiply(hec_context *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t limb0,
                        uint64_t nlimbs, uint64_t npolys);
/* device memory helpers for the primitive API and tests */
int hec_device_alloc(hec_context *ctx, uint64_t bytes, void **out);
int hec_device_free(hec_context *ctx, void *p);
int hec_memcpy_h2d(hec_context *ctx, void *dst, const void *src, uint64_t bytes);
int hec_memcpy_d2h(hec_context *ctx, void *dst, const void *src, uint64_t bytes);

/* ---------------------------------------------------------------- measurement ------------- */
/* Time `reps` launches of the batched forward NTT on the context stream with HIP events
 * (average ms per launch written to *ms). */
int hec_time_ntt_forward(hec_context *ctx, uint64_t *dev_data, uint64_t nlimbs, uint64_t npolys, int reps,
                         double *ms);
/* Per-kernel-class GPU timing of the engine's phases (ks_intt, ks_modup_a, ks_bmac, ks_moddown, galois,
 * tensor, relin, rescale, ...).  mode 0 off, 1 event pair + synchronize per phase, 2 asynchronous event
 * pairs (no host synchronisation inside calls; resolved by hec_profile_read).  Read cumulative ms and
 * phase counts per class. */
int hec_profile_enable(hec_context *ctx, int mode);
int hec_profile_read(hec_context *ctx, const char *kernel_class, double *total_ms, uint64_t *launches);
/* The same plus the class's algorithmic bytes (compulsory reads + writes of its kernels, summed over its
 * scopes) and kernel launches.  Classes named "k:<kernel>/<role>" wrap single kernels (k_fan, k_ntt, k_bmac,
 * k_hmacm, k_tensor_multi, k_zscan) inside the phases, so bytes / ms is that kernel's achieved GB/s. */
int hec_profile_read_ex(hec_context *ctx, const char *kernel_class, double *total_ms, uint64_t *scopes,
                        double *alg_bytes, uint64_t *kernel_launches);
/* Newline-separated names of every class recorded since hec_profile_enable; returns the bytes needed
 * (including the terminating NUL), writes at most cap bytes into buf when buf != NULL. */
uint64_t hec_profile_classes(hec_context *ctx, char *buf, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* HECDNA_H */
