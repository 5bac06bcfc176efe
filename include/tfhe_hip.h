/*
 * tfhe_hip.h -- C ABI of the MI355X (gfx950) TFHE gate-bootstrapping engine.
 *
 * This is the drop-in boundary for the hot path of thedonutfactory/rs-tfhe:
 *   gate linear prep -> blind rotation -> sample extract -> identity key switch.
 * Conventions follow the reference's only existing FFI, the SPQLIOS wrapper
 * (src/fft/spqlios/spqlios-wrapper.cpp:10-41, Rust decls spqlios_fft.rs:23-34):
 * opaque handle from *_create, freed by *_destroy; caller-owned, caller-allocated
 * flat u32 / f64 buffers passed as raw pointers; no callbacks, no torch types.
 *
 * Each entry point names the reference interface it replaces (paths relative
 * to the rs-tfhe repository root).  The reference has no Result on this path
 * (failure = panic); here every function returns 0 on success or a negative
 * TFHE_HIP_E* code, with tfhe_hip_last_error() giving the text.  A binding that
 * wants the reference's infallible signatures `expect()`s the code.
 *
 * Layouts crossing the boundary (all row-major, little-endian):
 *   TLWELv0     [n+1]  u32      (src/tlwe.rs:12-14)       p[0..n]=a, p[n]=b
 *   TLWELv1     [N+1]  u32      (src/tlwe.rs:217-219)
 *   TRLWELv1    [2][N] u32      (src/trlwe.rs:11-14)      a then b
 *   TRGSWLv1FFT [2l][2][N] f64  (src/trgsw.rs:53-55, src/trlwe.rs:85-88)
 *                                each [N] = re[0..N/2] || im[0..N/2] as produced
 *                                by KlemsaProcessor::ifft (src/fft/klemsa.rs:88-117)
 *   bootstrapping_key  [n] TRGSWLv1FFT                     (src/key.rs:51-56)
 *   key_switching_key  [N][t][base][n+1] u32, index base*t*i + base*j + k
 *                                                          (src/key.rs:102-122)
 * N = 1024 in every parameter set of the reference (src/params.rs).
 *
 * Pointers are HOST pointers unless the function name ends in _dev, in which
 * case they are device pointers on the context's GPU and the call is enqueued
 * on `stream` (a hipStream_t passed as void*; NULL = the context's own non-blocking
 * stream; pass hipStreamLegacy, i.e. (hipStream_t)1, to name the default stream)
 * without synchronising.  Intermediate buffers belong to the context: when a
 * call arrives on a different stream than the previous one, the library first
 * drains the previous stream (hipStreamSynchronize), so mixing streams on one
 * context is safe but serialising; use one context per stream for overlap.
 *
 * Alignment of device pointers.  A 32-bit operand of a _dev call (and a pinned host
 * operand, which the kernels read and write in place) needs 4-byte alignment and no
 * more, an int8 or uint8 operand (weights, gate codes) none: a pointer into the middle
 * of a larger buffer -- row 5 of a batch whose rows are 701 words -- gives the same
 * words as a fresh allocation, and the call writes the words of its output and no
 * other: nothing before its first word, nothing behind its last.  Where a call needs
 * more it says so at the call and refuses a pointer that has less with
 * TFHE_HIP_EINVAL before anything is launched: d0 / d1 / out of
 * tfhe_hip_batch_trlwe_cmux_dev, bodies / out of tfhe_hip_batch_encrypt_trlwe_dev and
 * of tfhe_hip_expand_seeded_trlwe_dev (16 bytes each).
 *
 * Thread safety: a context may be used from several host threads (the
 * reference's `Bootstrap: Send + Sync`, src/bootstrap/mod.rs:23).  Concurrent SMALL
 * host-pointer calls (tfhe_hip_batch_gate / _gates_mixed[_nks] / _bootstrap /
 * _lincomb_bootstrap / _mux / _blind_rotate of up to 2 x #CUs ciphertexts, and their
 * tfhe_hip_pool_* forms) are MERGED: whatever
 * calls arrive while a launch is running share the next one (one launch per key
 * view and operation class, per-ciphertext gate codes / test vectors), so T threads
 * that each evaluate one gate get T gates per launch time, not one -- what a Rayon
 * team calling one strategy expects of its cores (src/parallel/rayon_impl.rs:40-47).
 * Results are the same bits as the unmerged call; a lone caller sees the latency of
 * a one-ciphertext call; errors stay with the thread that caused them.  See
 * tfhe_hip_set_combining.  Every other call on one context is serialised
 * internally, first come first served (a thread that issues calls back to back
 * cannot starve the others).
 */
#ifndef TFHE_HIP_H
#define TFHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFHE_HIP_N 1024

/* error codes */
#define TFHE_HIP_OK 0
#define TFHE_HIP_EINVAL (-1)  /* bad argument / unsupported parameter set */
#define TFHE_HIP_EHIP (-2)    /* a HIP runtime call failed               */
#define TFHE_HIP_ENOKEY (-3)  /* cloud key not loaded                     */
#define TFHE_HIP_ENOMEM (-4)

/* Run-time form of SecurityParams / TrgswParams (src/params.rs:53-84). */
typedef struct tfhe_hip_params {
  int32_t n;       /* tlwe_lv0.n   (<= 1279)            */
  int32_t l;       /* trgsw_lv1.l  (1..3)               */
  int32_t bgbit;   /* trgsw_lv1.bgbit (l*bgbit <= 32)   */
  int32_t basebit; /* trgsw_lv1.basebit                 */
  int32_t t;       /* trgsw_lv1.iks_t (basebit*t <= 31) */
} tfhe_hip_params;

/* Gate selector for tfhe_hip_batch_gate*: the linear prep of src/gates.rs:54-150. */
typedef enum tfhe_hip_gate {
  TFHE_HIP_NAND = 0,   /* gates.rs:54-58   -(a+b), b += 1/8  */
  TFHE_HIP_OR = 1,     /* gates.rs:62-66    a+b,   b += 1/8  */
  TFHE_HIP_AND = 2,    /* gates.rs:70-74    a+b,   b -= 1/8  */
  TFHE_HIP_XOR = 3,    /* gates.rs:78-82    a+2b,  b += 1/4  */
  TFHE_HIP_XNOR = 4,   /* gates.rs:86-90    a-2b,  b -= 1/4  */
  TFHE_HIP_NOR = 5,    /* gates.rs:94-98   -(a+b), b -= 1/8  */
  TFHE_HIP_ANDNY = 6,  /* gates.rs:102-111 -a+b,   b -= 1/8  */
  TFHE_HIP_ANDYN = 7,  /* gates.rs:115-124  a-b,   b -= 1/8  */
  TFHE_HIP_ORNY = 8,   /* gates.rs:128-137 -a+b,   b += 1/8  */
  TFHE_HIP_ORYN = 9,   /* gates.rs:141-150  a-b,   b += 1/8  */
  TFHE_HIP_COPY = 10   /* no prep: plain bootstrap of a (vanilla.rs:40-52) */
} tfhe_hip_gate;

typedef struct tfhe_hip_ctx tfhe_hip_ctx;

/* ---- lifetime ---------------------------------------------------------- */

/* Replaces: FFT_PLAN thread-local construction (src/fft/mod.rs:47-61) and the
 * SPQLIOS precedent Spqlios_new (spqlios-wrapper.cpp:10-13).
 * `device` is the HIP device ordinal this context owns (one context per GPU;
 * one process per GPU under torch.distributed). */
int tfhe_hip_ctx_create(const tfhe_hip_params *params, int device, tfhe_hip_ctx **out);

/* Replaces: Drop for SpqliosFFT (spqlios_fft.rs:84-90). NULL is a no-op. */
void tfhe_hip_ctx_destroy(tfhe_hip_ctx *ctx);

/* Text of the CALLING THREAD's last error on this context (or of its last failed create when ctx == NULL).
 * Never NULL.  The text is kept per (thread, handle): threads that share a context (`Send + Sync`,
 * src/bootstrap/mod.rs:23) each read their own failure, and the pointer stays valid until the same thread's next
 * failing call on the same handle.  A thread that has not failed on the handle reads "" (it never sees another
 * thread's text, and reading stores nothing); a thread's table of texts is bounded: entries of destroyed handles are
 * dropped once it holds 64.  tfhe_hip_pool_last_error follows the same rule. */
const char *tfhe_hip_last_error(const tfhe_hip_ctx *ctx);

/* ---- key views: several resident cloud keys on ONE context -----------------------------------------
 * Replaces: the `&CloudKey` every call of the reference names (src/bootstrap/mod.rs:23-38, src/gates.rs:43-45;
 * strategies and keys are Send + Sync).  A context holds one cloud key of its own; tfhe_hip_key_create adds
 * another resident key to it and returns a KEY VIEW: a tfhe_hip_ctx handle that EVERY entry point of this header
 * accepts in place of the context -- tfhe_hip_load_cloud_key / tfhe_hip_gen_cloud_key* / tfhe_hip_cloud_key_buffers
 * + tfhe_hip_adopt_cloud_key fill the view's key, tfhe_hip_export_cloud_key reads it, every tfhe_hip_batch_* call
 * evaluates under it -- while device, streams, scratch buffers, profiling state and the mutex are the parent's.
 * So a call names its key by the handle it passes; calls under different keys of one context may come from
 * different threads (they serialise on the parent like any two calls on one context) and cost no second set of
 * scratch buffers, streams or twiddle tables.  tfhe_hip_ctx_destroy(view) drains the parent's queued work and
 * frees only the view's key; destroy every view before its parent (a parent destroyed first stays alive, unusable
 * through its own handle, until its last view is destroyed).  tfhe_hip_last_error(view) is the parent's. */
int tfhe_hip_key_create(tfhe_hip_ctx *ctx, tfhe_hip_ctx **key_view);
/* The context a key view runs on (the handle itself for a plain context). */
tfhe_hip_ctx *tfhe_hip_key_parent(tfhe_hip_ctx *key_view);
/* 1 when the handle's own key has been loaded / generated / adopted, else 0. */
int tfhe_hip_key_is_loaded(tfhe_hip_ctx *ctx_or_view);

/* "MI355X-native HIP (gfx950)" style identification: Bootstrap::name()
 * (src/bootstrap/mod.rs:37) of the strategy this library backs. */
const char *tfhe_hip_name(void);
/* Number of GPUs this process can open (hipGetDeviceCount; 0 when there is none or the runtime cannot start): what a
 * host binding needs to build "all GPUs of the node" for tfhe_hip_pool_create -- the stand-in for Rayon's default
 * "one worker per logical CPU" (src/parallel/rayon_impl.rs:15-27).  Does not initialise any device. */
int tfhe_hip_device_count(void);

/* ---- cloud key --------------------------------------------------------- */

/* Replaces: borrowing `&CloudKey` on every call (src/key.rs:51-56).  Uploads
 * and converts the key once; host buffers may be freed on return.
 *   bsk            [n][2l][2][N] f64, reference Klemsa spectral layout
 *   ksk            [N][t][base][n+1] u32 (k = 0 slots are ignored)
 *   decomp_offset  CloudKey::decomposition_offset (key.rs:78-89)
 *   testvec        CloudKey::blind_rotate_testvec [2][N] (key.rs:91-100) */
int tfhe_hip_load_cloud_key(tfhe_hip_ctx *ctx, const double *bsk, const uint32_t *ksk,
                            uint32_t decomp_offset, const uint32_t *testvec);

/* Replaces: CloudKey::new(&secret_key) (src/key.rs:59-66) = gen_decomposition_offset (:78-89),
 * gen_testvec (:91-100), gen_key_switching_key (:102-122) and gen_bootstrapping_key (:124-156),
 * generated on the GPU straight into the context (no upload).  Needs the secret key, so it is a
 * client-side call.  key_lv0 [n], key_lv1 [N]: 0/1 words (src/key.rs:21-49).
 * alpha_ksk = tlwe_lv0.alpha (KSK_ALPHA, params.rs:468), alpha_bsk = tlwe_lv1.alpha (BSK_ALPHA,
 * :469).
 *
 * Randomness.  The reference draws every mask word and noise sample from an OS-seeded ChaCha thread_rng
 * (tlwe.rs:38, trlwe.rs:36-41).  Here they are fixed positions of a ChaCha20 keystream (RFC 8439, 20 rounds)
 * under a 256-bit generator key; the distributions are the reference's.  A published cloud key is only as
 * secret as that generator key -- whoever can regenerate the noise solves the key rows for the secret key --
 * so:
 *   tfhe_hip_gen_cloud_key_secure    the generator key comes from getrandom(2).  USE THIS ONE.
 *   tfhe_hip_gen_cloud_key_with_key  the caller supplies 32 bytes from its own CSPRNG (e.g. Rust's OsRng).
 *   tfhe_hip_gen_cloud_key           TEST / BENCHMARK ONLY: a 64-bit seed is expanded into the generator key,
 *                                    which makes the cloud key reproducible bit for bit and exactly as
 *                                    guessable as the seed.  Never publish a key generated this way.
 * What the device holds of the secret keys and of the generator key is zeroed before any of the three returns. */
int tfhe_hip_gen_cloud_key_secure(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1,
                                  double alpha_ksk, double alpha_bsk);
int tfhe_hip_gen_cloud_key_with_key(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1,
                                    double alpha_ksk, double alpha_bsk, const uint8_t rng_key[32]);
int tfhe_hip_gen_cloud_key(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1,
                           double alpha_ksk, double alpha_bsk, uint64_t seed);

/* The loaded / generated cloud key back in the reference layouts of tfhe_hip_load_cloud_key
 * (any pointer may be NULL to skip that field).  load -> export is the identity. */
int tfhe_hip_export_cloud_key(tfhe_hip_ctx *ctx, double *bsk, uint32_t *ksk, uint32_t *decomp_offset,
                              uint32_t *testvec);

/* The context's cloud key as raw device buffers in the ENGINE layouts, for callers that
 * replicate a key device to device themselves -- one process per GPU, where the pool's hipMemcpyPeer cannot reach:
 * the owner of the key and every receiver call this (it allocates the buffers when the context has none yet),
 * the bytes travel (RCCL broadcast, hipMemcpyPeer, IPC), and each receiver then calls
 * tfhe_hip_adopt_cloud_key(ctx, decomp_offset of the owner).  The buffers stay owned by the context; while a
 * receiver's buffers are being written it must not run batches.  Any out pointer may be NULL. */
int tfhe_hip_cloud_key_buffers(tfhe_hip_ctx *ctx, void **bsk, size_t *bsk_bytes, void **ksk, size_t *ksk_bytes,
                               void **testvec, size_t *testvec_bytes, uint32_t *decomp_offset);
int tfhe_hip_adopt_cloud_key(tfhe_hip_ctx *ctx, uint32_t decomp_offset);

/* ---- seeded (compressed) cloud keys and ciphertexts ----------------------
 *
 * Nearly every byte of a cloud key is pseudorandom mask: every KSK row, every TRLWE row of the BSK and every fresh
 * TLWE ciphertext is (uniform mask, body).  Here the masks are fixed positions of a ChaCha20 keystream under a
 * PUBLIC 32-byte mask seed S, so only the bodies travel and the device regenerates the masks: 17.35 MB instead of
 * 172.2 MB on SECURITY_128_BIT, 7.11 MB instead of 349.7 MB on SECURITY_UINT4.  The expanded key is an ordinary
 * cloud key: every other entry point runs it unchanged, and tfhe_hip_export_cloud_key returns it in full.
 *
 * Format (normative).  All keystream words are the RFC 8439 ChaCha20 block function, 20 rounds,
 * block(key, counter, nonce n0, n1, n2).  A 32-byte seed is read as 8 little-endian u32 key words.  Word x of a row
 * is word x mod 16 of the block with counter x / 16.
 *   Mask seed S    32 bytes, public, shipped with the key.
 *   KSK row r = base*t*i + base*j + k, k >= 1: mask words x < n under S, nonce (r, 16, 0x4B534B); body
 *                  <a, s0> + gaussian_f64(k * s1[i] / 2^((j+1) basebit)).  k = 0 rows are zero; their body
 *                  slots are written 0 and ignored on load.
 *   BSK row r = i*2l + q of TRGSW(s0[i]): mask polynomial a, coefficients c < N under S, nonce (r, 18, 0x42534B).
 *                  With p = s0[i] and g_d = f64_to_torus(Bg^-(d+1)) the body is
 *                    q <  l: b = a (*) s1 + e - p*g_q*s1   (every coefficient of s1 scaled by p*g_q, wrapping)
 *                    q >= l: b = a (*) s1 + e + p*g_{q-l}  (on coefficient 0).
 *                  The reference adds the gadget to a[0] in the q < l rows; with a public mask that would publish
 *                  s0[i].  Folding -p*g_q*s1 into the body instead gives the same distribution (a - p*g is uniform)
 *                  and the same phase, so the external product is unchanged.
 *   Generator key K (secret; generation only).  S = words 0..7 of block(K, 0, 0, 20, 0x444553), a PRF output that
 *                  reveals nothing of K.  Noise: Box-Muller over the keystream under K, nonce (r, 17, 0x4B534B) for
 *                  the KSK and (r, 19, 0x42534B) for the BSK.  These streams differ from the ones
 *                  tfhe_hip_gen_cloud_key* use (1 and 3) ON PURPOSE: one K given to both entry points must not give
 *                  two published keys with equal noise, whose difference would reveal the secret key.
 *   Seeded TLWE lv0 (S, first_index, bodies[count]): ciphertext g = first_index + m has mask words under S, nonce
 *                  (g & 0xffffffff, g >> 32, 0x45574C), and the body encrypt_f64 computes for that mask.
 *                  NEVER reuse an (S, index) pair for two messages: the difference of their bodies is the difference
 *                  of the messages plus noise.
 *
 * Layouts: bsk_bodies [n][2l][N] u32, ksk_bodies [N][t][base] u32 (tfhe_hip_compressed_key_words gives both sizes). */

/* Word counts of bsk_bodies and ksk_bodies for `params`.  Initialises no device. */
int tfhe_hip_compressed_key_words(const tfhe_hip_params *params, size_t *bsk_words, size_t *ksk_words);
/* The compressed key of the secret key (key_lv0, key_lv1), as tfhe_hip_gen_cloud_key_with_key takes them: writes S
 * to mask_seed, the bodies and the decomposition offset, and leaves ctx (or the key view) loaded with the expanded
 * key -- bit for bit the key tfhe_hip_load_compressed_cloud_key rebuilds from the outputs.  rng_key: the generator
 * key K from the caller's CSPRNG, or NULL to draw it from getrandom(2).  The test vector is gen_testvec's. */
int tfhe_hip_gen_compressed_cloud_key(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1,
                                      double alpha_ksk, double alpha_bsk, const uint8_t rng_key[32],
                                      uint8_t mask_seed[32], uint32_t *bsk_bodies, uint32_t *ksk_bodies,
                                      uint32_t *decomp_offset);
/* tfhe_hip_load_cloud_key from the compressed form: uploads the bodies only and expands them on the device. */
int tfhe_hip_load_compressed_cloud_key(tfhe_hip_ctx *ctx, const uint8_t mask_seed[32], const uint32_t *bsk_bodies,
                                       const uint32_t *ksk_bodies, uint32_t decomp_offset, const uint32_t *testvec);
/* Seeded TLWE lv0 ciphertexts (S, first_index, bodies[count]) expanded to [count][n+1] words.  Needs no cloud key.
 * _dev: device pointers, queued on `stream` (NULL: the context's stream) like the other *_dev entry points. */
int tfhe_hip_expand_seeded_tlwe(tfhe_hip_ctx *ctx, const uint8_t mask_seed[32], uint64_t first_index,
                                const uint32_t *bodies, size_t count, uint32_t *out);
int tfhe_hip_expand_seeded_tlwe_dev(tfhe_hip_ctx *ctx, const uint8_t mask_seed[32], uint64_t first_index,
                                    const uint32_t *bodies, size_t count, uint32_t *out, void *stream);

/* ---- packing key switch: up to N = 1024 lv0 results in one TRLWE lv1 ------
 *
 * A result leaves the server as an (n+1)-word TLWE lv0 (2,804 bytes on SECURITY_128_BIT).  A TRLWE lv1 is 2N words
 * (8 KiB) and each of its N coefficients can carry the phase of one LWE: the packing key switch (LWE -> GLWE key
 * switching) turns a batch of lv0 results into ceil(count / N) TRLWEs that the client decrypts with the s1 it holds,
 * 350x fewer bytes on SECURITY_128_BIT and 410x on UINT4.
 *
 * Definition (normative).  From the context's set: n, N = 1024, beta = basebit (<= 7: the digits fit in a byte),
 * t = iks_t, B = 2^beta, g_l = 2^(32 - (l+1) beta).
 *   Packing key.  One TRLWE lv1 row under s1 for each (i < n, l < t), row r = i*t + l:
 *     a_r  N keystream words under a public 32-byte mask seed S (RFC 8439 block, word x = word x mod 16 of counter
 *          x / 16, as in the seeded section), nonce (r, 24, 0x504B53);
 *     b_r  = a_r (*) s1 + e_r + s0[i]*g_l*X^0, every coefficient mod 2^32, e_r = f64_to_torus(N(0, alpha)) per
 *          coefficient (alpha: alpha_lv1 of the set by default).
 *   Only the bodies travel: bodies [n][t][N] u32 (25.8 MB on SECURITY_128_BIT, 15.8 MB on 80-bit, 10.1 MB on UINT4,
 *   14.3 MB on UINT8).  The key encrypts bits of s0 under s1, exactly as the BSK does: it adds no new security
 *   assumption.
 *   Digits.  The identity key switch's rounding, then a signed decomposition:
 *     a_bar = ((a + 2^(31 - beta t)) mod 2^32) >> (32 - beta t);  carry = 0;
 *     for l = t-1 down to 0: v = ((a_bar >> beta(t-1-l)) & (B-1)) + carry;
 *                            v >= B/2 ? (d_l = v - B, carry = 1) : (d_l = v, carry = 0)     (the last carry is dropped)
 *     so d_l in [-B/2, B/2) and sum_l d_l g_l = a_bar 2^(32 - beta t) (mod 2^32).
 *   Pack.  Input c_m = (a_m, b_m), m < count, lands in group G = m / N, slot j = m mod N.  Per group, with
 *   D_{i,l}(X) = sum_j d_l(a_j[i]) X^j over the group's inputs:
 *     A = - sum_{i,l} D_{i,l} (*) a_{i,l},    B = sum_j b_j X^j - sum_{i,l} D_{i,l} (*) b_{i,l}
 *   negacyclic mod X^N + 1, wrapping mod 2^32.  Output [ceil(count / N)][2][N] u32, a row then b row (the layout of
 *   tfhe_hip_batch_blind_rotate).  Coefficient j of B - A (*) s1 is the phase of c_j plus the rounding error and the key
 *   noise; unused slots of the last group hold phase 0 plus noise.  The result is defined in integers: every device
 *   and parameter set gives these words exactly.
 * Semantics.  The packing key lives beside the cloud key of a context or key view: loading, generating or adopting a
 * cloud key (or loading a re-encryption key) leaves it, packing needs no cloud key, destroying a view frees its key.
 * Packing without one: TFHE_HIP_ENOKEY.  Packing calls are bulk calls (the context's mutex, never the combining
 * front end).  _dev: device pointers, queued on `stream` (NULL: the context's stream).
 *
 * Generation (normative).  tfhe_hip_gen_packing_key makes the key above on the device from the secret key and a
 * 32-byte generator key K (secret; generation only), so the whole key is a function of (s0, s1, K, alpha):
 *   Mask seed   S = words 0..7 of block(K, counter 0, nonce (0, 26, 0x444553)), a PRF output that reveals nothing of K.
 *               Stream 26 is not the compressed cloud key's stream 20 ON PURPOSE: one K gives two different public
 *               seeds.
 *   Noise       e_r under K, nonce (r, 25, 0x504B53), in the BSK generators' word order: block 2*lane + h (lane < 64,
 *               h < 2) holds four pairs; pair m < 4 is Box-Muller over words 4m..4m+3 of the block (the gauss2 of the
 *               seeded section's noise); its first sample is e[lane + 64(4h + m)], its second the same + 512;
 *               e = f64_to_torus(sample).
 *   Product     a_r (*) s1 is exact: the mask read as int32, s1 binary, N = 1024 terms, |coefficient| < 2^41.  The
 *               gadget s0[i]*g_l is added to coefficient 0 after the product, wrapping mod 2^32.
 *   Sharing K   One K may be given to this call, to tfhe_hip_gen_compressed_cloud_key and to
 *               tfhe_hip_gen_cloud_key_with_key: every noise stream differs (1, 3, 17, 19, 25), so no two published
 *               rows share a noise sample.
 * Away from samples that sit within rounding of a torus step (where two correct f64 libms may truncate to neighbouring
 * words) every implementation of this section gives the same bodies. */
/* Word count of `bodies` for `params`.  Initialises no device. */
int tfhe_hip_packing_key_words(const tfhe_hip_params *params, size_t *body_words);
/* Uploads the bodies and expands the key on the device (masks from S, then the kernel's byte planes). */
int tfhe_hip_load_packing_key(tfhe_hip_ctx *ctx, const uint8_t mask_seed[32], const uint32_t *bodies);
/* The packing key of the secret key (key_lv0 [n], key_lv1 [N], as tfhe_hip_gen_cloud_key_with_key takes them), made on
 * the device.  A CLIENT-side call, like tfhe_hip_gen_cloud_key*: it takes the secret key.  Writes S to mask_seed and,
 * unless `bodies` is NULL, the bodies [n][t][N]; the handle (context or key view) is left holding the key -- bit for
 * bit the one tfhe_hip_load_packing_key(mask_seed, bodies) builds from the outputs.  alpha: the noise's standard
 * deviation (alpha_lv1 of the set is the usual choice).  rng_key: K from the caller's CSPRNG, or NULL to draw it from
 * getrandom(2).  Needs no cloud key and leaves a loaded one alone.  TFHE_HIP_EINVAL (the previous packing key stays
 * loaded) for a NULL secret key or mask_seed, basebit > 7, alpha negative or NaN. */
int tfhe_hip_gen_packing_key(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha,
                             const uint8_t rng_key[32], uint8_t mask_seed[32], uint32_t *bodies);
/* 0 / 1, never an error code (no device call is made). */
int tfhe_hip_packing_key_is_loaded(tfhe_hip_ctx *ctx);
/* in [count][n+1] lv0 ciphertexts -> out [ceil(count / N)][2][N]. */
int tfhe_hip_batch_pack_tlwe(tfhe_hip_ctx *ctx, const uint32_t *in, size_t count, uint32_t *out);
int tfhe_hip_batch_pack_tlwe_dev(tfhe_hip_ctx *ctx, const uint32_t *in, size_t count, uint32_t *out, void *stream);

/* ---- unpacking key switch: slots of TRLWE lv1 ciphertexts back to lv0 ciphertexts ------
 *
 * The way back from the packed form: any slots of TRLWE lv1 ciphertexts under s1 -- what tfhe_hip_batch_pack_tlwe
 * wrote, or what a client encrypted itself (TRLWELv1::encrypt_bool, trlwe.rs:55-66) -- become TLWE lv0 ciphertexts
 * under s0 that the gate, mux, LUT and circuit calls accept.  State can so stay resident at 8 bytes a slot instead of
 * 4(n+1) (2,804 on SECURITY_128_BIT), and a client can upload 1,024 values in one 8 KiB ciphertext.
 *
 * Definition (normative).  N = 1024, n of the context's set.
 *   trlwe  [groups][2][N] u32, the a row then the b row of each group (the layout tfhe_hip_batch_pack_tlwe writes).
 *   Output m < count takes slot s = slots ? slots[m] : m, group G = s / N, coefficient j = s % N.
 *   The lv1 row of the slot, trlwe::sample_extract_index(trlwe_G, j) (trlwe.rs:106-120):
 *     r[i] = a_G[j - i]                     for i <= j,
 *     r[i] = 2^32 - 1 - a_G[N + j - i]      for j < i < N   (Torus::MAX - a: the reference's negation, one LSB below
 *                                                            0 - a; tfhe_hip_batch_sample_extract does the same),
 *     r[N] = b_G[j].
 *   out[m] = trgsw::identity_key_switching(r) (trgsw.rs:332-360) under the handle's cloud key: the words
 *   tfhe_hip_batch_identity_key_switch returns for r.  out is [count][n+1] u32.
 *   Both steps are integer arithmetic: every device, key-switch kernel and parameter set gives these words exactly.
 *   The phase of out[m] is coefficient j of b_G - a_G (*) s1 plus the key switch's rounding error and key noise.
 * Semantics.  The call needs the cloud key (its key-switching key) and no packing key: TFHE_HIP_ENOKEY on a handle
 * without a cloud key, a handle that holds a re-encryption key included.  count == 0 returns TFHE_HIP_OK.  Null trlwe
 * or out with count > 0: TFHE_HIP_EINVAL.  With slots NULL, count <= groups * N (else TFHE_HIP_EINVAL) and only the
 * first ceil(count / N) groups are read.  With slots given, every entry is < groups * N; duplicates and any order are
 * allowed.  The host-pointer form checks the entries and returns TFHE_HIP_EINVAL for one out of range.  The _dev form
 * only enqueues and cannot look at device memory without stalling: there the caller guarantees the range (an entry out
 * of range reads nothing and its output is the key switch of an all-zero row, not an error).  Unpacking calls are
 * bulk calls (the context's mutex, never the combining front end).  _dev: device pointers, slots included, queued on
 * `stream` (NULL: the context's stream); the rows pass through the context's lv1 scratch like a bootstrap's, and
 * TFHE_HIP_KS_KERNEL and the automatic choice of the key-switch kernel apply as they do there. */
int tfhe_hip_batch_unpack_trlwe(tfhe_hip_ctx *ctx, const uint32_t *trlwe, size_t groups, const uint32_t *slots,
                                size_t count, uint32_t *out);
int tfhe_hip_batch_unpack_trlwe_dev(tfhe_hip_ctx *ctx, const uint32_t *trlwe, size_t groups, const uint32_t *slots,
                                    size_t count, uint32_t *out, void *stream);

/* ---- encrypted linear layers: a plaintext int8 matrix times LWE ciphertexts or the slots of a TRLWE ------
 *
 * The linear step between bootstraps: y = W x + bias with a plaintext matrix W and encrypted x, for every one of
 * `groups` independent inputs (the samples of a batch).  On a binary-key torus scheme this is exact integer arithmetic
 * mod 2^32; it runs on the matrix cores (csrc/matmul.hpp) and needs no key unless the packed form is asked for the
 * final lv1 -> lv0 key switch.
 *
 * Definition (normative).  N = 1024, n of the context's set; all sums in wrapping u32 arithmetic.
 *   w     [rows][cols] int8, row-major.      bias  [rows] u32 torus words, or NULL for zero.
 * Dense form (tfhe_hip_batch_tlwe_matmul).  in [groups][cols][n+1], out [groups][rows][n+1]; for every word x <= n
 *     out[g][r][x] = sum_{j < cols} (int32)w[r][j] * in[g][j][x]  +  (x == n ? bias[r] : 0).
 *   1 <= cols <= 65,536 (each byte-plane accumulator of the kernel then stays at or below cols * 2^14 <= 2^30).
 * Packed form (tfhe_hip_batch_trlwe_matmul).  trlwe [groups][2][N], the a row then the b row (the layout
 *   tfhe_hip_batch_pack_tlwe writes); w acts on slots 0 .. cols-1 of every group, 1 <= cols <= N.  E_g[j], the lv1
 *   extraction of slot j of group g with the EXACT wrapping negation:
 *     E[j][i] = a[j - i]            for i <= j,
 *     E[j][i] = 0 - a[N + j - i]    for j < i < N,
 *     E[j][N] = b[j].
 *   This is deliberately not the Torus::MAX - a of the unpacking key switch and tfhe_hip_batch_sample_extract (the
 *   reference's negation), which is one LSB low per negated word: multiplied by the weights that would add the
 *   deterministic phase offset sum_i s1[i] * sum_{j < i} w[r][j], up to 2^26 LSB -- 1/64 of the torus -- at cols = 1024
 *   and weights of 127.
 *     lv1[g][r][x] = sum_{j < cols} (int32)w[r][j] * E_g[j][x]  +  (x == N ? bias[r] : 0).
 *   keyswitch == 0: out is [groups][rows][N+1] and holds these rows (ciphertexts under s1); no key is needed.
 *   keyswitch != 0: out is [groups][rows][n+1] and holds trgsw::identity_key_switching (trgsw.rs:332-360) of them
 *   under the handle's cloud key -- the words tfhe_hip_batch_identity_key_switch returns for the rows.  The rows pass
 *   through the context's lv1 scratch like a bootstrap's, and TFHE_HIP_KS_KERNEL and the automatic choice of the
 *   key-switch kernel apply as they do there.  TFHE_HIP_ENOKEY on a handle without a cloud key.
 * Consequences.  Before any key switch the phase of an output row is sum_j w[r][j] * phase(input j) + bias[r], exactly,
 *   mod 2^32 (input j: in[g][j], or slot j of trlwe[g]); the noise variance scales by sum_j w[r][j]^2.  Under the
 *   (msg mod m) / (2m) encoding the sum of the messages is therefore taken mod 2m on the torus.  Weights wider than int8
 *   are the caller's affair: split them into int8 limbs and combine the products with tfhe_hip_batch_tlwe_lincomb.
 * Semantics.  rows >= 1 and rows * groups <= 2^31 - 1.  TFHE_HIP_EINVAL for rows == 0, cols out of range, a NULL w,
 *   in / trlwe or out (with groups > 0) and rows * groups too large; groups == 0 with valid rows and cols returns
 *   TFHE_HIP_OK and writes nothing.  out must not overlap the input.  The calls are bulk calls (the context's mutex and
 *   the one staging path of the host-pointer forms, never the combining front end).  _dev: every pointer, w and bias
 *   included, is device memory; the call is queued on `stream` (NULL: the context's stream).  w needs no alignment
 *   (rows that start on 16-byte boundaries -- cols a multiple of 16 -- load fastest). */
int tfhe_hip_batch_tlwe_matmul(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols,
                               const uint32_t *in, size_t groups, uint32_t *out);
int tfhe_hip_batch_tlwe_matmul_dev(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols,
                                   const uint32_t *in, size_t groups, uint32_t *out, void *stream);
int tfhe_hip_batch_trlwe_matmul(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols,
                                const uint32_t *trlwe, size_t groups, int keyswitch, uint32_t *out);
int tfhe_hip_batch_trlwe_matmul_dev(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols,
                                    const uint32_t *trlwe, size_t groups, int keyswitch, uint32_t *out, void *stream);

/* ---- plaintext polynomial products on packed ciphertexts: TRLWE in, TRLWE out ------
 *
 * The module operation of a packed ciphertext: out(X) = sum_j w_j(X) * ct_j(X) + bias(X) mod X^N + 1 with plaintext
 * int8 polynomials w_j.  Input and output are both TRLWE lv1 ciphertexts, so the result stays packed: it can go into
 * tfhe_hip_batch_unpack_trlwe (chosen slots -> lv0 ciphertexts), tfhe_hip_batch_decrypt_trlwe, the bivariate bootstrap
 * or another product.  The product with +-X^k rotates the slots with the negacyclic sign (no Galois key); a feature map
 * of up to N values in ONE ciphertext times one polynomial per filter is a packed 2-D convolution (the encoding:
 * rs_tfhe_amd.linear.conv2d_packed_plan).  Exact integer arithmetic mod 2^32 on the matrix cores (csrc/matmul.hpp,
 * MmNegacyclic).  This is not tfhe_hip_batch_poly_mul, the inexact f64 FFT stage kernel of the parity tests.
 *
 * Definition (normative).  N = 1024; all sums in wrapping u32 arithmetic.
 *   w     [rows][cols][N] int8: the coefficients of rows x cols plaintext polynomials.
 *   bias  [rows][N] u32 torus words, a plaintext polynomial per output, or NULL for zero.
 *   trlwe [groups][cols][2][N], the a row then the b row of each (the layout tfhe_hip_batch_pack_tlwe and
 *         tfhe_hip_batch_encrypt_trlwe write).        out  [groups][rows][2][N].
 *   For a polynomial p: ext_p[t] = p[t] for 0 <= t < N, ext_p[t] = 0 - p[N + t] for -N < t < 0 -- the EXACT wrapping
 *   negation, as in the packed matmul, not Torus::MAX - a.  For component c in {a, b} and coefficient i:
 *     out[g][r][c][i] = sum_{j < cols} sum_{m < N} (int32)w[r][j][m] * ext_{in[g][j][c]}[i - m]
 *                       + (c == b ? bias[r][i] : 0).
 * Consequences.  The phase polynomial of out[g][r] is sum_j w[r][j](X) * phase(in[g][j])(X) + bias[r](X), exactly,
 *   mod 2^32 (the phase b - a s is linear in (a, b) over Z[X] / (X^N + 1), and a plaintext factor commutes with s).
 *   The noise variance of every slot scales by sum_j sum_m w[r][j][m]^2.  1 <= cols <= 64: the product is a GEMM with
 *   K = cols * N weights per output word, and each byte-plane accumulator of the kernel is a sum of K products of two
 *   signed bytes, |acc| <= K * 128 * 128 = cols * 2^24 <= 2^30 < 2^31 for cols <= 64 (K <= 65,536, the dense form's
 *   bound).  No key is needed.
 * Semantics.  As tfhe_hip_batch_trlwe_matmul: rows >= 1 and rows * groups <= 2^31 - 1.  TFHE_HIP_EINVAL for rows == 0,
 *   cols out of range, a NULL w, trlwe or out (with groups > 0) and rows * groups too large; groups == 0 with valid
 *   rows and cols returns TFHE_HIP_OK and writes nothing.  out must not overlap trlwe (not checked).  Bulk calls (the
 *   context's mutex and the one staging path of the host-pointer form, never the combining front end).  _dev: every
 *   pointer, w and bias included, is device memory; the call is queued on `stream` (NULL: the context's stream).  w
 *   needs no alignment (a 16-byte aligned w loads fastest).  A workgroup computes 64 rows: fewer rows cost the same
 *   (profiles/polymul_bench.json). */
int tfhe_hip_batch_trlwe_polymul(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols,
                                 const uint32_t *trlwe, size_t groups, uint32_t *out);
int tfhe_hip_batch_trlwe_polymul_dev(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols,
                                     const uint32_t *trlwe, size_t groups, uint32_t *out, void *stream);

/* ---- TRLWE key switch: packed re-encryption and slot automorphisms ------
 *
 * The one operation that takes a TRLWE lv1 under one ring key to a TRLWE lv1 under another.  With psi_k the
 * automorphism X -> X^k, a key that encrypts g_l * psi_k(s_from) under s_to takes a ciphertext under s_from to the
 * ciphertext of psi_k(phase) under s_to.  k = 1 with s_from != s_to is packed proxy re-encryption: 1,024 values in one
 * step per 8 KiB ciphertext, where tfhe_hip_batch_reencrypt takes 2,804 bytes per value.  k != 1 with
 * s_from = s_to = s1 is a Galois key: ct(X) -> ct(X^k) permutes the slots beyond the rotations of a product with
 * +-X^k, and the chain ct <- ct + switch_k(ct) over k = N/2^(s-1) + 1, s = 1 .. steps, is the partial trace that
 * clears the by-product slots of a packed product (rs_tfhe_amd.packing.trace).
 *
 * Definition (normative).  N = 1024; all arithmetic wraps mod 2^32; negation is the exact 0 - x, as in the packed
 * matmul, not Torus::MAX - x.
 *   Automorphism.  psi_k, k odd, 1 <= k < 2N, of a polynomial p: coefficient j goes to position j k mod 2N; a position
 *     P >= N is position P - N with the value negated.  psi_1 is the identity; psi_k psi_k' = psi_(k k' mod 2N).
 *   Switching key for (k, beta, t): 1 <= beta <= 7 (B = 2^beta; the negated digits fit a signed byte), 1 <= t <= 64
 *     (K = t N <= 65,536 keeps the byte-plane accumulators of the product at or below 2^30) and beta t <= 32.  t TRLWE
 *     rows under s_to; row l < t, with g_l = 2^(32 - (l+1) beta):
 *       a_l  N keystream words under a public 32-byte mask seed S (RFC 8439 block, word x = word x mod 16 of counter
 *            x / 16, natural order, as for the packing key), nonce (64 k + l, 27, 0x544B53);
 *       b_l  = a_l (*) s_to + e_l + g_l * psi_k(s_from), every coefficient mod 2^32, the gadget polynomial added after
 *            the product; e_l = f64_to_torus(N(0, alpha)) per coefficient.
 *     Only the bodies travel: bodies [t][N] u32 (24 KiB at t = 6).
 *   Digits of a word x.  The packing key switch's rounding and decomposition ("packing key switch", Digits) with this
 *     key's (beta, t): a_bar, the carry chain and d_l in [-B/2, B/2), sum_l d_l g_l = a_bar 2^(32 - beta t).  At
 *     beta t = 32 nothing is rounded: a_bar = x.
 *   Switch.  For ct = (a, b):  a' = psi_k(a), b' = psi_k(b), D_l(X) = sum_j d_l(a'[j]) X^j,
 *       out.a = - sum_l D_l (*) a_l,        out.b = b' - sum_l D_l (*) b_l        (negacyclic mod X^N + 1).
 *     in and out are [count][2][N] u32, the a row then the b row of each.
 * Consequences.  The phase out.b - out.a (*) s_to equals psi_k(b - a (*) s_from) plus a rounding error and the key
 *   noise.  With a binary key of about N/2 ones, per coefficient the rounding error has variance about
 *   (N/2) * 2^(-2 beta t) / 12 and the key noise about N * t * (B^2 / 12) * alpha^2 (torus units squared).  The result
 *   is defined in integers: every device gives these words exactly.  A ten-step trace (ct <- ct + switch(ct), ten
 *   times) multiplies what it keeps by 2^10 and leaves noise of variance 4^10 (V_in + V_switch / 3).  Safe choices -- 8
 *   standard deviations of (a fresh encryption at alpha_lv1 plus the switches) inside the decoding half-interval, 1/8
 *   for a boolean and 1/64 for an m = 16 message, key noise at alpha_lv1 of the set (DESIGN.md section 9 has the table):
 *     one switch           (4, 6) on every set, booleans and m = 16 (8 sigma <= 1.1e-4).
 *     ten-step trace, bool (4, 6) on every set (8 sigma <= 0.064 on SECURITY_80_BIT).
 *     ten-step trace, m=16 (4, 6) on SECURITY_UINT2 .. UINT8 (8 sigma = 1.8e-3); (2, 12) on SECURITY_128_BIT and UINT1
 *                          (1.2e-2; (4, 6) gives 3.4e-2: not safe); (1, 24) on SECURITY_110_BIT (1.3e-2); none on
 *                          SECURITY_80_BIT ((1, 24) gives 1.61e-2 against 1.56e-2): take m = 8 there.
 * Generation (normative).  Under a 32-byte generator key K (secret; generation only):
 *   Mask seed   S = words 0..7 of block(K, counter 0, nonce (0, 29, 0x444553)).
 *   Noise       e_l under K, nonce (64 k + l, 28, 0x544B53), in the BSK generators' word order, as for the packing key.
 *   Product     a_l (*) s_to is exact (|coefficient| < 2^41).
 *   Sharing K   One K serves ONE key per k: the nonce row 64 k + l (l < 64) gives every (k, l) its own noise sample,
 *               and streams 27 / 28 / 29 are no other generator's, so the same K may also be given to
 *               tfhe_hip_gen_packing_key and the cloud-key generators.  Two keys for the same k under one K (another
 *               (beta, t), or other secrets) would share noise samples: use another K.
 *   Away from samples that sit within rounding of a torus step every implementation gives the same bodies.
 * Semantics.  A context or key view holds up to 16 switching keys, found by k, each with its own (beta, t); the k = 1
 *   entry is the re-encryption key.  They live beside the cloud key like the packing key: loading or generating a
 *   cloud key leaves them, destroying a view frees them.  A switch needs no other key.  TFHE_HIP_ENOKEY when no key
 *   for k is loaded (switch, drop).  TFHE_HIP_EINVAL, with the previous entry for k still loaded and answering: k even
 *   or out of range, beta or t out of range or beta t > 32, a seventeenth key, NULL pointers (with count > 0 for the
 *   switch), alpha negative or NaN, count > 2^31 - 1.  count == 0 returns TFHE_HIP_OK and writes nothing.  out must not
 *   overlap in (the _dev form does not check it).  Bulk calls: the context's mutex and the one staging path of the
 *   host-pointer form, never the combining front end.  _dev: device pointers, queued on `stream` (NULL: the context's
 *   stream); the digits pass through a scratch of the context, 2,048 ciphertexts a pass.  There are no pool forms. */
/* Word count of `bodies` for t rows.  Initialises no device. */
int tfhe_hip_trlwe_switch_key_words(int t, size_t *body_words);
/* The switching key (k, basebit, t) from key_from_lv1 [N] to key_to_lv1 [N], made on the device.  A CLIENT-side call: it
 * takes secret keys.  Writes S to mask_seed and, unless `bodies` is NULL, the bodies [t][N]; the handle is left holding
 * the key -- bit for bit the one tfhe_hip_load_trlwe_switch_key(k, basebit, t, mask_seed, bodies) builds from the
 * outputs.  rng_key: K from the caller's CSPRNG, or NULL to draw it from getrandom(2). */
int tfhe_hip_gen_trlwe_switch_key(tfhe_hip_ctx *ctx, const uint32_t *key_from_lv1, const uint32_t *key_to_lv1, int k,
                                  int basebit, int t, double alpha, const uint8_t rng_key[32], uint8_t mask_seed[32],
                                  uint32_t *bodies);
/* Uploads the bodies and expands the key on the device (masks from S). */
int tfhe_hip_load_trlwe_switch_key(tfhe_hip_ctx *ctx, int k, int basebit, int t, const uint8_t mask_seed[32],
                                   const uint32_t *bodies);
/* 0 / 1, never an error code (no device call is made). */
int tfhe_hip_trlwe_switch_key_is_loaded(tfhe_hip_ctx *ctx, int k);
/* Frees the key for k. */
int tfhe_hip_drop_trlwe_switch_key(tfhe_hip_ctx *ctx, int k);
/* in [count][2][N] -> out [count][2][N] under the key for k. */
int tfhe_hip_batch_trlwe_keyswitch(tfhe_hip_ctx *ctx, int k, const uint32_t *in, size_t count, uint32_t *out);
int tfhe_hip_batch_trlwe_keyswitch_dev(tfhe_hip_ctx *ctx, int k, const uint32_t *in, size_t count, uint32_t *out,
                                       void *stream);
/* While profiling is enabled (tfhe_hip_set_profiling) the two steps of every pass of the switch -- the digits kernel, and
 * the contraction (the product's kernel and its bias kernel) -- are bracketed by HIP events on the stream they run on.
 * Synchronises the recorded events, returns the sums since the last call and resets them. */
typedef struct tfhe_hip_trlwe_switch_times {
  double digits_ms;      /* sum of the digits kernel durations                  */
  double contraction_ms; /* sum of the matrix-core contraction durations        */
  uint64_t passes;       /* passes of each (one per 2,048 ciphertexts)          */
} tfhe_hip_trlwe_switch_times;
int tfhe_hip_get_trlwe_switch_times(tfhe_hip_ctx *ctx, tfhe_hip_trlwe_switch_times *out);

/* ---- packed CMUX: caller-held TRGSW selectors ------
 *
 * The one product whose second operand is encrypted data of the caller's own: the external product TRGSW (.) TRLWE and
 * the CMUX on it, out = d0 + sel (.) (d1 - d0) -- trgsw::cmux and external_product_with_fft of the reference
 * (trgsw.rs:77-116, 173-196) with a TRGSW the caller holds (TRGSWLv1::encrypt_torus, trgsw.rs:29-49), not a row of the
 * bootstrapping key.  A server selects between packed ciphertexts under an encrypted bit: an encrypted `if`, or a lookup
 * in a table of packed ciphertexts by an encrypted index (rs_tfhe_amd.packing.lookup).  No bootstrap, no cloud key.
 *
 * Definition (normative).  N = 1024; all arithmetic wraps mod 2^32; (*) is the negacyclic product mod X^N + 1.
 *   Shapes.  A gadget (beta, t) with 1 <= beta <= 7 (the digits fit a signed byte), 1 <= t <= 32 (2t <= 64 columns of
 *     the polynomial product) and beta t <= 32: the TRLWE key switch's box with 2t columns.  g_i = 2^(32 - beta (i+1)),
 *     0 <= i < t.
 *   TRGSW.  [2t][2][N] u32 carrying a message polynomial mu(X) with small integer coefficients: every row a TRLWE lv1
 *     encryption of zero (the a half, then the b half), then g_i mu(X) added to the a half of row i and to the b half of
 *     row t + i.  This is the reference's row order; its encrypt_torus(p) is mu = p, a constant.
 *   Digits of a word w.  off = sum_i 2^(beta-1) g_i; rnd = 2^(31 - beta t) when beta t < 32, else 0;
 *       u_i(w) = ((w + off + rnd) >> (32 - beta (i+1))) & (2^beta - 1),      d_i(w) = u_i(w) - 2^(beta-1)
 *     in [-2^(beta-1), 2^(beta-1)): the rounding decomposition of packing and of the TRLWE key switch.  With the flag
 *     TFHE_HIP_CMUX_REFERENCE_DIGITS rnd = 0: trgsw::decomposition (trgsw.rs:144-171) word for word, so that
 *     (beta, t) = (bgbit, l) reproduces the reference's cmux.  Truncation leaves a bias of about
 *     |s|_1 2^(-beta t - 1) mu per level at the end slots, which a CMUX tree, unlike a blind rotation, never rotates
 *     away: the default rounds.
 *   The call.  sel is ONE TRGSW; d0, d1 and out are [count][2][N].  With x = d1 - d0, or x = d1 when d0 == NULL, and
 *     D_i(p) = sum_j d_i(p[j]) X^j, for each half c:
 *       out[m][c] = (d0 ? d0[m][c] : 0) + sum_{i<t} D_i(x[m].a) (*) sel[i][c] + sum_{i<t} D_i(x[m].b) (*) sel[t+i][c].
 *     d0 == NULL is the plain external product.  One selector serves the whole batch: the shape of a lookup level,
 *     and what makes the batch the rows of one integer GEMM (the plaintext polynomial product's, with the digit
 *     polynomials for weights).  The result is defined in integers: every device gives these words exactly.
 * Consequences.  For mu in {0, 1} the phase of out is that of d0 + mu (d1 - d0) plus, per coefficient, noise of
 *   variance about  2t N (2^(2 beta) / 12) alpha^2  +  mu (1 + N/2) 2^(-2 beta t) / 12  (torus units squared; alpha the
 *   selector's noise).  DESIGN.md section 9 tabulates which (beta, t) keep a boolean and an m = 16 message inside 8
 *   standard deviations after ten levels.
 * Selector encryption (normative).  tfhe_hip_batch_encrypt_trgsw makes `count` TRGSWs [count][2t][2][N] from
 *   mu [count][N] int32 under key_lv1 and a 32-byte generator key K.  Row `row` of selector m has the 64-bit index
 *   r = first_index + m 2t + row:
 *     Mask seed  S = words 0..7 of block(K, counter 0, nonce (0, 30, 0x444553)), returned in mask_seed_out.
 *     a          N keystream words under S, natural order (word x = word x mod 16 of counter x / 16), nonce
 *                (r & 0xffffffff, r >> 32, 0x45474C "EGL").
 *     e          f64_to_torus(N(0, alpha)) per coefficient under K, nonce (r & 0xffffffff, r >> 32, 0x45474E "EGN"),
 *                in the BSK generators' word order, as for packed encryption.  alpha = 0 gives exactly zero noise.
 *     b          = a (*) s1 + e (the product exact), and AFTER the body is formed g_i mu(X) is added to a (row < t,
 *                i = row) or to b (i = row - t).
 *   Full form only.  A (K, index) pair must never encrypt twice.  Away from samples within rounding of a torus step
 *   every implementation gives the same words.
 * Semantics.  A CMUX needs no key: it runs on a context with no cloud key loaded.  count == 0 returns TFHE_HIP_OK and
 *   writes nothing.  TFHE_HIP_EINVAL, nothing written: sel, d1 or out NULL (count > 0), a shape outside the box, an
 *   unknown flag bit, count > 2^31 - 1 (encryption: count 2t > 2^31 - 1, key_lv1 NULL or not binary, mu or out NULL,
 *   alpha negative or NaN, row indices past 2^64).  out must not overlap sel, d0 or d1; this is not checked.  Bulk
 *   calls: the context's mutex and the one staging path of the host-pointer form, never the combining front end.
 *   _dev: device pointers, d0 / d1 / out 16-byte aligned (TFHE_HIP_EINVAL, nothing launched, for one that is not; sel
 *   needs 4 bytes like any operand), queued on `stream` (NULL: the context's stream); the digits
 *   pass through a scratch of the context, 2,048 ciphertexts (2,048 2t N bytes) a pass.  The encryption's _dev form
 *   takes mu and out on the device, runs on the context's stream and has finished when it returns (the staged secrets
 *   are wiped behind it); key_lv1 and rng_key (NULL: getrandom(2)) are host pointers in both forms, mask_seed_out may
 *   be NULL.  There are no pool forms. */
enum { TFHE_HIP_CMUX_REFERENCE_DIGITS = 1 }; /* flags; rnd = 0: the reference's truncating decomposition */
int tfhe_hip_batch_trlwe_cmux(tfhe_hip_ctx *ctx, const uint32_t *sel, int basebit, int t, int flags, const uint32_t *d0,
                              const uint32_t *d1, size_t count, uint32_t *out);
int tfhe_hip_batch_trlwe_cmux_dev(tfhe_hip_ctx *ctx, const uint32_t *sel, int basebit, int t, int flags, const uint32_t *d0,
                                  const uint32_t *d1, size_t count, uint32_t *out, void *stream);
/* A CLIENT-side call: it takes the secret key. */
int tfhe_hip_batch_encrypt_trgsw(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const int32_t *mu, size_t count, int basebit, int t,
                                 double alpha, const uint8_t rng_key[32], uint64_t first_index, uint8_t mask_seed_out[32],
                                 uint32_t *out);
int tfhe_hip_batch_encrypt_trgsw_dev(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const int32_t *mu, size_t count, int basebit,
                                     int t, double alpha, const uint8_t rng_key[32], uint64_t first_index,
                                     uint8_t mask_seed_out[32], uint32_t *out);
/* While profiling is enabled the three steps of every pass of the CMUX -- the digits kernel, the contraction (the
 * product's kernel) and the addend kernel (no pair without d0) -- are bracketed by HIP events on the stream they run on.
 * Synchronises the recorded events, returns the sums since the last call and resets them. */
typedef struct tfhe_hip_cmux_times {
  double digits_ms;      /* sum of the digits kernel durations                  */
  double contraction_ms; /* sum of the matrix-core contraction durations        */
  double addend_ms;      /* sum of the addend kernel durations                  */
  uint64_t passes;       /* passes of each (one per 2,048 ciphertexts)          */
} tfhe_hip_cmux_times;
int tfhe_hip_get_cmux_times(tfhe_hip_ctx *ctx, tfhe_hip_cmux_times *out);

/* ---- encrypted 2-D convolution: int8 filters over a feature map of LWE ciphertexts ------
 *
 * The convolutional layer beside the linear one: `out_c` plaintext int8 filters of k_h x k_w x in_c slide over an
 * in_h x in_w map whose every pixel holds in_c LWE ciphertexts, for each of `groups` independent maps.  It is the dense
 * form's product evaluated as an implicit GEMM (csrc/matmul.hpp, MmConv): the kernel reads each tap's ciphertexts
 * where they lie, so no im2col copy of the input is ever made; exact mod 2^32, no key, no atomics.
 *
 * Definition (normative).  Channels-last on both sides, so one layer's output is the next layer's input without a
 * transpose; n of the context's set; all sums in wrapping u32 arithmetic.
 *   out_h = (in_h + 2 pad_h - k_h) / stride_h + 1,  out_w likewise   (k_h <= in_h + 2 pad_h, k_w <= in_w + 2 pad_w)
 *   in   [groups][in_h][in_w][in_c][n+1]     u32
 *   w    [out_c][k_h][k_w][in_c]             int8  (the im2col order: K = k_h * k_w * in_c contiguous per filter)
 *   bias [out_c] u32 torus words, or NULL for zero
 *   out  [groups][out_h][out_w][out_c][n+1]  u32
 *     out[g][oy][ox][oc][x] = sum_{ky,kx,ic} (int32)w[oc][ky][kx][ic]
 *                                            * in[g][oy*stride_h + ky - pad_h][ox*stride_w + kx - pad_w][ic][x]
 *                             + (x == n ? bias[oc] : 0)
 *   where a term whose input coordinate falls outside the map is zero (the trivial encryption of 0: exact).
 *   1 <= K <= 65,536 (the dense form's accumulator bound).  A 1-D convolution is in_h = k_h = 1.
 * Consequences.  The phase of an output is sum w * phase(input) + bias[oc], exactly, mod 2^32; the noise variance scales
 *   by the sum of w^2 over the taps that fall inside the map (a border output has fewer terms than an interior one).
 *   What the dense form says about the message encoding and about weights wider than int8 holds here too.
 * Semantics.  Every field but pad_h and pad_w is at least 1; in_h + 2 pad_h and in_w + 2 pad_w are at most 2^31 - 1;
 *   groups * out_h * out_w * out_c <= 2^31 - 1 and groups * in_h * in_w * in_c <= 2^31 - 1 (ciphertexts written and
 *   read).  TFHE_HIP_EINVAL for a NULL shape, a field that is zero or out of range, a filter larger than the padded map,
 *   K out of range, a NULL w, in or out (with groups > 0) and a product too large -- checked in this order, shape first,
 *   then as the dense form checks rows = out_c, cols = K and one group per output position; groups == 0 with a valid
 *   shape returns TFHE_HIP_OK and writes nothing.  out must not overlap in.  Bulk calls (the context's mutex and the one
 *   staging path of the host-pointer form, never the combining front end); no key is needed.  _dev: every pointer but
 *   `shape`, w and bias included, is device memory; the call is queued on `stream` (NULL: the context's stream).  w
 *   needs no alignment; in_c a multiple of 16 takes the kernel's fast path (one tap per 16 K-rows). */
typedef struct tfhe_hip_conv2d_shape {
  uint32_t in_h, in_w, in_c;   /* input feature map */
  uint32_t out_c, k_h, k_w;    /* filters */
  uint32_t stride_h, stride_w; /* >= 1 */
  uint32_t pad_h, pad_w;       /* zero padding on both sides of each axis */
} tfhe_hip_conv2d_shape;
int tfhe_hip_batch_tlwe_conv2d(tfhe_hip_ctx *ctx, const tfhe_hip_conv2d_shape *shape, const int8_t *w,
                               const uint32_t *bias, const uint32_t *in, size_t groups, uint32_t *out);
int tfhe_hip_batch_tlwe_conv2d_dev(tfhe_hip_ctx *ctx, const tfhe_hip_conv2d_shape *shape, const int8_t *w,
                                   const uint32_t *bias, const uint32_t *in, size_t groups, uint32_t *out, void *stream);

/* ---- encrypted-table key switch and the tree bootstrap: any function of two encrypted digits ------
 *
 * A programmable bootstrap evaluates a table of ONE input, whose message modulus the parameter set caps (16 on
 * SECURITY_UINT4).  A function f(x, y) of two digits of modulus m is the tree-based bootstrap (Guimaraes, Borin,
 * Aranha, TCHES 2021): bootstrap y with the m tables f(i, .), turn the m results into ONE encrypted test vector, and
 * blind-rotate that by x -- m / k + 1 blind rotations with k-fold many-LUT tables, and no modulus above m anywhere.
 * The middle step is the encrypted-table key switch: the packing key switch of the m results, each spread over its box.
 *
 * Definition (normative).  In integers mod 2^32, negacyclic mod X^N + 1.  The key, the digits d_l and the gadget are
 * the packing key's (section above): no new key material and no new security assumption.  m is a power of two,
 * 2 <= m <= 512; W = N / m, off = W / 2 (div_round(x N, m) = x W and div_round(N, 2m) of the LUT generator).
 *   in   [m][count][n+1] u32, function-major: ciphertext c of function x at in[x][c] -- the layout
 *        tfhe_hip_batch_lincomb_bootstrap_many writes.
 *   out  [count][2][N] u32, the a row then the b row.
 *   For ciphertext c, with c_x = (a_x, b_x) = in[x][c]:
 *     P_x = ( - sum_{i,l} d_l(a_x[i]) a_{i,l} ,  b_x X^0 - sum_{i,l} d_l(a_x[i]) b_{i,l} )    (packing's result for one
 *                                                                                             input at slot 0)
 *     Q   = sum_x X^(x W) P_x
 *     out[c] = X^(-off) (1 + X + ... + X^(W-1)) Q   on both rows, i.e.
 *     out[c][h][y] = sum_{r < W} Q~[h][y + off - r],  Q~ the negacyclic extension (Q~[i] = -Q[i -/+ N] outside 0..N-1).
 *   Q is what tfhe_hip_batch_pack_tlwe returns for a group that holds c_x at slot x W and zero ciphertexts elsewhere.
 *   For trivial inputs (a = 0, b = v_x) the result is key-free: a row 0, b row the generator's table of the values v.
 *   The phase of out[c] under s1 is that table of the inputs' phases -- each input's rounding error replicated across
 *   its box, not summed -- plus key noise summed over W terms.  Every device and parameter set gives these words exactly.
 * Semantics.  The call needs the packing key and no cloud key: TFHE_HIP_ENOKEY without one.  TFHE_HIP_EINVAL for m not
 * a power of two in [2, 512], for m * count >= 2^31, or for a null pointer with count > 0; count == 0 returns
 * TFHE_HIP_OK.  Bulk calls (the context's mutex, never the combining front end).  _dev: device pointers, only enqueued
 * on `stream` (NULL: the context's stream). */
int tfhe_hip_batch_pack_table(tfhe_hip_ctx *ctx, const uint32_t *in, int m, size_t count, uint32_t *out);
int tfhe_hip_batch_pack_table_dev(tfhe_hip_ctx *ctx, const uint32_t *in, int m, size_t count, uint32_t *out,
                                  void *stream);
/* The tree bootstrap.  x, y, out [count][n+1]; testvecs [m / k][2][N] with k = n_luts in {1, 2, 4, 8}, k <= m: table j
 * packs f(j k + r, .), r < k, as the many-LUT generator does (k = 1: the plain LUT of f(j, .)).
 *   S[j k + r] = output r of tfhe_hip_batch_lincomb_bootstrap_many(1 * y, table j, n_luts = k, key switch on)
 *   T          = tfhe_hip_batch_pack_table(S, m)
 *   out        = tfhe_hip_batch_bootstrap(x, T, per_ct = 1, keyswitch)
 * word for word: x selects among the m stage-1 results, y is what stage 1 rotates by.  The batch is processed in chunks
 * so that the context-owned stage-1 scratch [m][chunk][n+1] stays at or under 256 MiB (TFHE_HIP_BIVARIATE_CHUNK in
 * the environment lowers the chunk, in ciphertexts: for tests); neither chunking nor the kernel selectors change a bit.
 * The scratch grows on demand and is freed with the context.  Needs the cloud key and the packing key
 * (TFHE_HIP_ENOKEY for either); TFHE_HIP_EINVAL for bad m or n_luts, null tables, or null x / y / out with count > 0.
 * Bulk calls, like the many-LUT bootstrap.  _dev only enqueues on `stream`. */
int tfhe_hip_batch_bootstrap_bivariate(tfhe_hip_ctx *ctx, const uint32_t *x, const uint32_t *y, const uint32_t *testvecs,
                                       int m, int n_luts, int keyswitch, uint32_t *out, size_t count);
int tfhe_hip_batch_bootstrap_bivariate_dev(tfhe_hip_ctx *ctx, const uint32_t *x, const uint32_t *y,
                                           const uint32_t *testvecs, int m, int n_luts, int keyswitch, uint32_t *out,
                                           size_t count, void *stream);

/* Pinned host buffers.  The host entry points below take ordinary (pageable) memory and stage it through the
 * device around the kernels: 3 x 184 MB for a 65,536-ciphertext gate batch, about 7 % of the call.  When EVERY
 * ciphertext operand of a call (inputs and output) is pinned host memory -- allocated here, or the caller's own
 * buffers registered with hipHostRegister -- the kernels read and write it in place over PCIe (each ciphertext is
 * read once in the blind rotation's prologue and written once by the key switch) and the call runs at the
 * device-resident rate.  Nothing else changes: same functions, same arguments, same results. */
int tfhe_hip_host_alloc(size_t bytes, void **out);
void tfhe_hip_host_free(void *p);

/* ---- the hot path, batched --------------------------------------------- */

/* Replaces: gates::batch_{nand,and,or,xor,nor,xnor}[_with_railgun]
 * (src/gates.rs:352-547) and, with count == 1, Gates::{nand,...,or_yn}
 * (src/gates.rs:54-150).  a, b, out: [count][n+1].  b is ignored for COPY. */
int tfhe_hip_batch_gate(tfhe_hip_ctx *ctx, int gate, const uint32_t *a, const uint32_t *b,
                        uint32_t *out, size_t count);
int tfhe_hip_batch_gate_dev(tfhe_hip_ctx *ctx, int gate, const uint32_t *a, const uint32_t *b,
                            uint32_t *out, size_t count, void *stream);

/* A batch whose ciphertexts carry different gates: gates[c] is the tfhe_hip_gate of
 * ciphertext pair c.  This is what a levelised circuit (e.g. the ripple-carry adder of
 * examples/add_two_numbers.rs) issues per level: every gate of the level in ONE launch,
 * whatever its type.  Same semantics as count calls of the Gates method
 * (src/gates.rs:54-150); b is read for every gate but COPY.  The host entry rejects codes
 * above TFHE_HIP_COPY with TFHE_HIP_EINVAL; the _dev entry cannot read device memory on the
 * host: the kernel treats such a ciphertext as COPY and raises a device-side flag that the next
 * tfhe_hip_synchronize() reports as TFHE_HIP_EINVAL. */
int tfhe_hip_batch_gates_mixed(tfhe_hip_ctx *ctx, const uint8_t *gates, const uint32_t *a,
                               const uint32_t *b, uint32_t *out, size_t count);
int tfhe_hip_batch_gates_mixed_dev(tfhe_hip_ctx *ctx, const uint8_t *gates, const uint32_t *a,
                                   const uint32_t *b, uint32_t *out, size_t count, void *stream);

/* The same per-ciphertext gates ending in bootstrap_without_key_switch (bootstrap/mod.rs:31-35): the output is
 * sample_extract_index_2 of the rotated accumulator, [count][n+1] (trlwe.rs:122-136; needs n <= N).  This is the
 * first level of Gates::mux (gates.rs:165-177: and(a, b) and and(not(a), c) without key switch) for a whole batch in
 * ONE launch -- gates = AND for the first operand pairs, ANDNY for the second; the second level (or(u1, u2),
 * gates.rs:179-182) is a tfhe_hip_batch_gates_mixed launch that can carry other gates of the same circuit level
 * beside it.  Same gate-code rules as above. */
int tfhe_hip_batch_gates_mixed_nks(tfhe_hip_ctx *ctx, const uint8_t *gates, const uint32_t *a, const uint32_t *b,
                                   uint32_t *out, size_t count);
int tfhe_hip_batch_gates_mixed_nks_dev(tfhe_hip_ctx *ctx, const uint8_t *gates, const uint32_t *a, const uint32_t *b,
                                       uint32_t *out, size_t count, void *stream);

/* Replaces: Bootstrap::bootstrap / bootstrap_without_key_switch
 * (src/bootstrap/vanilla.rs:40-63) and LutBootstrap::bootstrap_lut
 * (src/bootstrap/lut.rs:79-99), mapped over a batch.
 *   in        [count][n+1]
 *   testvec   NULL = the cloud key's test vector; else a LookupTable.poly
 *             ([2][N], shared by the batch) or [count][2][N] when per_ct != 0
 *   keyswitch 1: sample_extract_index(.,0) + identity_key_switching
 *             0: sample_extract_index_2(.,0)  (vanilla.rs:54-63)
 *   out       [count][n+1] */
int tfhe_hip_batch_bootstrap(tfhe_hip_ctx *ctx, const uint32_t *in, const uint32_t *testvec,
                             int per_ct, int keyswitch, uint32_t *out, size_t count);
int tfhe_hip_batch_bootstrap_dev(tfhe_hip_ctx *ctx, const uint32_t *in, const uint32_t *testvec,
                                 int per_ct, int keyswitch, uint32_t *out, size_t count,
                                 void *stream);

/* Replaces: the TLWE arithmetic between bootstraps -- Add, Sub, Neg, AddMul, SubMul for &TLWELv0
 * (src/tlwe.rs:129-214) -- mapped over a batch:  out = ca * a + cb * b  on all n+1 words (wrapping u32),
 * then out[n] += cconst.  Add = (1, 1, 0), Sub = (1, -1, 0), Neg = (-1, 0, 0) with b = NULL,
 * AddMul(k) = (1, k, 0), SubMul(k) = (1, -k, 0).  b may be NULL when cb == 0.  out may alias a or b. */
int tfhe_hip_batch_tlwe_lincomb(tfhe_hip_ctx *ctx, uint32_t ca, const uint32_t *a, uint32_t cb,
                                const uint32_t *b, uint32_t cconst, uint32_t *out, size_t count);
int tfhe_hip_batch_tlwe_lincomb_dev(tfhe_hip_ctx *ctx, uint32_t ca, const uint32_t *a, uint32_t cb,
                                    const uint32_t *b, uint32_t cconst, uint32_t *out, size_t count,
                                    void *stream);

/* Replaces: `bootstrap_lut(&(&x + &y), &lut, &cloud_key)` -- a TLWE linear combination fed straight
 * into a (programmable) bootstrap, the shape of every step of the reference's LUT arithmetic
 * (examples/lut_add_two_numbers.rs:124-158, examples/lut_arithmetic_demo.rs) and, with the default
 * test vector, of every gate (src/gates.rs:54-150).  The combination is computed in the prologue of
 * the blind-rotation kernel; arguments as in tfhe_hip_batch_tlwe_lincomb and tfhe_hip_batch_bootstrap. */
int tfhe_hip_batch_lincomb_bootstrap(tfhe_hip_ctx *ctx, uint32_t ca, const uint32_t *a, uint32_t cb,
                                     const uint32_t *b, uint32_t cconst, const uint32_t *testvec,
                                     int per_ct, int keyswitch, uint32_t *out, size_t count);
int tfhe_hip_batch_lincomb_bootstrap_dev(tfhe_hip_ctx *ctx, uint32_t ca, const uint32_t *a, uint32_t cb,
                                         const uint32_t *b, uint32_t cconst, const uint32_t *testvec,
                                         int per_ct, int keyswitch, uint32_t *out, size_t count,
                                         void *stream);

/* Many-LUT programmable bootstrap (Chillotti, Ligier, Orfila, Tap 2021, "PBS-manyLUT"; tfhe-rs
 * apply_many_lookup_table): n_luts = k in {1, 2, 4, 8} functions of the same input from ONE blind
 * rotation.  The input is prepared as in tfhe_hip_batch_lincomb_bootstrap; with d = log2 k the rotation
 * amounts are rounded to multiples of k:  a~_i = ((p_i + 2^(20+d)) mod 2^32) >> (21+d) << d  and
 * b~ = 2N - ((((u64)p_n + 2^(20+d)) >> (21+d)) << d)  (d = 0: the ordinary bootstrap, trgsw.rs:202-211).
 * Output j < k is sample_extract_index(acc, j) then the key switch (keyswitch != 0), or
 * sample_extract_index_2(acc, j) (keyswitch == 0; needs n <= N), trlwe.rs:106-136.  out is FUNCTION-MAJOR,
 * [k][count][n+1]: out + j*count*(n+1) holds what a single-LUT call for function j would write.
 * testvec ([2][N], or [count][2][N] with per_ct) is required and must pack the k functions
 * (lut.Generator.generate_many_lookup_table / rs_tfhe::lut::Generator::generate_many_lookup_table:
 * position r of message x's box holds f_(r mod k)(x)).  Rounding to multiples of k scales the
 * mod-switch error by k: a k-LUT of message modulus m fails like a single LUT of modulus m*k, so keep
 * m*k <= 16 on SECURITY_UINT4.  TFHE_HIP_EINVAL: n_luts not in {1, 2, 4, 8}, testvec NULL, cb != 0
 * with b NULL, k*count > 2^31 - 1.  These calls do not join the combining front end
 * (tfhe_hip_set_combining): each is launched as it is made. */
int tfhe_hip_batch_lincomb_bootstrap_many(tfhe_hip_ctx *ctx, uint32_t ca, const uint32_t *a, uint32_t cb,
                                          const uint32_t *b, uint32_t cconst, const uint32_t *testvec, int per_ct,
                                          int n_luts, int keyswitch, uint32_t *out, size_t count);
int tfhe_hip_batch_lincomb_bootstrap_many_dev(tfhe_hip_ctx *ctx, uint32_t ca, const uint32_t *a, uint32_t cb,
                                              const uint32_t *b, uint32_t cconst, const uint32_t *testvec, int per_ct,
                                              int n_luts, int keyswitch, uint32_t *out, size_t count, void *stream);

/* Replaces: trgsw::batch_blind_rotate[_with_railgun] (src/trgsw.rs:289-305),
 * trgsw::blind_rotate (:198-226) and blind_rotate_with_testvec (:242-274).
 * in [count][n+1]; testvec NULL or [2][N]; out_trlwe [count][2][N]. */
int tfhe_hip_batch_blind_rotate(tfhe_hip_ctx *ctx, const uint32_t *in, const uint32_t *testvec,
                                uint32_t *out_trlwe, size_t count);
int tfhe_hip_batch_blind_rotate_dev(tfhe_hip_ctx *ctx, const uint32_t *in,
                                    const uint32_t *testvec, uint32_t *out_trlwe, size_t count,
                                    void *stream);

/* Replaces: Gates::mux (src/gates.rs:157-183, naive == 0; the reference
 * formula reproduced bit-for-bit) and Gates::mux_naive
 * (src/gates.rs:189-199, naive != 0), mapped over a batch.  [count][n+1] each. */
int tfhe_hip_batch_mux(tfhe_hip_ctx *ctx, int naive, const uint32_t *a, const uint32_t *b,
                       const uint32_t *c, uint32_t *out, size_t count);
int tfhe_hip_batch_mux_dev(tfhe_hip_ctx *ctx, int naive, const uint32_t *a, const uint32_t *b,
                           const uint32_t *c, uint32_t *out, size_t count, void *stream);

/* ---- single stages (parity tests; same kernels' device code) ------------ */

/* Replaces: trgsw::external_product_with_fft (src/trgsw.rs:77-116) with
 * trgsw_fft = cloud_key.bootstrapping_key[bsk_index[c]].
 * trlwe_in/out [count][2][N]; bsk_index [count]. */
int tfhe_hip_batch_external_product(tfhe_hip_ctx *ctx, const uint32_t *trlwe_in,
                                    const int32_t *bsk_index, uint32_t *trlwe_out, size_t count);

/* Replaces: trlwe::sample_extract_index(., k) (src/trlwe.rs:106-120), 0 <= k < N (the bootstrap uses
 * k = 0): out[i] = a[k-i] for i <= k, MAX - a[N+k-i] for i > k, out[N] = b[k].
 * trlwe [count][2][N] -> out [count][N+1]. */
int tfhe_hip_batch_sample_extract(tfhe_hip_ctx *ctx, const uint32_t *trlwe, int k, uint32_t *out,
                                  size_t count);

/* Replaces: trgsw::identity_key_switching (src/trgsw.rs:332-360).
 * tlwe_lv1 [count][N+1] -> out [count][n+1]. */
int tfhe_hip_batch_identity_key_switch(tfhe_hip_ctx *ctx, const uint32_t *tlwe_lv1,
                                       uint32_t *out, size_t count);

/* ---- proxy re-encryption (the reference's feature `proxy-reenc`, src/proxy_reenc.rs; SURVEY 8(f) rank 4: "same
 * digit-lookup kernel shape as keyswitch") -------------------------------------------------------------------------
 * Replaces: proxy_reenc::reencrypt_tlwe_lv0 (src/proxy_reenc.rs:468-510) over a batch:
 *   out.b = in.b;  for i < n, j < t:  k = ((in.a[i] + 2^(32-(1+basebit*t))) >> (32-(j+1)*basebit)) & (base-1);
 *                                     k != 0: out -= key[base*t*i + base*j + k]          (all n+1 words, wrapping)
 * i.e. trgsw::identity_key_switching with a source of n coefficients, and it runs on the same kernels (the source is
 * padded to N coefficients whose digits are all zero).  A context -- or a key view of one (tfhe_hip_key_create), so that
 * cloud keys and re-encryption keys stay resident side by side -- holds EITHER a cloud key OR a re-encryption key:
 * loading one drops the other; the bootstrap entry points return TFHE_HIP_ENOKEY on a handle that holds a
 * re-encryption key, and these return it on a handle that does not.
 *   key [n][t][base][n+1] u32 = ProxyReencryptionKey::key_encryptions (src/proxy_reenc.rs:224-233; the k = 0 entries
 *   are never read, as in the reference :311-313), with base = 2^basebit and t of the context's parameter set (the
 *   reference's new_symmetric / new_asymmetric use params::trgsw_lv1::{BASEBIT, IKS_T}, :271-279, :362-370; for
 *   *_with_params keys create the context with that basebit / t).  The key is generated by the client (it needs the
 *   delegator's secret key): rs-tfhe_amd/proxy_reenc.py mirrors PublicKeyLv0 and ProxyReencryptionKey.
 *   Needs n <= N = 1024 (every set but SECURITY_UINT5 .. 8): TFHE_HIP_EINVAL otherwise.
 *   in [count][n+1] -> out [count][n+1]; the _dev form takes device pointers and a hipStream_t (NULL = the context's)
 *   and only enqueues. */
int tfhe_hip_load_reenc_key(tfhe_hip_ctx *ctx, const uint32_t *key);
int tfhe_hip_reenc_key_is_loaded(tfhe_hip_ctx *ctx);
int tfhe_hip_batch_reencrypt(tfhe_hip_ctx *ctx, const uint32_t *in, uint32_t *out, size_t count);
int tfhe_hip_batch_reencrypt_dev(tfhe_hip_ctx *ctx, const uint32_t *in, uint32_t *out, size_t count, void *stream);

/* ---- public-key encryption and the asymmetric re-encryption key ------------------------------------------------
 *
 * What happens BEFORE the proxy: a data owner who holds only a public key encrypts (PublicKeyLv0::encrypt_f64,
 * src/proxy_reenc.rs:168-200), and a delegator makes the re-encryption key towards a delegatee's public key
 * (ProxyReencryptionKey::new_asymmetric, :271-326, the mode the reference recommends).  Both are one exact integer
 * contraction out[r] = sum_e c[r][e] * E[e], c in {-1, 0, +1}, over the public key E [size][n+1] (encryptions of zero
 * under the secret key, :95-99), and run on the matrix cores the way the packing key switch does: E is split once, at
 * load, into four balanced signed byte planes; |acc| <= 128 * size <= 2^20, so the sum is equal word for word.
 *
 * Format (normative).  Keystream words are block(K, counter, nonce (n0, n1, n2)) of the seeded section, under a SECRET
 * 32-byte generator key K.  A row index g is 64 bits; its nonce is (g & 0xffffffff, g >> 32, domain):
 *
 *   what                                    domain               counter   use
 *   public-key encryption selectors         0x504B45 ("PKE")     w / 16    selector word w of row g is word w % 16
 *   public-key encryption noise             0x504B4E ("PKN")     0         g0 of gauss2(words 0..3, alpha); rest unused
 *   re-encryption key selectors / noise     0x524B45 ("RKE") /   as above  row g = base*t*i + base*j + k, k >= 1
 *                                           0x524B4E ("RKN")
 *
 *   Entry e < size of row g reads bits 2*(e % 16) (take) and 2*(e % 16) + 1 (sign, 1 = subtract) of selector word e / 16:
 *   c_e = take ? (sign ? -1 : +1) : 0 -- the reference's two gen_bool(0.5) draws.
 *   out[g] = sum_e c_e * E[e] on all n + 1 words, wrapping u32; the body then gets + plain + f64_to_torus(g0), gauss2
 *   and f64_to_torus those of the seeded section.  With alpha == 0 the noise is exactly zero.
 *   Re-encryption key: plain = f64_to_torus(((k * key_from[i]) as u32 as f64) / 2^((j+1)*basebit)); the k = 0 rows are
 *   zero and their streams are unused.
 *   The domains differ from every other one of this header (KSK, BSK, EWL, DES, PKS), so one K may serve all generators.
 * Security.  (1) A (K, g) pair must never encrypt two messages: the difference of the two ciphertexts would be the
 * difference of the plaintexts in the clear.  With a caller-held K, first_index must move past every row already used.
 * (2) Whoever knows K can strip the mask: the selectors are a function of (K, g) and E is public.  Hence rng_key == NULL
 * means "draw K from getrandom(2) for this call", and a caller-held K is as secret as the plaintexts.  The library
 * zeroes the selectors on the device behind each pass; K travels to the kernels as a launch argument.  The host form's
 * staged plaintexts are zeroed before it returns (rule (5) of the symmetric section).
 * Away from noise samples that sit within rounding of a torus step every implementation of this section gives the same
 * words.
 * Out of scope: pool forms.  (The public key itself and the symmetric re-encryption key are made on the device by the
 * next section.) */
/* encryptions [size][n+1], 1 <= size <= 8192 (TFHE_HIP_EINVAL otherwise, and the previous public key stays).  Builds
 * the byte planes on the device, on a context or a key view; needs no cloud key; a cloud-key or re-encryption-key
 * change leaves it in place; freeing the view frees it. */
int tfhe_hip_load_public_key(tfhe_hip_ctx *ctx_or_view, const uint32_t *encryptions, size_t size);
/* 0 / 1, never an error code (no device call is made). */
int tfhe_hip_public_key_is_loaded(tfhe_hip_ctx *ctx_or_view);
/* plain [count] torus words (f64_to_torus of the messages) -> out [count][n+1]; row m uses g = first_index + m.
 * alpha: the fresh noise's standard deviation.  TFHE_HIP_ENOKEY without a public key.  The host form stages through the
 * context's buffers; _dev takes device pointers and a hipStream_t (NULL = the context's) and only enqueues. */
int tfhe_hip_batch_pk_encrypt(tfhe_hip_ctx *ctx, const uint32_t *plain, size_t count, double alpha,
                              const uint8_t rng_key[32], uint64_t first_index, uint32_t *out);
int tfhe_hip_batch_pk_encrypt_dev(tfhe_hip_ctx *ctx, const uint32_t *plain, size_t count, double alpha,
                                  const uint8_t rng_key[32], uint64_t first_index, uint32_t *out, void *stream);
/* The asymmetric re-encryption key from key_from [n] (the delegator's secret key: a CLIENT-side call) towards the public
 * key loaded on this handle, with basebit and t of the context's parameter set.  The handle is left holding it -- bit
 * for bit what tfhe_hip_load_reenc_key(key_out) builds; key_out [n][t][base][n+1] may be NULL (no download).
 * TFHE_HIP_ENOKEY without a public key; TFHE_HIP_EINVAL for n > 1024, a NULL key_from, alpha negative or NaN.  A refused
 * call leaves the handle's keys as they were. */
int tfhe_hip_gen_reenc_key_asymmetric(tfhe_hip_ctx *ctx_or_view, const uint32_t *key_from, double alpha,
                                      const uint8_t rng_key[32], uint32_t *key_out);
/* While profiling is enabled (tfhe_hip_set_profiling) the two kernels of every pass of the calls above -- the keystream
 * pass that writes the selectors, and the contraction -- are bracketed by HIP events on the stream they run on.
 * Synchronises the recorded events, returns the sums since the last call and resets them. */
typedef struct tfhe_hip_pk_encrypt_times {
  double selectors_ms;   /* sum of the keystream (selector) kernel durations */
  double contraction_ms; /* sum of the matrix-core kernel durations          */
  uint64_t passes;       /* launches of each (one per 65,536 rows)           */
} tfhe_hip_pk_encrypt_times;
int tfhe_hip_get_pk_encrypt_times(tfhe_hip_ctx *ctx, tfhe_hip_pk_encrypt_times *out);

/* ---- symmetric encryption: ciphertexts, the public key and the symmetric re-encryption key ------------------------
 *
 * Everything made with the SECRET key: ordinary TLWE lv0 encryptions in bulk (TLWELv0::encrypt_f64, src/tlwe.rs:37-53),
 * the public key's encryptions of zero (PublicKeyLv0::new, src/proxy_reenc.rs:125-153) and the symmetric re-encryption
 * key (ProxyReencryptionKey::new_symmetric, :362-425).  All three are the same row, made by one wave of one kernel
 * (csrc/sym_encrypt.hpp); with these and the packed TRLWE ciphertexts of the "packed encryption" section below every
 * key and ciphertext type of the reference has a device constructor.
 *
 * Format (normative).  Keystream words, gauss2 and f64_to_torus are those of the seeded section.  A row index g is
 * 64 bits; its nonce is (g & 0xffffffff, g >> 32, domain).  Mask word x < n of row g is word x % 16 of the block with
 * counter x / 16 of the mask stream; the noise is g0 of gauss2(words 0..3 of block 0 of the noise stream, alpha), the
 * rest of that block unused.
 *
 *   use                              row index g                  mask: key, domain              noise: under K, domain
 *   bulk TLWE lv0                    first_index + m              public seed S, 0x45574C "EWL"  0x45574E "EWN"
 *                                                                 (the seeded-TLWE masks)
 *   public key row                   e < size                     K, 0x504B4D "PKM"              0x504B5A "PKZ"
 *   symmetric re-encryption key row  base*t*i + base*j + k, k>=1  K, 0x524B4D "RKM"              0x524B53 "RKS"
 *
 *   row = (a, <a, s0> + plain + f64_to_torus(g0)), wrapping u32.  With alpha == 0 the noise is exactly zero.
 *   plain: bulk TLWE: the caller's torus word; public key: 0; re-encryption key:
 *   f64_to_torus(((k * key_from[i]) as u32 as f64) / 2^((j+1)*basebit)) -- the k = 0 rows are zero and their streams are
 *   unused, as in the asymmetric key.
 *   A bulk result (S, first_index, bodies) is by construction a seeded TLWE batch: tfhe_hip_expand_seeded_tlwe expands
 *   it to the words the full form writes.
 *   The five new domains differ from every other one of this header, so one K may serve all generators.
 * Security.  (1) A (K, g) pair is used once, whatever S is: two rows with equal noise and different masks give a
 * noise-free LWE sample of the secret key.  With a caller-held K, first_index must move past every row already used, and
 * one K makes one public key and one re-encryption key.  (2) An (S, g) pair is used once (the seeded section's rule).
 * (3) rng_key == NULL draws K from getrandom(2) per call; a caller-held K is as secret as the secret key: whoever can
 * regenerate the noise reads the key off the rows.  (4) The staged secret keys and K's device copy are zeroed before a
 * host-form call returns, as tfhe_hip_gen_cloud_key* does; the _dev form, which only enqueues, queues the zeroing on
 * `stream` behind its kernel, also where the call fails.  The library's host copies are wiped.  (5) Every host form
 * of this header that stages plaintexts or returns decrypted words -- this section's, public-key and packed
 * encryption, decryption -- zeroes them in its staging buffer before it returns: the device buffer and, on pool
 * members, its pinned host arena.
 * Away from noise samples that sit within rounding of a torus step every implementation of this section gives the same
 * words.
 * Out of scope: pool forms. */
/* key_lv0 [n] (host memory in both forms), plain [count] torus words -> bodies [count] and / or out [count][n+1]; either
 * may be NULL, and with out == NULL no mask is written (the seeded form).  Needs no key on the handle; every parameter
 * set (n <= 1279).  TFHE_HIP_EINVAL for a NULL key_lv0, mask_seed or plain, for bodies and out both NULL with count > 0,
 * alpha negative or NaN, first_index + count beyond 2^64.  count == 0 returns TFHE_HIP_OK.  _dev: plain / bodies / out
 * are device pointers, queued on `stream` (NULL: the context's stream). */
int tfhe_hip_batch_encrypt(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *plain, size_t count, double alpha,
                           const uint8_t rng_key[32], const uint8_t mask_seed[32], uint64_t first_index,
                           uint32_t *bodies, uint32_t *out);
int tfhe_hip_batch_encrypt_dev(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *plain, size_t count, double alpha,
                               const uint8_t rng_key[32], const uint8_t mask_seed[32], uint64_t first_index,
                               uint32_t *bodies, uint32_t *out, void *stream);
/* `size` encryptions of zero under key_lv0 [n], 1 <= size <= 8192 (TFHE_HIP_EINVAL otherwise, and the previous public
 * key stays).  The handle is left holding the public key -- bit for bit what tfhe_hip_load_public_key(encryptions_out)
 * builds; encryptions_out [size][n+1] may be NULL (no download). */
int tfhe_hip_gen_public_key(tfhe_hip_ctx *ctx_or_view, const uint32_t *key_lv0, size_t size, double alpha,
                            const uint8_t rng_key[32], uint32_t *encryptions_out);
/* The symmetric re-encryption key from key_from [n] to key_to [n] (both secret: a call for whoever holds both), with
 * basebit and t of the context's parameter set.  The handle is left holding it -- bit for bit what
 * tfhe_hip_load_reenc_key(key_out) builds; key_out [n][t][base][n+1] may be NULL (no download).  TFHE_HIP_EINVAL for
 * n > 1024, a NULL key, alpha negative or NaN.  A refused call leaves the handle's keys as they were. */
int tfhe_hip_gen_reenc_key_symmetric(tfhe_hip_ctx *ctx_or_view, const uint32_t *key_from, const uint32_t *key_to,
                                     double alpha, const uint8_t rng_key[32], uint32_t *key_out);

/* ---- decryption: phases, booleans and messages of LWE rows and of packed TRLWE slots --------------------------------
 *
 * The last step a client takes with the SECRET key (TLWELv0::decrypt_bool, src/tlwe.rs:60-68; decrypt_lwe_message,
 * :111-126), on results that already sit in device memory (csrc/decrypt.hpp).  rs-tfhe_amd/client.py (SecretKey.phase,
 * decrypt_bool, decrypt_lwe_message, packed_phase) is the definition: every word of every mode equals it.
 *
 * Format (normative).
 *   LWE form     in [count][key_len+1], key [key_len] binary; key_len is the context's n (lv0 ciphertexts under key_lv0)
 *                or N = 1024 (lv1 rows under key_lv1: what tfhe_hip_batch_sample_extract and the keyswitch == 0 form of
 *                tfhe_hip_batch_trlwe_matmul return).  out [count] u32 in every mode.
 *   packed form  trlwe [groups][2][N] under key_lv1; out[i], i < count <= groups * N, is slot i % N of group i / N.
 *                Groups past the one that holds result count - 1 are not read.
 *   PHASE        b - <a, s>, wrapping u32; packed: coefficient j of B - A (*) s1 mod X^N + 1.  Exact integers, no FFT.
 *   BOOL         1 where the phase read as i32 is >= 0, else 0.
 *   MESSAGE      (f64(phase) / 2^32 / (1 / (2 m)) + 0.5) truncated to an integer, then % m, in f64, in those operations
 *                and that order; m = modulus, 2 <= m <= 65,536.  In the other modes modulus is ignored.
 * TFHE_HIP_EINVAL for a key_len other than n or N, a NULL pointer, a key word other than 0 or 1, a mode other than the
 * three, a modulus outside [2, 65,536] in MESSAGE mode, count > 0x7FFFFFFF, count > groups * N.  count == 0 returns
 * TFHE_HIP_OK and touches nothing.  Needs no key on the handle; every parameter set.
 * Security.  The key is host memory in both forms.  What the device holds of it is zeroed behind the kernel on the
 * call's stream, and the library's host copy is wiped; a host-form call also zeroes the staging buffer that held the
 * phases or messages before it returns (rule (5) of the symmetric section).  _dev: in / trlwe / out are device
 * pointers, queued on `stream` (NULL: the context's stream); the decrypted words are then the caller's to guard.
 * Out of scope: pool forms, slot lists for the packed form. */
enum { TFHE_HIP_DECRYPT_PHASE = 0, TFHE_HIP_DECRYPT_BOOL = 1, TFHE_HIP_DECRYPT_MESSAGE = 2 };
int tfhe_hip_batch_decrypt(tfhe_hip_ctx *ctx, const uint32_t *key, size_t key_len, const uint32_t *in, size_t count,
                           int mode, uint32_t modulus, uint32_t *out);
int tfhe_hip_batch_decrypt_dev(tfhe_hip_ctx *ctx, const uint32_t *key, size_t key_len, const uint32_t *in, size_t count,
                               int mode, uint32_t modulus, uint32_t *out, void *stream);
int tfhe_hip_batch_decrypt_trlwe(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const uint32_t *trlwe, size_t groups,
                                 size_t count, int mode, uint32_t modulus, uint32_t *out);
int tfhe_hip_batch_decrypt_trlwe_dev(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const uint32_t *trlwe, size_t groups,
                                     size_t count, int mode, uint32_t modulus, uint32_t *out, void *stream);

/* ---- packed encryption: TRLWE lv1 ciphertexts, N values to a ciphertext -- full, seeded and expansion -------------
 *
 * TRLWELv1::encrypt_f64 / encrypt_bool (src/trlwe.rs:30-66) made with the SECRET ring key on the device
 * (csrc/trlwe_encrypt.hpp): the input form of tfhe_hip_batch_trlwe_matmul and tfhe_hip_batch_unpack_trlwe and what
 * tfhe_hip_batch_decrypt_trlwe reads back.  With these and the symmetric section every key and ciphertext type of the
 * reference has a device constructor.
 *
 * Format (normative).  Keystream words, gauss2, f64_to_torus and the nonce conventions are those of the seeded and
 * symmetric sections.  A batch of `count` plaintext torus words fills groups = ceil(count / N) TRLWEs, N = 1024: slot j
 * of group m holds plain[m N + j]; the slots at or past `count` of the last group encrypt 0 and plain is never read
 * there.  Group m has the 64-bit index g = first_group + m and the nonce (g & 0xffffffff, g >> 32, domain), with no
 * stream number.
 *
 *   what               key                domain           layout
 *   mask polynomial a  public seed S      0x45524C "ERL"   natural order: coefficient c is word c % 16 of the block with
 *                                                          counter c / 16 (64 blocks)
 *   noise e            generator key K    0x45524E "ERN"   the order of the BSK generators: block counter 2 lane + h,
 *                                                          lane < 64, h < 2; pair q < 4 is gauss2(w[4q..4q+3], alpha):
 *                                                          g0 -> e[lane + 64 (4h + q)], g1 -> the same index + 512
 *
 *   body: b[c] = (a (*) s1)[c] + f64_to_torus(e[c]) + plain[c], wrapping u32, the product mod X^N + 1, exact.  With
 *   alpha == 0 the noise is exactly zero.  The two domains differ from every other one of this header, so one K may
 *   serve this generator and every other one.
 *   A seeded packed batch is (S, first_group, bodies [groups][N], count): 4 KiB a ciphertext instead of 8, and by
 *   construction what the bodies-only output of the encrypting call returns; tfhe_hip_expand_seeded_trlwe expands it
 *   to the words the full form writes.
 * Security: the rules of the symmetric section.  A (K, g) pair is used once, whatever S is; an (S, g) pair is used
 * once; rng_key == NULL draws K from getrandom(2) per call; a caller-held K is as secret as the secret key.  K, s1
 * and the spectrum of s1 (which is secret too) are staged and zeroed as rule (4) there says, the host form's plaintexts
 * as rule (5).
 * Away from noise samples that sit within rounding of a torus step every implementation of this section gives the same
 * words.
 * Out of scope: pool forms. */
/* key_lv1 [N] (host memory in both forms), plain [count] torus words -> bodies [groups][N] and / or out [groups][2][N]
 * (a half, b half); either may be NULL, and with out == NULL no mask is stored.  Needs no key on the handle; every
 * parameter set.  TFHE_HIP_EINVAL for a NULL key_lv1, plain or mask_seed, for bodies and out both NULL with count > 0,
 * alpha negative or NaN, a key word other than 0 or 1, count > 0x7FFFFFFF, first_group + groups - 1 past 2^64, and (_dev)
 * a bodies or out pointer that is not 16-byte aligned.  count == 0 returns TFHE_HIP_OK and touches nothing.  _dev:
 * plain / bodies / out are device pointers, queued on `stream` (NULL: the context's stream). */
int tfhe_hip_batch_encrypt_trlwe(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const uint32_t *plain, size_t count,
                                 double alpha, const uint8_t rng_key[32], const uint8_t mask_seed[32], uint64_t first_group,
                                 uint32_t *bodies, uint32_t *out);
int tfhe_hip_batch_encrypt_trlwe_dev(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const uint32_t *plain, size_t count,
                                     double alpha, const uint8_t rng_key[32], const uint8_t mask_seed[32],
                                     uint64_t first_group, uint32_t *bodies, uint32_t *out, void *stream);
/* bodies [groups][N] -> out [groups][2][N]: out[m][0] the mask of group first_group + m under mask_seed, out[m][1] the
 * bodies.  No secret.  TFHE_HIP_EINVAL for a NULL mask_seed, bodies or out, first_group + groups - 1 past 2^64, groups
 * > 0x7FFFFFFF and (_dev) a pointer that is not 16-byte aligned.  groups == 0 returns TFHE_HIP_OK and touches
 * nothing. */
int tfhe_hip_expand_seeded_trlwe(tfhe_hip_ctx *ctx, const uint8_t mask_seed[32], uint64_t first_group,
                                 const uint32_t *bodies, size_t groups, uint32_t *out);
int tfhe_hip_expand_seeded_trlwe_dev(tfhe_hip_ctx *ctx, const uint8_t mask_seed[32], uint64_t first_group,
                                     const uint32_t *bodies, size_t groups, uint32_t *out, void *stream);

/* Replaces: FFTProcessor::{ifft, fft, poly_mul, batch_ifft, batch_fft}
 * (src/fft/mod.rs:80-107; KlemsaProcessor src/fft/klemsa.rs:88-174) and the
 * SPQLIOS C ABI Spqlios_ifft_lv1 / _fft_lv1 / _poly_mul_1024
 * (spqlios-wrapper.cpp:19-40).  Spectra use the Klemsa layout and scaling.
 *   ifft:     src [count][N] u32 -> res [count][N] f64
 *   fft:      src [count][N] f64 -> res [count][N] u32
 *   poly_mul: a, b [count][N] u32 -> res [count][N] u32  (negacyclic) */
int tfhe_hip_batch_ifft(tfhe_hip_ctx *ctx, double *res, const uint32_t *src, size_t count);
int tfhe_hip_batch_fft(tfhe_hip_ctx *ctx, uint32_t *res, const double *src, size_t count);
int tfhe_hip_batch_poly_mul(tfhe_hip_ctx *ctx, uint32_t *res, const uint32_t *a,
                            const uint32_t *b, size_t count);

/* ---- concurrent callers --------------------------------------------------- */

/* Replaces: the concurrency a `Send + Sync` strategy gets from Rayon's workers (src/bootstrap/mod.rs:23-38,
 * src/parallel/rayon_impl.rs:40-47).  Host-pointer calls of at most `max_count` ciphertexts are merged with the calls
 * other threads make meanwhile (see "Thread safety" above); larger calls run alone, as before.  The default bound is
 * twice the device's CU count (512: what one launch of the latency kernels takes; a lone caller pays nothing up to
 * there, concurrent callers of 512-gate calls gain 23 %); 0 switches merging off, the largest bound is 4096.  The
 * environment variable TFHE_HIP_COMBINE (a number, 0 = off), read when a context is created, sets the same bound.
 * Accepts a context or a key view (the setting is the context's).
 * Bulk work yields to small calls: a merged launch needs whole CUs and cannot start while a launch of tens of thousands
 * of ciphertexts holds them all, so while small calls have been arriving (within the last 250 ms) the batch kernel of a
 * large call on the same context goes out in launches of 8,192 ciphertexts -- a small call then waits for a chunk
 * boundary (about 40 ms) instead of the whole batch (300 ms), at 1.7 % of the batch's throughput.  Same results; with no
 * small calls in flight a batch is one launch, as before. */
int tfhe_hip_set_combining(tfhe_hip_ctx *ctx, size_t max_count);

typedef struct tfhe_hip_combine_stats {
  uint64_t max_count;               /* the bound in force                                         */
  uint64_t launches;                /* merged launches issued                                     */
  uint64_t requests;                /* calls they carried                                         */
  uint64_t ciphertexts;             /* ciphertexts they carried                                   */
  uint64_t max_requests_per_launch; /* most calls taken by one leader at once                     */
  uint64_t lingers;                 /* leaders that waited for the previous launch's callers      */
  double linger_us;                 /* ... and for how long in all                                */
  double pack_us;                   /* leaders' time, summed: packing operands into the arena     */
  double gpu_us;                    /* ... copies in, kernels, copy out, the synchronise          */
  double unpack_us;                 /* ... handing every caller its rows                          */
} tfhe_hip_combine_stats;
/* Counters since the last call; resets them. */
int tfhe_hip_get_combine_stats(tfhe_hip_ctx *ctx, tfhe_hip_combine_stats *out);

/* ---- measurement -------------------------------------------------------- */

/* When enabled, every blind-rotate / key-switch launch is bracketed by HIP
 * events on the stream it is launched on. */
int tfhe_hip_set_profiling(tfhe_hip_ctx *ctx, int enabled);

typedef struct tfhe_hip_kernel_times {
  double blind_rotate_ms; /* sum of blind-rotate kernel durations       */
  double key_switch_ms;   /* sum of key-switch kernel durations         */
  uint64_t blind_rotate_launches;
  uint64_t key_switch_launches;
  uint64_t bootstraps;    /* ciphertexts that went through blind rotate */
} tfhe_hip_kernel_times;

/* Synchronises the recorded events, returns the sums since the last reset and
 * resets them. */
int tfhe_hip_get_kernel_times(tfhe_hip_ctx *ctx, tfhe_hip_kernel_times *out);

/* Shader clock actually sustained by the blind-rotation kernel: while profiling is enabled every
 * workgroup adds its s_memtime (shader cycles) and s_memrealtime (constant-rate counter) deltas to a
 * device counter; shader_mhz = cycles / ticks * rtc_mhz over all workgroups since the last call.
 * Synchronises, returns the sample and resets it.  (Needed to price the kernel against the FP64
 * issue roofline at the clock the chip really ran, not at the 2.4 GHz datasheet maximum.) */
typedef struct tfhe_hip_clock_sample {
  double shader_mhz;       /* 0 when nothing was sampled */
  double rtc_mhz;          /* rate of the constant counter (hipDeviceAttributeWallClockRate) */
  uint64_t shader_cycles;  /* summed over workgroups */
  uint64_t rtc_ticks;
} tfhe_hip_clock_sample;
int tfhe_hip_get_clock_sample(tfhe_hip_ctx *ctx, tfhe_hip_clock_sample *out);
/* The same sample for the matrix-core key switch (k_key_switch_mfma; the other key-switch kernels do not
 * sample): the clock that prices it against the int8 MFMA roofline. */
int tfhe_hip_get_key_switch_clock_sample(tfhe_hip_ctx *ctx, tfhe_hip_clock_sample *out);

/* Which kernels a batch of `count` ciphertexts runs on under this handle's dispatch rules (the cloud key must be
 * loaded: the base-4 matrix-core key switch exists only once its byte planes do), as one line of text:
 *   "blind_rotate=batch[0,1024)+single[1024,1100) key_switch=mfma(k=4)"
 * blind_rotate: up to two launches over contiguous parts of the batch, each `batch` (k_blind_rotate, one wave per
 * ciphertext), `single` (k_blind_rotate_wide2, one eight-wave workgroup per ciphertext) or `pair`
 * (k_blind_rotate_pair); key_switch: `mfma` / `sliced` / `b4` / `generic` / `split` with the number of partial
 * walks merged by integer atomics (k) and, for `sliced`, the accumulator sets per lane.  Every choice returns the
 * same result bits (tests/test_gpu_parity.py::test_dispatch_crossovers_bit_exact); the line exists so that tests,
 * profiles and bench.py can say WHICH kernels a number was measured on.  buf receives a NUL-terminated string.
 *
 * Environment variables read at tfhe_hip_ctx_create / tfhe_hip_pool_create -- the complete supported list:
 *   TFHE_HIP_BR_KERNEL = auto | batch | single | pair            (default auto) run that blind-rotation kernel at
 *                                                                 every batch size instead of picking per size
 *   TFHE_HIP_KS_KERNEL = auto | mfma | sliced | b4 | generic | split  (default auto) likewise for the key switch;
 *                        creation fails with TFHE_HIP_EINVAL when the parameter set cannot run the kernel named:
 *                        mfma needs basebit = 2, 6 <= t <= 13 and n <= 767 (24 column tiles); sliced needs
 *                        4 <= basebit <= 7; b4 needs basebit = 2 and n <= 1023 (four waves a row: the ring of five
 *                        passes 64 KiB of LDS); generic and split run every accepted set.  Within these bounds every
 *                        kernel returns identity_key_switching word for word (tests/test_gpu_ks_shapes.py)
 *   TFHE_HIP_POOL_RCCL = 0 | 1 | 2    pools: 0 never use RCCL (peer copies only), 1 (default) RCCL when the pool's
 *                                      devices are distinct, 2 also for a pool of one (plumbing test)
 *   TFHE_HIP_POOL_PINNED_STAGING = 0 | 1   pools: stage pageable operands through per-member pinned arenas
 *                                      (default: 1 for pools of several members)
 * Anything else (crossover counts, chunk counts, ring depths) is compiled in: constants of the kernels and of the
 * dispatch, with no override. */
int tfhe_hip_describe_dispatch(tfhe_hip_ctx *ctx, size_t count, char *buf, size_t buflen);

/* How this context's blind-rotation kernels round the external product (KlemsaProcessor::fft's `round() as i64 as u32`,
 * src/fft/klemsa.rs:145-146): "fast" when the parameter set bounds the pre-rounding magnitude below 2^51
 * (2l * N * Bg/2 * 2^31: the 128 / 110 / 80-bit sets) and one add does it, "general" otherwise (|x| < 2^63: the
 * multiple of 2^32 is peeled off first; the l = 1 and l = 2 message-space sets).  Both give the reference's bits
 * wherever the f64 product is exact.  Chosen at tfhe_hip_ctx_create from (l, bgbit); constant for the context. */
const char *tfhe_hip_rounding_mode(const tfhe_hip_ctx *ctx);

/* Block until everything this context enqueued -- on its own stream and on the caller's stream of the
 * last *_dev call -- has finished.  Returns TFHE_HIP_EINVAL (and clears the condition) if a
 * tfhe_hip_batch_gates_mixed_dev launch since the last call met a gate code outside tfhe_hip_gate. */
int tfhe_hip_synchronize(tfhe_hip_ctx *ctx);

/* ---- several GPUs behind one handle --------------------------------------------------------------
 * Replaces: the Rayon `par_map` the reference's batch functions run on
 * (src/parallel/rayon_impl.rs:40-47, called from src/gates.rs:357-383, src/trgsw.rs:289-305): an
 * order-preserving, embarrassingly parallel map over the ciphertexts of a slice under one shared read-only
 * &CloudKey.  A pool is that map over devices: one context per entry of `devices` (an entry may repeat: two
 * contexts on one GPU), the cloud key generated / uploaded once on the first device and replicated device to
 * device in the engine layouts, the batch split contiguously over the first k = min(ndev, ceil(count / 256))
 * members (shard r of k = tfhe_hip_pool_shard; batches under 256 ciphertexts per device are not cut thinner: a
 * device runs that many in the time of one), one host thread per shard, results written into the caller's output
 * slice in input order.  No collective and no
 * exchange between devices on the data path.  Pool calls are serialised per pool; a member context borrowed
 * with tfhe_hip_pool_ctx() (for the *_dev entry points) must not be used while a pool call runs. */
typedef struct tfhe_hip_pool tfhe_hip_pool;

int tfhe_hip_pool_create(const tfhe_hip_params *params, const int *devices, int ndev, tfhe_hip_pool **out);
void tfhe_hip_pool_destroy(tfhe_hip_pool *pool);
int tfhe_hip_pool_size(const tfhe_hip_pool *pool);
/* How the pool's last cloud key reached the members: "rccl" (one grouped ncclBroadcast per key buffer over xGMI,
 * in place in the engine layouts; librccl is opened at run time; used when the pool's devices are distinct; the
 * communicator is created once per pool, on first use, and lives until tfhe_hip_pool_destroy) or
 * "peer-copy" (serial hipMemcpyPeer from member 0: the fallback, and what pools with a repeated device use).
 * TFHE_HIP_POOL_RCCL=0 disables the RCCL path. */
const char *tfhe_hip_pool_key_transport(const tfhe_hip_pool *pool);
/* A key view of a pool: one tfhe_hip_key_create view per member (same devices, streams and scratch), accepted by
 * every tfhe_hip_pool_* entry point; tfhe_hip_pool_destroy(view) frees only its keys.  Destroy views first. */
int tfhe_hip_pool_key_create(tfhe_hip_pool *pool, tfhe_hip_pool **key_view);
/* A member context, BORROWED: valid until tfhe_hip_pool_destroy, never to be passed to tfhe_hip_ctx_destroy. */
tfhe_hip_ctx *tfhe_hip_pool_ctx(tfhe_hip_pool *pool, int member);
/* Text of the last failed pool call ("device D: ..."), or of the last failed create when pool == NULL. */
const char *tfhe_hip_pool_last_error(const tfhe_hip_pool *pool);
/* [lo, hi) of shard `shard` of `nshards` over `count` items: contiguous, sizes differ by at most one, earlier
 * shards take the remainder (the split every pool batch call uses). */
void tfhe_hip_pool_shard(size_t count, int shard, int nshards, size_t *lo, size_t *hi);
/* Members a batch of `count` is actually spread over (= the nshards of its split): min(size, ceil(count / 256)),
 * at least 1 -- one device runs up to 256 ciphertexts in the time of one, so small batches are not cut thinner. */
int tfhe_hip_pool_members_for(const tfhe_hip_pool *pool, size_t count);

/* Cloud key for every member: same arguments and meaning as the tfhe_hip_*_cloud_key calls above. */
int tfhe_hip_pool_load_cloud_key(tfhe_hip_pool *pool, const double *bsk, const uint32_t *ksk, uint32_t decomp_offset,
                                 const uint32_t *testvec);
int tfhe_hip_pool_gen_cloud_key_secure(tfhe_hip_pool *pool, const uint32_t *key_lv0, const uint32_t *key_lv1,
                                       double alpha_ksk, double alpha_bsk);
int tfhe_hip_pool_gen_cloud_key_with_key(tfhe_hip_pool *pool, const uint32_t *key_lv0, const uint32_t *key_lv1,
                                         double alpha_ksk, double alpha_bsk, const uint8_t rng_key[32]);
int tfhe_hip_pool_gen_cloud_key(tfhe_hip_pool *pool, const uint32_t *key_lv0, const uint32_t *key_lv1,
                                double alpha_ksk, double alpha_bsk, uint64_t seed); /* TEST / BENCHMARK ONLY */
/* tfhe_hip_load_compressed_cloud_key on the first member, then the expanded key replicated as for a full load. */
int tfhe_hip_pool_load_compressed_cloud_key(tfhe_hip_pool *pool, const uint8_t mask_seed[32], const uint32_t *bsk_bodies,
                                            const uint32_t *ksk_bodies, uint32_t decomp_offset, const uint32_t *testvec);
int tfhe_hip_pool_export_cloud_key(tfhe_hip_pool *pool, int member, double *bsk, uint32_t *ksk,
                                   uint32_t *decomp_offset, uint32_t *testvec);
/* Packing key switch on a pool: every member loads the packing key; a batch is split in whole groups of N over the
 * members, in input order (the _dev form through the grouped scatter / gather, a last partial group on home). */
int tfhe_hip_pool_load_packing_key(tfhe_hip_pool *pool, const uint8_t mask_seed[32], const uint32_t *bodies);
/* tfhe_hip_gen_packing_key on the first member; every other member loads the same (mask_seed, bodies) -- from a host
 * buffer of the call's own when `bodies` is NULL.  Takes a pool or a pool key view. */
int tfhe_hip_pool_gen_packing_key(tfhe_hip_pool *pool, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha,
                                  const uint8_t rng_key[32], uint8_t mask_seed[32], uint32_t *bodies);
int tfhe_hip_pool_batch_pack_tlwe(tfhe_hip_pool *pool, const uint32_t *in, size_t count, uint32_t *out);
int tfhe_hip_pool_batch_pack_tlwe_dev(tfhe_hip_pool *pool, int home_member, const uint32_t *in, size_t count,
                                      uint32_t *out, void *stream);
/* Unpacking key switch on a pool (same arguments and result as tfhe_hip_batch_unpack_trlwe[_dev]).  With slots NULL the
 * batch is cut on group boundaries, so a member receives only the whole groups it unpacks (the _dev form through the
 * grouped scatter / gather, the outputs of a last partial group on home).  With slots given the outputs are split in
 * input order and every member may receive all groups. */
int tfhe_hip_pool_batch_unpack_trlwe(tfhe_hip_pool *pool, const uint32_t *trlwe, size_t groups, const uint32_t *slots,
                                     size_t count, uint32_t *out);
int tfhe_hip_pool_batch_unpack_trlwe_dev(tfhe_hip_pool *pool, int home_member, const uint32_t *trlwe, size_t groups,
                                         const uint32_t *slots, size_t count, uint32_t *out, void *stream);
/* The tree bootstrap on a pool, HOST pointers (same arguments and result as tfhe_hip_batch_bootstrap_bivariate): the
 * batch is cut by count over the members in input order, every member gets the tables whole.  Needs the cloud key
 * and tfhe_hip_pool_load_packing_key. */
int tfhe_hip_pool_batch_bootstrap_bivariate(tfhe_hip_pool *pool, const uint32_t *x, const uint32_t *y,
                                            const uint32_t *testvecs, int m, int n_luts, int keyswitch, uint32_t *out,
                                            size_t count);

/* The batched hot path over all members, HOST pointers: same arguments and semantics as the single-context host
 * entry points of the same name (gates.rs:352-547; gates.rs:157-199; bootstrap/{vanilla,lut}.rs; trgsw.rs:289-305;
 * tlwe.rs:129-214).  One host thread per shard; results land in the caller's output slice in input order.
 * Small calls (gate / gates_mixed[_nks] / bootstrap / lincomb_bootstrap / mux / blind_rotate of at most the combining bound, see tfhe_hip_set_combining)
 * made by concurrent threads do not queue on the pool: each goes to the member (one per distinct device) with the least
 * work queued and shares launches there with the other threads' calls. */
int tfhe_hip_pool_batch_gate(tfhe_hip_pool *pool, int gate, const uint32_t *a, const uint32_t *b, uint32_t *out,
                             size_t count);
int tfhe_hip_pool_batch_gates_mixed(tfhe_hip_pool *pool, const uint8_t *gates, const uint32_t *a, const uint32_t *b,
                                    uint32_t *out, size_t count);
int tfhe_hip_pool_batch_gates_mixed_nks(tfhe_hip_pool *pool, const uint8_t *gates, const uint32_t *a, const uint32_t *b,
                                        uint32_t *out, size_t count);
int tfhe_hip_pool_batch_bootstrap(tfhe_hip_pool *pool, const uint32_t *in, const uint32_t *testvec, int per_ct,
                                  int keyswitch, uint32_t *out, size_t count);
int tfhe_hip_pool_batch_tlwe_lincomb(tfhe_hip_pool *pool, uint32_t ca, const uint32_t *a, uint32_t cb, const uint32_t *b,
                                     uint32_t cconst, uint32_t *out, size_t count);
int tfhe_hip_pool_batch_lincomb_bootstrap(tfhe_hip_pool *pool, uint32_t ca, const uint32_t *a, uint32_t cb,
                                          const uint32_t *b, uint32_t cconst, const uint32_t *testvec, int per_ct,
                                          int keyswitch, uint32_t *out, size_t count);
/* (many-LUT: never combined; each member's [k][m] result is placed into the caller's [k][count]) */
int tfhe_hip_pool_batch_lincomb_bootstrap_many(tfhe_hip_pool *pool, uint32_t ca, const uint32_t *a, uint32_t cb,
                                               const uint32_t *b, uint32_t cconst, const uint32_t *testvec, int per_ct,
                                               int n_luts, int keyswitch, uint32_t *out, size_t count);
int tfhe_hip_pool_batch_mux(tfhe_hip_pool *pool, int naive, const uint32_t *a, const uint32_t *b, const uint32_t *c,
                            uint32_t *out, size_t count);
int tfhe_hip_pool_batch_blind_rotate(tfhe_hip_pool *pool, const uint32_t *in, const uint32_t *testvec,
                                     uint32_t *out_trlwe, size_t count);

/* The same calls for a batch that is RESIDENT ON ONE MEMBER'S GPU.
 * Replaces: the same Rayon par_map (src/parallel/rayon_impl.rs:40-47, src/gates.rs:357-383) for a caller whose
 * ciphertexts already live in device memory -- the levels of a circuit, the output of a previous pool call -- and
 * that has no torch.distributed to shard them with: every operand and the result are DEVICE pointers on member
 * `home_member`'s GPU, and `stream` is a stream of that GPU (NULL = the member context's own).  The call only
 * ENQUEUES, like the single-context *_dev calls:
 *   - the batch is cut as tfhe_hip_pool_shard cuts it over tfhe_hip_pool_members_for(count) members; shard r runs on
 *     member (home_member + r) mod size, so shard 0 -- and any batch too small to cut -- never leaves home;
 *   - every other shard travels to its member and its result back by ONE grouped ncclSend / ncclRecv pair per
 *     operand and peer over the pool's persistent RCCL communicator (all xGMI links concurrently; shared operands
 *     such as one test vector for the batch are sent whole to every peer), or by hipMemcpyPeerAsync behind events
 *     when the pool has no communicator (a repeated device, no librccl, TFHE_HIP_POOL_RCCL=0) --
 *     tfhe_hip_pool_data_transport() says which ran;
 *   - members compute on their own streams, home on `stream`; work enqueued on `stream` after the call sees the
 *     complete result (the gather is ordered into `stream`).  Results are in input order.
 * Errors detected while enqueueing are returned; tfhe_hip_pool_synchronize() drains the members' streams and reports
 * device-side conditions (see tfhe_hip_synchronize).  The members must not be used through tfhe_hip_pool_ctx() by
 * other threads meanwhile.  gates (mixed forms) is a device pointer too. */
int tfhe_hip_pool_batch_gate_dev(tfhe_hip_pool *pool, int home_member, int gate, const uint32_t *a, const uint32_t *b,
                                 uint32_t *out, size_t count, void *stream);
int tfhe_hip_pool_batch_gates_mixed_dev(tfhe_hip_pool *pool, int home_member, const uint8_t *gates, const uint32_t *a,
                                        const uint32_t *b, uint32_t *out, size_t count, void *stream);
int tfhe_hip_pool_batch_gates_mixed_nks_dev(tfhe_hip_pool *pool, int home_member, const uint8_t *gates,
                                            const uint32_t *a, const uint32_t *b, uint32_t *out, size_t count,
                                            void *stream);
int tfhe_hip_pool_batch_bootstrap_dev(tfhe_hip_pool *pool, int home_member, const uint32_t *in, const uint32_t *testvec,
                                      int per_ct, int keyswitch, uint32_t *out, size_t count, void *stream);
int tfhe_hip_pool_batch_tlwe_lincomb_dev(tfhe_hip_pool *pool, int home_member, uint32_t ca, const uint32_t *a,
                                         uint32_t cb, const uint32_t *b, uint32_t cconst, uint32_t *out, size_t count,
                                         void *stream);
int tfhe_hip_pool_batch_lincomb_bootstrap_dev(tfhe_hip_pool *pool, int home_member, uint32_t ca, const uint32_t *a,
                                              uint32_t cb, const uint32_t *b, uint32_t cconst, const uint32_t *testvec,
                                              int per_ct, int keyswitch, uint32_t *out, size_t count, void *stream);
int tfhe_hip_pool_batch_lincomb_bootstrap_many_dev(tfhe_hip_pool *pool, int home_member, uint32_t ca, const uint32_t *a,
                                                   uint32_t cb, const uint32_t *b, uint32_t cconst,
                                                   const uint32_t *testvec, int per_ct, int n_luts, int keyswitch,
                                                   uint32_t *out, size_t count, void *stream);
int tfhe_hip_pool_batch_mux_dev(tfhe_hip_pool *pool, int home_member, int naive, const uint32_t *a, const uint32_t *b,
                                const uint32_t *c, uint32_t *out, size_t count, void *stream);
int tfhe_hip_pool_batch_blind_rotate_dev(tfhe_hip_pool *pool, int home_member, const uint32_t *in,
                                         const uint32_t *testvec, uint32_t *out_trlwe, size_t count, void *stream);

/* Drain every member's own stream (what the *_dev pool calls enqueued on the members); the caller's `stream` is the
 * caller's to synchronise.  Reports the device-side conditions tfhe_hip_synchronize reports. */
int tfhe_hip_pool_synchronize(tfhe_hip_pool *pool);
/* How the last *_dev pool call moved its shards: "rccl", "peer-copy", or "none" (nothing left the home GPU). */
const char *tfhe_hip_pool_data_transport(const tfhe_hip_pool *pool);

/* Measurement: tfhe_hip_set_profiling on every member, plus HIP-event pairs around every shard transfer of the *_dev
 * pool calls.  tfhe_hip_pool_get_transfer_times synchronises those events, returns the sums since the last call and
 * resets them: *_ms_sum over all transfers, *_ms_max the longest single one (transfers to different peers overlap).
 * Each moved shard is bracketed on the member's stream (the receiver of a scatter, the sender of a gather; a
 * gather's bracket opens after the member's compute); on the RCCL path the call's group is bracketed on the home
 * stream too, and a shard's time is the SHORTER of the two: a transfer starts when both ends have reached it, so the
 * end that arrived last brackets the transfer alone and the other one also brackets its wait for the peer.  (When both
 * brackets live on one device -- a self send / receive -- their events are comparable and the time is exact: from the
 * later arrival to the later completion.)
 * comm_create_ms / key_replication_ms are host wall-clock set-up costs and are NOT reset by reading: the creation of
 * the pool's persistent communicator (0 when it has none) and the last replication of a cloud key to the members. */
typedef struct tfhe_hip_pool_transfer_times {
  double scatter_ms_sum, scatter_ms_max;
  double gather_ms_sum, gather_ms_max;
  uint64_t scatter_bytes, gather_bytes;
  uint64_t calls; /* *_dev pool calls since the last read */
  double comm_create_ms, key_replication_ms;
  /* RCCL path: the home stream's bracket around each call's WHOLE group (every peer's transfer; for a gather also the
   * wait for the slowest member's compute), summed over calls -- an upper bound of any one transfer in the group.  Under
   * RCCL between distinct devices a shard's figure above is bounded by it, so *_ms_sum can approach (members - 1) x this:
   * read per-link cost from *_ms_max and the byte counts, not from the sums.  0 on the peer-copy path. */
  double scatter_group_ms_sum, gather_group_ms_sum;
} tfhe_hip_pool_transfer_times;
int tfhe_hip_pool_set_profiling(tfhe_hip_pool *pool, int enabled);
int tfhe_hip_pool_get_transfer_times(tfhe_hip_pool *pool, tfhe_hip_pool_transfer_times *out);

/* ---- circuits: gate / mux / LUT DAGs, scheduled and run natively ------------------------------------------------
 * Replaces the reference's one-gate-at-a-time evaluation of a gate DAG (examples/add_two_numbers.rs:11-50: full_adder
 * / add; examples/lut_add_two_numbers.rs:82-158: the LUT nibble adder).  A circuit has n_inputs input wires (ids
 * 0 .. n_inputs-1); every tfhe_hip_circuit_add_* appends one node and returns its wire id in *wire.  Nodes:
 *   gate(op, a, b)                 Gates::<op> (src/gates.rs:54-150), op a tfhe_hip_gate code, b ignored for COPY
 *   mux(a, b, c)                   Gates::mux (src/gates.rs:157-183; the reference formula, not mux_naive)
 *   pbs(ca, a, cb, b, cconst, lut) programmable bootstrap (src/bootstrap/lut.rs:79-99) of ca*a + cb*b, body + cconst,
 *                                  with the test vector add_lut registered ([2][N] u32, N = 1024); b ignored if cb == 0
 *   lincomb(coefs, wires, cconst)  sum coefs[i] * wires[i], body + cconst: TLWE `+` / `-` / scaling, no bootstrap
 *   not(a) = -a, constant(value)   src/gates.rs:202-219 (constant(0) has body 1 - 1/8 as in the reference: 0xE0000001)
 * tfhe_hip_circuit_compile levelises it (no device needed; run calls it too): inputs are level 0, a bootstrap is one
 * level above its deepest operand, a linear node at the level of its deepest operand.  Wires are renumbered into store
 * SLOTS: inputs take slots 0 .. n_inputs-1, each level's outputs one contiguous range.  Per level at most one lincomb
 * launch (linear operands that cannot be folded), one bootstrap-without-key-switch launch (the muxes' two halves), one
 * key-switched gate launch (gates and the muxes' or), then one launch per (lut, coefficients) group.  A bootstrap whose
 * linear operands expand to at most two source wires folds them into its prologue (exact wrapping arithmetic: the
 * words are the reference's).  Bootstraps read their operands out of the store by row index inside the blind
 * rotation; nothing is scattered or gathered between levels.  The indices are built once per (circuit, context, batch
 * size) and kept on the device with the circuit, so a repeated run uploads only its inputs.
 * Bad wire ids, a gate code above COPY, an unknown lut id, adding after compile, and slots x batch >= 2^32 are
 * TFHE_HIP_EINVAL.  A circuit may be shared between threads; destroy it after the work it enqueued is done.  It keeps
 * device state for at most four (context, batch size) pairs, dropping the least recently used. */
typedef struct tfhe_hip_circuit tfhe_hip_circuit;
int tfhe_hip_circuit_create(uint32_t n_inputs, tfhe_hip_circuit **out);
void tfhe_hip_circuit_destroy(tfhe_hip_circuit *circ);
int tfhe_hip_circuit_add_gate(tfhe_hip_circuit *circ, int gate, uint32_t a, uint32_t b, uint32_t *wire);
int tfhe_hip_circuit_add_mux(tfhe_hip_circuit *circ, uint32_t a, uint32_t b, uint32_t c, uint32_t *wire);
int tfhe_hip_circuit_add_lut(tfhe_hip_circuit *circ, const uint32_t *testvec, uint32_t *lut);
int tfhe_hip_circuit_add_pbs(tfhe_hip_circuit *circ, uint32_t ca, uint32_t a, uint32_t cb, uint32_t b, uint32_t cconst,
                             uint32_t lut, uint32_t *wire);
/* Many-LUT bootstrap (tfhe_hip_batch_lincomb_bootstrap_many): the n_luts in {1, 2, 4, 8} functions packed in `lut` of
 * ca*a + cb*b + cconst from ONE blind rotation; wires[0 .. n_luts-1] receive the k consecutive output wires (function j
 * at wires[j]).  Operands fold as for add_pbs.  Compile groups many-LUT nodes by (lut, ca, cb, cconst, k), one launch
 * per group, with function-major slots (node q, function j at base + j * nodes + q); describe counts such a launch in
 * lut_launches and each node once in lut_nodes.  TFHE_HIP_EINVAL: n_luts not in {1, 2, 4, 8}, wires NULL, and the
 * cases of add_pbs. */
int tfhe_hip_circuit_add_pbs_many(tfhe_hip_circuit *circ, uint32_t ca, uint32_t a, uint32_t cb, uint32_t b,
                                  uint32_t cconst, uint32_t lut, int n_luts, uint32_t *wires);
int tfhe_hip_circuit_add_lincomb(tfhe_hip_circuit *circ, const uint32_t *coefs, const uint32_t *wires, size_t n_terms,
                                 uint32_t cconst, uint32_t *wire);
int tfhe_hip_circuit_add_not(tfhe_hip_circuit *circ, uint32_t a, uint32_t *wire);
int tfhe_hip_circuit_add_constant(tfhe_hip_circuit *circ, int value, uint32_t *wire);
int tfhe_hip_circuit_compile(tfhe_hip_circuit *circ);
/* The schedule, for tests and tools: *n_levels levels (level 0 = the inputs); for each of the first `cap` levels
 * TFHE_HIP_CIRCUIT_LEVEL_WORDS words: first slot, end slot (exclusive), then (launches, nodes) for the lincomb,
 * bootstrap-without-key-switch, gate and lut launches in that order.  levels may be NULL (count only). */
#define TFHE_HIP_CIRCUIT_LEVEL_WORDS 10
int tfhe_hip_circuit_describe(tfhe_hip_circuit *circ, uint32_t *levels, size_t cap, size_t *n_levels);
/* Slots of the store ([slots][batch][n+1] u32); a wire's slot (0xFFFFFFFF: a linear node, formed where it is read);
 * the slots a bootstrap node's launch reads (up to 3: a mux's a, b, c; for a folded node its source wires'). */
int tfhe_hip_circuit_slots(tfhe_hip_circuit *circ, uint32_t *slots);
int tfhe_hip_circuit_wire_slot(tfhe_hip_circuit *circ, uint32_t wire, uint32_t *slot);
int tfhe_hip_circuit_operand_slots(tfhe_hip_circuit *circ, uint32_t wire, uint32_t *slots, uint32_t *n);
/* Host arrays: inputs [n_inputs][batch][n+1] -> out [n_out][batch][n+1], wire out_wires[k] in out[k].  Holds the
 * context's lock for the whole run (a key change cannot interleave); needs a loaded key. */
int tfhe_hip_circuit_run(tfhe_hip_ctx *ctx, tfhe_hip_circuit *circ, const uint32_t *inputs, size_t batch,
                         const uint32_t *out_wires, size_t n_out, uint32_t *out);
/* Device store `wires` [slots][batch][n+1] on the context's GPU; `inputs` [n_inputs][batch][n+1] is copied into slots
 * 0 .. n_inputs-1 first (NULL: already there).  Enqueue only.  Replaces the per-level torch gathers of Circuit.run_dev. */
int tfhe_hip_circuit_run_dev(tfhe_hip_ctx *ctx, tfhe_hip_circuit *circ, const uint32_t *inputs, uint32_t *wires,
                             size_t batch, void *stream);
/* out [n_out][batch][n+1] = wires out_wires[k] (caller's numbering) read out of a run's store; a linear node is formed
 * from its sources here.  out_wires is a host array. */
int tfhe_hip_circuit_gather_dev(tfhe_hip_ctx *ctx, tfhe_hip_circuit *circ, const uint32_t *wires, size_t batch,
                                const uint32_t *out_wires, size_t n_out, uint32_t *out, void *stream);
/* The same through a pool: the store lives on member `home`; each level's operands are gathered into staging there
 * and go through tfhe_hip_pool_batch_gates_mixed[_nks]_dev / _lincomb_bootstrap_dev (cut over the members).  The
 * host form keeps the store on member 0.  Runs of one circuit through one pool -- or through key views of it, which
 * share its members -- are serialised by the library, whatever the threads and streams; the staging is the circuit's. */
int tfhe_hip_circuit_run_pool(tfhe_hip_pool *pool, tfhe_hip_circuit *circ, const uint32_t *inputs, size_t batch,
                              const uint32_t *out_wires, size_t n_out, uint32_t *out);
int tfhe_hip_circuit_run_pool_dev(tfhe_hip_pool *pool, int home_member, tfhe_hip_circuit *circ, const uint32_t *inputs,
                                  uint32_t *wires, size_t batch, void *stream);
int tfhe_hip_circuit_gather_pool_dev(tfhe_hip_pool *pool, int home_member, tfhe_hip_circuit *circ, const uint32_t *wires,
                                     size_t batch, const uint32_t *out_wires, size_t n_out, uint32_t *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TFHE_HIP_H */
