// sym_encrypt.hpp -- symmetric (secret-key) TLWE lv0 encryption on the GPU, behind the C ABI: bulk ciphertexts, the
// public key's encryptions of zero and the symmetric proxy re-encryption key.
//
// The format is normative in include/tfhe_hip.h ("symmetric encryption").  All three are launches of the library's LWE
// row kernel, k_lwe_rows (keygen.hpp): the row (a, <a, s0> + plain + f64_to_torus(noise)) with the mask a under
// (mask key, g, mask domain) and the one noise sample under (K, g, noise domain), no stream number.
//
//   bulk TLWE        g = first_index + m, masks under the public seed S ("EWL": the seeded-TLWE masks), out [count][n+1]
//                    and / or bodies [count]; bodies-only mode stages and stores no mask.
//   public key       g = e < size, masks under K, plain 0, out [size][n+1]; k_pke_planes builds the byte planes from it.
//   re-encryption    g = base t i + base j + k, plain from (i, j, k) and key_from in the kernel, k = 0 rows zero, out
//                    in the engine layout of the key-switching key (rows of ksk_row_words(n), zero padding): what
//                    k_ksk_convert would have made, so no conversion pass follows.
#pragma once
#include "pk_encrypt.hpp"

// ---- symmetric encryption (sym_encrypt.hpp) -----------------------------------------------------------------------
namespace {
// The secrets of one launch, through a SecretStage over the context's `sym_sec`: K, s0 [n], key_from [n] (or nothing)
size_t sym_sec_bytes(const tfhe_hip_ctx *ctx, bool key_rows) { return (8 + (size_t)ctx->P.n * (key_rows ? 2 : 1)) * 4; }
static_assert((8 + 2 * (size_t)kLweMaxN) * 4 <= kSecretImageMax, "the largest image a call stages");
int sym_land(tfhe_hip_ctx *ctx, SecretStage &sec, const ChaChaKey &k, const uint32_t *key_lv0, const uint32_t *key_from) {
  const size_t n4 = (size_t)ctx->P.n * 4;
  sec.put(k.k, 32, 0);
  sec.put(key_lv0, n4, 32);
  if (key_from) sec.put(key_from, n4, 32 + n4);
  return sec.land("symmetric encryption: ");
}

// `rows` rows from index `first_index` over the staged secrets (sym_land), under the indexed domains dom_mask /
// dom_noise; masks under `seed`, or (NULL) under K.  plain / bodies / out are device pointers, any may be NULL.
int sym_launch(tfhe_hip_ctx *ctx, const SecretStage &staged, const ChaChaKey *seed, uint32_t dom_mask, uint32_t dom_noise,
               uint64_t first_index, size_t rows, double alpha, const uint32_t *plain, bool key_rows, uint32_t *bodies,
               uint32_t *out, int stride, hipStream_t s) {
  const uint32_t *sec = staged.dev(0);
  LweRowJob j{};
  if (seed) j.seed = *seed;
  j.k = (const ChaChaKey *)sec;
  j.mask_under_k = !seed;
  j.dom_mask = dom_mask;
  j.dom_noise = dom_noise;
  j.first_index = first_index;
  j.rows = rows;
  j.alpha = alpha;
  j.s0 = sec + 8;
  j.plain = plain;
  j.key_rows = key_rows;
  j.key_from = key_rows ? sec + 8 + ctx->P.n : nullptr;
  j.bodies = bodies;
  j.out = out;
  j.stride = stride;
  return lwe_rows_launch(ctx, j, s);
}

const char *sym_refusal(const tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *plain, size_t count, double alpha,
                        const uint8_t *mask_seed, uint64_t first_index, const uint32_t *bodies, const uint32_t *out) {
  if (!key_lv0 || !mask_seed || !plain) return "null pointer";
  if (count && !bodies && !out) return "no output: bodies and out are both null";
  if (!(alpha >= 0.0)) return "negative noise parameter";
  if (count && first_index + (uint64_t)(count - 1) < first_index) return "the row indices run past 2^64";
  if (count > 0x7FFFFFFFull) return "count too large";
  return nullptr;
}

// on stream s: stage, launch, wipe.  plain / bodies / out are device pointers.
int sym_bulk(tfhe_hip_ctx *ctx, const ChaChaKey &seed, const ChaChaKey &k, const uint32_t *key_lv0, const uint32_t *plain,
             size_t count, double alpha, uint64_t first_index, uint32_t *bodies, uint32_t *out, hipStream_t s) {
  SecretStage sec(ctx, ctx->sym_sec, s, sym_sec_bytes(ctx, false));
  int rc = sym_land(ctx, sec, k, key_lv0, nullptr);
  if (rc == TFHE_HIP_OK)
    rc = sym_launch(ctx, sec, &seed, kSeedDomainTlwe, kSeedDomainSymNoise, first_index, count, alpha, plain, false, bodies, out,
                    ctx->P.n + 1, s);
  return sec.finish(rc);
}
}  // namespace

int tfhe_hip_batch_encrypt(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *plain, size_t count, double alpha,
                           const uint8_t rng_key[32], const uint8_t mask_seed[32], uint64_t first_index,
                           uint32_t *bodies, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (const char *why = sym_refusal(ctx, key_lv0, plain, count, alpha, mask_seed, first_index, bodies, out))
    return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  const ChaChaKey seed = seed_key(mask_seed);
  return encrypt_host_call(ctx, plain, count, bodies, count * 4, out, tlwe_bytes(ctx, count),
                           [&](const uint32_t *d_plain, uint32_t *d_bodies, uint32_t *d_out) {
                             return sym_bulk(ctx, seed, gk.k, key_lv0, d_plain, count, alpha, first_index, d_bodies, d_out, ctx->stream);
                           });
}

int tfhe_hip_batch_encrypt_dev(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *plain, size_t count, double alpha,
                               const uint8_t rng_key[32], const uint8_t mask_seed[32], uint64_t first_index,
                               uint32_t *bodies, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (const char *why = sym_refusal(ctx, key_lv0, plain, count, alpha, mask_seed, first_index, bodies, out))
    return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  return sym_bulk(ctx, seed_key(mask_seed), gk.k, key_lv0, plain, count, alpha, first_index, bodies, out, pick(ctx, stream));
}

// The public key (proxy_reenc.rs:125-153): `size` encryptions of zero made on the device, then the byte planes by
// the kernel tfhe_hip_load_public_key runs: the handle holds bit for bit what loading encryptions_out would build.
int tfhe_hip_gen_public_key(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, size_t size, double alpha, const uint8_t rng_key[32],
                            uint32_t *encryptions_out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  // validation first: a refused call leaves the old public key encrypting
  if (!key_lv0) return fail(ctx, TFHE_HIP_EINVAL, "null key pointer");
  if (size < 1 || size > (size_t)kPkeMaxSize)
    return fail(ctx, TFHE_HIP_EINVAL, "public key size must be in [1, 8192] (exact i32 accumulation)");
  if (!(alpha >= 0.0)) return fail(ctx, TFHE_HIP_EINVAL, "negative noise parameter");
  const tfhe_hip_params &P = ctx->P;
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  KeyState &k = *ctx->K;
  const size_t bytes = pke_plane_bytes(P.n, (int)size), chunks = bytes / 16, enc_bytes = size * (size_t)(P.n + 1) * 4;
  CHK(begin_side_key(ctx, k.pke_loaded, k.d_pke8, bytes));
  SecretStage sec(ctx, ctx->sym_sec, ctx->stream, sym_sec_bytes(ctx, false), true);  // (wiped on every exit path)
  CHK(sym_land(ctx, sec, gk.k, key_lv0, nullptr));
  CHK(upload_through_temp(ctx, "public key generation", {}, enc_bytes, [&](void *d_enc) -> hipError_t {
    if (sym_launch(ctx, sec, nullptr, kSeedDomainPkMask, kSeedDomainPkNoise, 0, size, alpha, nullptr, false, nullptr,
                   (uint32_t *)d_enc, P.n + 1, ctx->stream) != TFHE_HIP_OK)
      return hipErrorLaunchFailure;
    hipLaunchKernelGGL(k_pke_planes<256>, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const uint32_t *)d_enc, k.d_pke8, P.n, (int)size, chunks);
    if (const hipError_t e = hipGetLastError()) return e;
    if (encryptions_out) return hipMemcpyAsync(encryptions_out, d_enc, enc_bytes, hipMemcpyDeviceToHost, ctx->stream);
    return hipSuccess;
  }));
  k.pke_size = (int)size;
  commit_side_key(k.pke_loaded);
  return TFHE_HIP_OK;
}

// The symmetric re-encryption key (proxy_reenc.rs:362-425): n t base rows written straight into the engine layout of
// d_ksk (the rows past n t base stay zero: a source of n coefficients); key_out, when asked for, is the export of it.
int tfhe_hip_gen_reenc_key_symmetric(tfhe_hip_ctx *ctx, const uint32_t *key_from, const uint32_t *key_to, double alpha,
                                     const uint8_t rng_key[32], uint32_t *key_out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  // validation first: a refused call leaves the handle's keys as they were
  if (!key_from || !key_to) return fail(ctx, TFHE_HIP_EINVAL, "null key pointer");
  const tfhe_hip_params &P = ctx->P;
  if (P.n > kN) return fail(ctx, TFHE_HIP_EINVAL, "proxy re-encryption needs n <= N = 1024 (this parameter set's n is larger)");
  if (!(alpha >= 0.0)) return fail(ctx, TFHE_HIP_EINVAL, "negative noise parameter");
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  CHK(begin_key_change(ctx, KEY_BUF_KSK));  // (both flags go: the buffer is shared with a cloud key's key-switching key)
  const int base = 1 << P.basebit;
  const size_t rows = (size_t)P.n * P.t * base, key_words = rows * (size_t)(P.n + 1);
  SecretStage sec(ctx, ctx->sym_sec, ctx->stream, sym_sec_bytes(ctx, true), true);  // (wiped on every exit path)
  CHK(sym_land(ctx, sec, gk.k, key_to, key_from));
  if (const hipError_t e = hipMemsetAsync(ctx->K->d_ksk, 0, ksk_bytes(P), ctx->stream))
    return fail(ctx, TFHE_HIP_EHIP, std::string("re-encryption key generation: ") + hipGetErrorString(e));
  CHK(sym_launch(ctx, sec, nullptr, kSeedDomainRkMask, kSeedDomainRkNoise, 0, rows, alpha, nullptr, true, nullptr, ctx->K->d_ksk,
                 ksk_row_words(P.n), ctx->stream));
  if (key_out)
    CHK(upload_through_temp(ctx, "re-encryption key export", {}, key_words * 4, [&](void *d_ref) -> hipError_t {
      if (const hipError_t e = ksk_export_launch(ctx, (uint32_t *)d_ref, rows)) return e;
      return hipMemcpyAsync(key_out, d_ref, key_words * 4, hipMemcpyDeviceToHost, ctx->stream);
    }));
  return commit_reenc_key(ctx);
}
