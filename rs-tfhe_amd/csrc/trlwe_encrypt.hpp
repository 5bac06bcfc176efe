// trlwe_encrypt.hpp -- packed TRLWE lv1 encryption on the GPU, behind the C ABI: full ciphertexts, the seeded
// (bodies-only) form and its expansion.
//
// The format is normative in include/tfhe_hip.h ("packed encryption").  Group m of a batch is the TRLWE
// (a, a (*) s1 + e + plain[m N ..]) of TRLWELv1::encrypt_f64 (trlwe.rs:30-53) with index g = first_group + m: the mask
// a in natural order under (S, g, "ERL"), the noise e in the BSK generators' word order under (K, g, "ERN"), no stream
// number.  The row is the one k_gen_packing_key (packing_keygen.hpp) builds, from the same pieces of keygen.hpp:
//
//   k_trlwe_rows     one wave (one workgroup) per group: natural_mask<STORE> under S, row_noise under K,
//                    add_ring_product against the staged spectrum of s1 (exact, |coefficients| < 2^41), the lane's 16
//                    plaintext words (none at or past `count`), store_row to out[m][1] and / or bodies[m].  With
//                    out == NULL no mask is stored.  A wave takes one group: the grid is the number of groups.
//   k_expand_trlwe   no secret: one wave per group writes its 64 keystream blocks as whole dwordx4 chunks into
//                    out[m][0] and copies the bodies into out[m][1].
//
// Secrets travel as in sym_encrypt.hpp, through a SecretStage (secrets.hpp) over the context's `sym_sec` buffer:
// K [8 words], s1 [N words] and the spectrum of s1 [N / 2 double2] (k_key_spectrum, as stage_secrets runs it -- the
// spectrum is secret too).  The host copy is wiped, and the buffer is zeroed behind the kernel on the same stream.
#pragma once
#include "internal.hpp"

namespace tfhe {

// One wave per group m = blockIdx.x.  plain: [count]; out: [groups][2][N] or NULL; bodies: [groups][N] or NULL.
__global__ __launch_bounds__(64) void k_trlwe_rows(const double2 *__restrict__ s1_spec, const double2 *__restrict__ twt,
                                                    const ChaChaKey *__restrict__ key_p, ChaChaKey seed, uint64_t first_group,
                                                    const uint32_t *__restrict__ plain, size_t count, double alpha,
                                                    uint32_t *__restrict__ bodies, uint32_t *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double2 *tile = reinterpret_cast<double2 *>(smem);
  const int lane = threadIdx.x;
  const size_t m = blockIdx.x;
  const uint64_t g = first_group + (uint64_t)m;
  const uint32_t g_lo = (uint32_t)g, g_hi = TFHE_MUT(kMut_trlwe_group_hi) ? 0u : (uint32_t)(g >> 32);
  Twiddles tw;
  tw.load(twt, reinterpret_cast<double2 *>(smem + kTileBytes), lane);
  uint32_t *dst_a = out ? out + m * (size_t)(2 * kN) : nullptr;
  uint32_t a_lo[8], a_hi[8], b_lo[8], b_hi[8];
  if (dst_a) natural_mask<true>(seed, g_lo, g_hi, kSeedDomainTrlweMask, reinterpret_cast<uint32_t *>(smem), lane, dst_a, a_lo, a_hi);
  else natural_mask<false>(seed, g_lo, g_hi, kSeedDomainTrlweMask, reinterpret_cast<uint32_t *>(smem), lane, nullptr, a_lo, a_hi);
  row_noise(*key_p, g_lo, g_hi, kSeedDomainTrlweNoise, alpha, lane, b_lo, b_hi);
  double are[8], aim[8];
  add_ring_product(a_lo, a_hi, s1_spec, tw, tile, lane, are, aim, b_lo, b_hi);
  // the lane's plaintext words, after the product, wrapping; the slots at or past `count` encrypt 0 and are not read
  const size_t base = m * (size_t)kN + (size_t)lane;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const size_t lo = base + (size_t)(64 * q), hi = lo + (size_t)kN2;
    if (lo < count) b_lo[q] += plain[lo];
    if (hi < count) b_hi[q] += plain[hi];
  }
  if (dst_a) store_row(dst_a + kN, lane, b_lo, b_hi);
  if (bodies) store_row(bodies + m * (size_t)kN, lane, b_lo, b_hi);
}

// One wave per group, WAVES groups a workgroup (the waves share nothing).  bodies: [groups][N], out: [groups][2][N],
// both 16-byte aligned.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_expand_trlwe(ChaChaKey seed, uint64_t first_group,
                                                             const uint32_t *__restrict__ bodies, size_t groups,
                                                             uint32_t *__restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t m = (size_t)blockIdx.x * WAVES + (size_t)wave;
  if (m >= groups) return;  // (wave-uniform; nothing below synchronises)
  const uint64_t g = first_group + (uint64_t)m;
  uint32_t w[16];
  chacha20_block(seed, (uint32_t)lane, (uint32_t)g, TFHE_MUT(kMut_trlwe_group_hi) ? 0u : (uint32_t)(g >> 32), kSeedDomainTrlweMask, w);
  uint4 *dst = reinterpret_cast<uint4 *>(out + m * (size_t)(2 * kN));
  const uint4 *src = reinterpret_cast<const uint4 *>(bodies + m * (size_t)kN);
#pragma unroll
  for (int q = 0; q < 4; ++q) dst[lane * 4 + q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
#pragma unroll
  for (int q = 0; q < 4; ++q) dst[kN / 4 + 64 * q + lane] = src[64 * q + lane];
}

}  // namespace tfhe

// ---- packed encryption (trlwe_encrypt.hpp) --------------------------------------------------------------------------
namespace {
constexpr int kTrlweExpandWaves = 4;
// the staged secrets in sym_sec: K at word 0, s1 at word 8, the spectrum of s1 behind it (16-byte aligned)
constexpr size_t kTrlweSecSpecAt = (8 + (size_t)kN) * 4;
constexpr size_t kTrlweSecBytes = kTrlweSecSpecAt + (size_t)kN2 * sizeof(double2);
static_assert(kTrlweSecSpecAt % 16 == 0, "the spectrum is read as double2");

size_t trlwe_groups(size_t count) { return (count + (size_t)kN - 1) / (size_t)kN; }
bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
bool groups_wrap(uint64_t first_group, size_t groups) { return groups && first_group + (uint64_t)(groups - 1) < first_group; }

// the checks both forms share, in sym_refusal's style: why the call is TFHE_HIP_EINVAL, or nullptr
const char *trlwe_enc_refusal(const uint32_t *key_lv1, const uint32_t *plain, size_t count, double alpha, const uint8_t *mask_seed,
                              uint64_t first_group, const uint32_t *bodies, const uint32_t *out) {
  if (!key_lv1 || !mask_seed || !plain) return "null pointer";
  if (count && !bodies && !out) return "no output: bodies and out are both null";
  if (!(alpha >= 0.0)) return "negative noise parameter";
  if (count > 0x7FFFFFFFull) return "count too large";
  if (groups_wrap(first_group, trlwe_groups(count))) return "the group indices run past 2^64";
  for (int x = 0; x < kN; ++x)
    if (key_lv1[x] > 1u) return "secret keys are binary";
  return nullptr;
}
const char *trlwe_expand_refusal(const uint8_t *mask_seed, uint64_t first_group, const uint32_t *bodies, size_t groups,
                                 const uint32_t *out) {
  if (!mask_seed || !bodies || !out) return "null pointer";
  if (groups > 0x7FFFFFFFull) return "groups too large";
  if (groups_wrap(first_group, groups)) return "the group indices run past 2^64";
  return nullptr;
}

// on stream s: stage K, s1 and the spectrum of s1, launch, wipe.  plain / bodies / out are device pointers.
int trlwe_bulk(tfhe_hip_ctx *ctx, const ChaChaKey &seed, const ChaChaKey &k, const uint32_t *key_lv1, const uint32_t *plain,
               size_t count, double alpha, uint64_t first_group, uint32_t *bodies, uint32_t *out, hipStream_t s) {
  SecretStage sec(ctx, ctx->sym_sec, s, kTrlweSecSpecAt);
  sec.put(k.k, 32, 0);
  sec.put(key_lv1, (size_t)kN * 4, 32);
  int rc = sec.land("packed encryption: ", kTrlweSecBytes);
  if (rc == TFHE_HIP_OK) {
    double2 *d_spec = sec.dev<double2>(kTrlweSecSpecAt);
    rc = key_spectrum_launch(ctx, sec.dev(32), d_spec, s);
    if (rc == TFHE_HIP_OK) {
      hipLaunchKernelGGL(k_trlwe_rows, dim3((unsigned)trlwe_groups(count)), dim3(64), kStageLdsBytes, s, (const double2 *)d_spec,
                         ctx->d_tw, sec.dev<const ChaChaKey>(0), seed, first_group, plain, count, alpha, bodies, out);
      rc = launched(ctx);
    }
  }
  return sec.finish(rc);
}

int trlwe_expand_launch(tfhe_hip_ctx *ctx, const ChaChaKey &seed, uint64_t first_group, const uint32_t *bodies, size_t groups,
                        uint32_t *out, hipStream_t s) {
  const size_t per = (size_t)kTrlweExpandWaves;
  hipLaunchKernelGGL(k_expand_trlwe<kTrlweExpandWaves>, dim3((unsigned)((groups + per - 1) / per)), dim3(64 * kTrlweExpandWaves), 0, s,
                     seed, first_group, bodies, groups, out);
  return launched(ctx);
}
}  // namespace

int tfhe_hip_batch_encrypt_trlwe(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const uint32_t *plain, size_t count, double alpha,
                                 const uint8_t rng_key[32], const uint8_t mask_seed[32], uint64_t first_group,
                                 uint32_t *bodies, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (const char *why = trlwe_enc_refusal(key_lv1, plain, count, alpha, mask_seed, first_group, bodies, out))
    return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  const ChaChaKey seed = seed_key(mask_seed);
  const size_t groups = trlwe_groups(count), body_bytes = groups * (size_t)kN * 4;
  return encrypt_host_call(ctx, plain, count, bodies, body_bytes, out, trlwe_bytes(groups),
                           [&](const uint32_t *d_plain, uint32_t *d_bodies, uint32_t *d_out) {
                             return trlwe_bulk(ctx, seed, gk.k, key_lv1, d_plain, count, alpha, first_group, d_bodies, d_out, ctx->stream);
                           });
}

int tfhe_hip_batch_encrypt_trlwe_dev(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const uint32_t *plain, size_t count, double alpha,
                                     const uint8_t rng_key[32], const uint8_t mask_seed[32], uint64_t first_group,
                                     uint32_t *bodies, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (const char *why = trlwe_enc_refusal(key_lv1, plain, count, alpha, mask_seed, first_group, bodies, out))
    return fail(ctx, TFHE_HIP_EINVAL, why);
  if (!aligned16(bodies) || !aligned16(out)) return fail(ctx, TFHE_HIP_EINVAL, "bodies and out must be 16-byte aligned");
  if (count == 0) return TFHE_HIP_OK;
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  return trlwe_bulk(ctx, seed_key(mask_seed), gk.k, key_lv1, plain, count, alpha, first_group, bodies, out, pick(ctx, stream));
}

int tfhe_hip_expand_seeded_trlwe(tfhe_hip_ctx *ctx, const uint8_t mask_seed[32], uint64_t first_group, const uint32_t *bodies,
                                 size_t groups, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (const char *why = trlwe_expand_refusal(mask_seed, first_group, bodies, groups, out)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (groups == 0) return TFHE_HIP_OK;
  const ChaChaKey seed = seed_key(mask_seed);
  return host_call(ctx, false, {{bodies, groups * (size_t)kN * 4, &ctx->a}}, out, trlwe_bytes(groups), [&](const void *const *d, void *o) {
    return trlwe_expand_launch(ctx, seed, first_group, u32(d[0]), groups, (uint32_t *)o, ctx->stream);
  });
}

int tfhe_hip_expand_seeded_trlwe_dev(tfhe_hip_ctx *ctx, const uint8_t mask_seed[32], uint64_t first_group, const uint32_t *bodies,
                                     size_t groups, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (const char *why = trlwe_expand_refusal(mask_seed, first_group, bodies, groups, out)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (!aligned16(bodies) || !aligned16(out)) return fail(ctx, TFHE_HIP_EINVAL, "bodies and out must be 16-byte aligned");
  if (groups == 0) return TFHE_HIP_OK;
  return trlwe_expand_launch(ctx, seed_key(mask_seed), first_group, bodies, groups, out, pick(ctx, stream));
}
