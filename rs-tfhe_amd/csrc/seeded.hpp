// seeded.hpp -- seeded (compressed) cloud keys and fresh ciphertexts, expanded on the GPU.
//
// Every row of the key-switching key, every TRLWE row of the bootstrapping key and every fresh TLWE ciphertext is
// (uniform mask, body).  When the mask is a fixed position of a ChaCha20 keystream under a PUBLIC 32-byte seed S,
// only the bodies travel; the expansion regenerates the masks and writes the engine layouts the existing kernels
// read.  The format (nonces, word order, the q < l body rule of the BSK) is normative and documented in
// include/tfhe_hip.h; keygen.hpp holds the ChaCha20 block function, the stream table every nonce here is named in
// (kStream*, kSeedDomain*), the seed derivation, the ring-row helpers shared with the plain generator, and the LWE
// row kernel k_lwe_rows: the key-switching key's rows (bodies only under S, streams 16 / 17 of "KSK") and the
// expansion of them and of seeded TLWE ciphertexts ("EWL") are launches of it, so only the ring rows have kernels here.
#pragma once
#include "internal.hpp"

namespace tfhe {

// ---- bootstrapping key --------------------------------------------------------------------------------------------
// Row r = i*2l + q of TRGSW(s0[i]), p = s0[i], g_d = f64_to_torus(Bg^-(d+1)), a from S (natural_mask over
// (r, 18, "BSK")), e from (r, 19, "BSK") under K in k_gen_bsk's word order:
//   q <  l: b = a (*) s1 + e - p*g_q*s1      (the reference's a[0] += p*g_q folded into the body: a stays the seed's)
//   q >= l: b = a (*) s1 + e + p*g_{q-l}     (on coefficient 0, as k_gen_bsk)
// computed as (a - p*g*[q < l]) (*) s1 through the FFT of k_gen_bsk (|coefficients| < 2^41: the rounding is exact).
// bodies: [n][2l][N] u32, natural coefficient order.
template <int L>
__global__ __launch_bounds__(64) void k_gen_compressed_bsk(const uint32_t *__restrict__ key_lv0,
                                                            const double2 *__restrict__ s1_spec,
                                                            const double2 *__restrict__ twt, uint32_t *__restrict__ bodies,
                                                            int bgbit, double alpha,
                                                            const ChaChaKey *__restrict__ key_p, ChaChaKey seed) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double2 *tile = reinterpret_cast<double2 *>(smem);
  const int lane = threadIdx.x;
  const uint32_t row = blockIdx.x;
  const int q = row % (2 * L), i = row / (2 * L);
  Twiddles tw;
  tw.load(twt, reinterpret_cast<double2 *>(smem + kTileBytes), lane);
  uint32_t a_lo[8], a_hi[8], b_lo[8], b_hi[8];
  natural_mask<false>(seed, row, kStreamSeededBskMask, kSeedDomainBsk, reinterpret_cast<uint32_t *>(smem), lane, nullptr, a_lo,
                      a_hi);
  row_noise(*key_p, row, kStreamSeededBskNoise, kSeedDomainBsk, alpha, lane, b_lo, b_hi);
  const uint32_t gadget = key_lv0[i] * dev_f64_to_torus(exp2(-(double)(bgbit * (q % L + 1))));
  if (q < L && lane == 0) a_lo[0] -= gadget;
  double are[8], aim[8];
  add_ring_product(a_lo, a_hi, s1_spec, tw, tile, lane, are, aim, b_lo, b_hi);
  if (q >= L && lane == 0) b_lo[0] += gadget;
  store_row(bodies + (size_t)row * kN, lane, b_lo, b_hi);
}

// Spectra of (a from S, b from `bodies`) in the engine layout of k_gen_bsk, scaled by 2 * key_scale(fast).
__global__ __launch_bounds__(64) void k_expand_bsk(const uint32_t *__restrict__ bodies, const double2 *__restrict__ twt,
                                                    double2 *__restrict__ bsk_eng, ChaChaKey seed, double scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double2 *tile = reinterpret_cast<double2 *>(smem);
  const int lane = threadIdx.x;
  const uint32_t row = blockIdx.x;
  Twiddles tw;
  tw.load(twt, reinterpret_cast<double2 *>(smem + kTileBytes), lane);
  uint32_t lo[8], hi[8];
  natural_mask<false>(seed, row, kStreamSeededBskMask, kSeedDomainBsk, reinterpret_cast<uint32_t *>(smem), lane, nullptr, lo, hi);
  const double k2 = 2.0 * scale;
  double2 *dst = bsk_eng + (size_t)row * 2 * kN2;
  double re[8], im[8];
  torus_spectrum(lo, hi, re, im, tw, tile, lane);
#pragma unroll
  for (int s = 0; s < 8; ++s) dst[s * 64 + lane] = make_double2(re[s] * k2, im[s] * k2);
  load_row(bodies + (size_t)row * kN, lane, lo, hi);
  torus_spectrum(lo, hi, re, im, tw, tile, lane);
#pragma unroll
  for (int s = 0; s < 8; ++s) dst[kN2 + s * 64 + lane] = make_double2(re[s] * k2, im[s] * k2);
}

}  // namespace tfhe

// ---- seeded (compressed) cloud keys and ciphertexts (seeded.hpp) ---------------------------------------------
int tfhe_hip_compressed_key_words(const tfhe_hip_params *params, size_t *bsk_words, size_t *ksk_words) {
  if (!params || !bsk_words || !ksk_words || !params_supported(params)) return TFHE_HIP_EINVAL;
  *bsk_words = (size_t)params->n * 2 * params->l * kN;
  *ksk_words = (size_t)kN * params->t * ((size_t)1 << params->basebit);
  return TFHE_HIP_OK;
}

namespace {
// Queues, on ctx->stream, the engine layouts from the bodies at d_bsk_bodies [n][2l][N] / d_ksk_bodies [N][t][base] and
// the masks of `seed`.  ctx->mu held, key buffers allocated (begin_key_change).
hipError_t expand_key_locked(tfhe_hip_ctx *ctx, const ChaChaKey &seed, const uint32_t *d_bsk_bodies, const uint32_t *d_ksk_bodies) {
  const tfhe_hip_params &P = ctx->P;
  hipLaunchKernelGGL(k_expand_bsk, dim3((unsigned)(P.n * 2 * P.l)), dim3(64), kStageLdsBytes, ctx->stream, d_bsk_bodies,
                     ctx->d_tw, ctx->K->d_bsk, seed, key_scale(ctx->dispatch.fast_round));
  if (const hipError_t e = hipGetLastError()) return e;
  // key-switching key: the engine layout of k_ksk_convert (rows of ksk_row_words(n), zero padding, k = 0 rows all zero)
  LweRowJob j{};
  j.seed = seed;
  j.stream_mask = kStreamSeededKskMask;
  j.dom_mask = kSeedDomainKsk;
  j.rows = ksk_rows(P);
  j.plain = d_ksk_bodies;
  j.key_rows = true;
  j.out = ctx->K->d_ksk;
  j.stride = ksk_row_words(P.n);
  return lwe_rows_launch(ctx, j, ctx->stream) == TFHE_HIP_OK ? hipSuccess : hipErrorLaunchFailure;
}

// ctx->mu held, ctx's device current
int gen_compressed_locked(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha_ksk,
                          double alpha_bsk, const ChaChaKey &rk, uint8_t mask_seed[32], uint32_t *bsk_bodies,
                          uint32_t *ksk_bodies, uint32_t *decomp_offset) {
  const tfhe_hip_params &P = ctx->P;
  const size_t bsk_words = (size_t)P.n * 2 * P.l * kN, ksk_words = ksk_rows(P);
  CHK(begin_key_change(ctx, KEY_BUF_ALL));
  StagedSecrets s(ctx);  // (wiped on every exit path)
  CHK(stage_secrets(ctx, key_lv0, key_lv1, rk, s));
  const uint32_t *d_k0 = s.d_k0;
  const double2 *d_spec = s.d_spec;
  const ChaChaKey *d_rk = s.d_rk;
  ChaChaKey seed;
  CHK(derive_public_seed<kStreamSeededSeed>(ctx, s, seed));
  // bodies: public, in ctx->out
  CHK(ensure(ctx, ctx->out.dev, (bsk_words + ksk_words) * 4));
  uint32_t *d_bb = (uint32_t *)ctx->out.dev.p, *d_kb = d_bb + bsk_words;
  const auto gen_bsk = kernel_inst(ctx, false, [](auto inst) { return k_gen_compressed_bsk<decltype(inst)::L>; });
  hipLaunchKernelGGL(gen_bsk, dim3((unsigned)(P.n * 2 * P.l)), dim3(64), kStageLdsBytes, ctx->stream, d_k0, d_spec, ctx->d_tw,
                     d_bb, P.bgbit, alpha_bsk, d_rk, seed);
  HIPCHK(ctx, hipGetLastError());
  CHK(ksk_rows_launch(ctx, s, &seed, alpha_ksk, d_kb, nullptr));
  HIPCHK(ctx, hipMemcpyAsync(bsk_bodies, d_bb, bsk_words * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ksk_bodies, d_kb, ksk_words * 4, hipMemcpyDeviceToHost, ctx->stream));
  // the context's key is what tfhe_hip_load_compressed_cloud_key rebuilds from these bodies, bit for bit
  HIPCHK(ctx, expand_key_locked(ctx, seed, d_bb, d_kb));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  CHK(default_offset_and_testvec(ctx, decomp_offset));
  memcpy(mask_seed, seed.k, 32);
  return commit_cloud_key(ctx, *decomp_offset);
}
}  // namespace

int tfhe_hip_gen_compressed_cloud_key(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1,
                                      double alpha_ksk, double alpha_bsk, const uint8_t rng_key[32],
                                      uint8_t mask_seed[32], uint32_t *bsk_bodies, uint32_t *ksk_bodies,
                                      uint32_t *decomp_offset) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (!key_lv0 || !key_lv1 || !mask_seed || !bsk_bodies || !ksk_bodies || !decomp_offset)
    return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  if (!(alpha_ksk >= 0.0) || !(alpha_bsk >= 0.0)) return fail(ctx, TFHE_HIP_EINVAL, "negative noise parameter");
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  return gen_compressed_locked(ctx, key_lv0, key_lv1, alpha_ksk, alpha_bsk, gk.k, mask_seed, bsk_bodies, ksk_bodies,
                               decomp_offset);
}

int tfhe_hip_load_compressed_cloud_key(tfhe_hip_ctx *ctx, const uint8_t mask_seed[32], const uint32_t *bsk_bodies,
                                       const uint32_t *ksk_bodies, uint32_t decomp_offset, const uint32_t *testvec) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (!mask_seed || !bsk_bodies || !ksk_bodies || !testvec) return fail(ctx, TFHE_HIP_EINVAL, "null key pointer");
  CHK(begin_key_change(ctx, KEY_BUF_ALL));
  const tfhe_hip_params &P = ctx->P;
  const size_t bsk_words = (size_t)P.n * 2 * P.l * kN, ksk_words = ksk_rows(P);
  // the bodies travel (17 MB instead of 172 on SECURITY_128_BIT); the masks are regenerated on the device
  CHK(upload_through_temp(ctx, "key bodies", {{bsk_bodies, bsk_words * 4}, {ksk_bodies, ksk_words * 4}}, 0, [&](void *d_bodies) {
    return expand_key_locked(ctx, seed_key(mask_seed), (const uint32_t *)d_bodies, (const uint32_t *)d_bodies + bsk_words);
  }));
  HIPCHK(ctx, hipMemcpyAsync(ctx->K->d_testvec, testvec, key_testvec_bytes(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return commit_cloud_key(ctx, decomp_offset);
}

namespace {
int expand_seeded_launch(tfhe_hip_ctx *ctx, const ChaChaKey &seed, uint64_t first_index, const uint32_t *bodies, size_t count,
                         uint32_t *out, hipStream_t s) {
  LweRowJob j{};
  j.seed = seed;
  j.dom_mask = kSeedDomainTlwe;
  j.first_index = first_index;
  j.rows = count;
  j.plain = bodies;
  j.out = out;
  j.stride = ctx->P.n + 1;
  return lwe_rows_launch(ctx, j, s);
}
}  // namespace

int tfhe_hip_expand_seeded_tlwe(tfhe_hip_ctx *ctx, const uint8_t mask_seed[32], uint64_t first_index,
                                const uint32_t *bodies, size_t count, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (!mask_seed) return fail(ctx, TFHE_HIP_EINVAL, "null mask seed");
  if (count == 0) return TFHE_HIP_OK;
  if (!bodies || !out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  const ChaChaKey seed = seed_key(mask_seed);
  return host_call(ctx, false, {{bodies, count * 4, &ctx->a}}, out, count * (size_t)(ctx->P.n + 1) * 4,
                   [&](const void *const *d, void *o) {
                     return expand_seeded_launch(ctx, seed, first_index, u32(d[0]), count, (uint32_t *)o, ctx->stream);
                   });
}

int tfhe_hip_expand_seeded_tlwe_dev(tfhe_hip_ctx *ctx, const uint8_t mask_seed[32], uint64_t first_index,
                                    const uint32_t *bodies, size_t count, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (!mask_seed) return fail(ctx, TFHE_HIP_EINVAL, "null mask seed");
  if (count && (!bodies || !out)) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  if (count == 0) return TFHE_HIP_OK;
  return expand_seeded_launch(ctx, seed_key(mask_seed), first_index, bodies, count, out, pick(ctx, stream));
}
