// packing_keygen.hpp -- the packing key generated on the GPU, behind the C ABI.
//
// The key is the one tfhe_hip_load_packing_key defines (include/tfhe_hip.h, "packing key switch"): row r = i t + l is
// (a_r, b_r = a_r (*) s1 + e_r + s0[i] g_l X^0), a_r the keystream (r, 24, "PKS") under the public mask seed S.  What
// this header adds is where S and e_r come from under a 32-byte generator key K (normative in the header):
//   S    words 0..7 of block(K, 0, nonce (0, 26, "DES")) -- stream 26, not the compressed cloud key's 20;
//   e_r  Box-Muller over the keystream (r, 25, "PKS") under K, in the BSK generators' word order.
// The product a_r (*) s1 runs through the FFT of k_gen_compressed_bsk and is exact (|coefficients| < 2^41).  The rows
// land in the temporary [n t][2][N] that k_pack_expand_key would fill, so k_pack_planes builds the same byte planes
// and the handle holds, bit for bit, the key tfhe_hip_load_packing_key(S, bodies) would build.
#pragma once
#include "packing.hpp"

namespace tfhe {

// One wave per row r = i t + l.  rows: [n t][2][N] (a half, b half), bodies: [n t][N].
__global__ __launch_bounds__(64) void k_gen_packing_key(const uint32_t *__restrict__ key_lv0,
                                                         const double2 *__restrict__ s1_spec,
                                                         const double2 *__restrict__ twt, uint32_t *__restrict__ rows,
                                                         uint32_t *__restrict__ bodies, int basebit, int t, double alpha,
                                                         const ChaChaKey *__restrict__ key_p, ChaChaKey seed) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double2 *tile = reinterpret_cast<double2 *>(smem);
  const int lane = threadIdx.x;
  const uint32_t row = blockIdx.x;
  const int l = (int)(row % (uint32_t)t), i = (int)(row / (uint32_t)t);
  Twiddles tw;
  tw.load(twt, reinterpret_cast<double2 *>(smem + kTileBytes), lane);
  uint32_t *dst_a = rows + (size_t)row * 2 * kN;
  uint32_t a_lo[8], a_hi[8], b_lo[8], b_hi[8];
  natural_mask<true>(seed, row, kStreamPackMask, kSeedDomainPack, reinterpret_cast<uint32_t *>(smem), lane, dst_a, a_lo, a_hi);
  row_noise(*key_p, row, kStreamPackNoise, kSeedDomainPack, alpha, lane, b_lo, b_hi);
  double are[8], aim[8];
  add_ring_product(a_lo, a_hi, s1_spec, tw, tile, lane, are, aim, b_lo, b_hi);
  // the gadget s0[i] g_l on coefficient 0, after the product, wrapping
  if (lane == 0) b_lo[0] += key_lv0[i] * (1u << (32 - (l + 1) * basebit));
  store_row(dst_a + kN, lane, b_lo, b_hi);
  store_row(bodies + (size_t)row * kN, lane, b_lo, b_hi);
}

}  // namespace tfhe

// ---- packing key generation (packing_keygen.hpp) ---------------------------------------------------------------
namespace {
// ctx->mu held, ctx's device current, arguments validated
int gen_packing_key_locked(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha,
                           const ChaChaKey &rk, uint8_t mask_seed[32], uint32_t *bodies) {
  const tfhe_hip_params &P = ctx->P;
  KeyState &k = *ctx->K;
  CHK(begin_side_key(ctx, k.pk_loaded, k.d_pk8, pk_plane_bytes(P.n, P.t)));
  StagedSecrets s(ctx);  // (wiped on every exit path)
  CHK(stage_secrets(ctx, key_lv0, key_lv1, rk, s));
  const uint32_t *d_k0 = s.d_k0;
  const double2 *d_spec = s.d_spec;
  const ChaChaKey *d_rk = s.d_rk;
  ChaChaKey seed;
  CHK(derive_public_seed<kStreamPackSeed>(ctx, s, seed));
  const size_t rows = (size_t)P.n * P.t, body_words = rows * kN;
  const size_t chunks = pk_plane_bytes(P.n, P.t) / 16;
  // the temporary: the rows [n t][2][N], then the bodies [n t][N]; drained and freed on every path
  CHK(upload_through_temp(ctx, "packing key generation", {}, (rows * 2 * kN + body_words) * 4, [&](void *tmp) {
    uint32_t *d_rows = (uint32_t *)tmp, *d_bodies = d_rows + rows * 2 * kN;
    hipLaunchKernelGGL(k_gen_packing_key, dim3((unsigned)rows), dim3(64), kStageLdsBytes, ctx->stream, d_k0, d_spec,
                       ctx->d_tw, d_rows, d_bodies, P.basebit, P.t, alpha, d_rk, seed);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_pack_planes<256>, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, ctx->stream, d_rows,
                       k.d_pk8, P.n, P.t, chunks);
    if (const hipError_t e = hipGetLastError()) return e;
    if (bodies) return hipMemcpyAsync(bodies, d_bodies, body_words * 4, hipMemcpyDeviceToHost, ctx->stream);
    return hipSuccess;
  }));
  memcpy(mask_seed, seed.k, 32);
  commit_side_key(k.pk_loaded);
  return TFHE_HIP_OK;
}
}  // namespace

int tfhe_hip_gen_packing_key(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha,
                             const uint8_t rng_key[32], uint8_t mask_seed[32], uint32_t *bodies) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  // validation first: a refused call leaves the old packing key answering
  if (!key_lv0 || !key_lv1 || !mask_seed) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  if (!packing_supported(&ctx->P)) return fail(ctx, TFHE_HIP_EINVAL, kPackingRefusal);
  if (!(alpha >= 0.0)) return fail(ctx, TFHE_HIP_EINVAL, "negative noise parameter");
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  return gen_packing_key_locked(ctx, key_lv0, key_lv1, alpha, gk.k, mask_seed, bodies);
}
