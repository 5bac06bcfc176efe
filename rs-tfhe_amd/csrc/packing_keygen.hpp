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
//
// Every kernel here is a template: instantiations are emitted after the library's other kernels, so the code of every
// existing kernel stays byte-identical.
#pragma once
#include "packing.hpp"

namespace tfhe {

constexpr uint32_t kPackMaskStream = 24u;   // masks, under S (k_pack_expand_key)
constexpr uint32_t kPackNoiseStream = 25u;  // noise, under K
constexpr uint32_t kPackSeedStream = 26u;   // S from K, domain "DES"

// seed = words 0..7 of block 0 of the generator key's stream (0, STREAM, "DES")
template <int WG, uint32_t STREAM>
__global__ __launch_bounds__(WG) void k_derive_stream_seed(const ChaChaKey *__restrict__ key_p, ChaChaKey *__restrict__ seed) {
  if (threadIdx.x != 0) return;
  uint32_t w[16];
  chacha20_block(*key_p, 0u, 0u, STREAM, kSeedDomainSeed, w);
#pragma unroll
  for (int c = 0; c < 8; ++c) seed->k[c] = w[c];
}

// Mask polynomial of packing-key row `row`: lane q makes block q (coefficients 16q..16q+15) of (row, 24, "PKS"), writes
// it to `a_out` in natural order (the words k_pack_expand_key writes) and, through the LDS, hands lane l the
// coefficients l+64m and l+64m+512 the FFT wants.  One wave per workgroup; the tile is the transforms' afterwards.
__device__ __forceinline__ void pack_key_mask(const ChaChaKey &seed, uint32_t row, uint32_t *s, int lane,
                                              uint32_t *__restrict__ a_out, uint32_t (&a_lo)[8], uint32_t (&a_hi)[8]) {
  uint32_t w[16];
  chacha20_block(seed, (uint32_t)lane, row, kPackMaskStream, kSeedDomainPack, w);
  uint4 *s4 = reinterpret_cast<uint4 *>(s) + lane * 4;
  uint4 *g4 = reinterpret_cast<uint4 *>(a_out) + lane * 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint4 v = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    s4[q] = v;
    g4[q] = v;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    a_lo[m] = s[lane + 64 * m];
    a_hi[m] = s[lane + 64 * m + kN2];
  }
  __syncthreads();
}

// One wave per row r = i t + l.  rows: [n t][2][N] (a half, b half), bodies: [n t][N].
template <int WG>
__global__ __launch_bounds__(WG) void k_gen_packing_key(const uint32_t *__restrict__ key_lv0,
                                                         const double2 *__restrict__ s1_spec,
                                                         const double2 *__restrict__ twt, uint32_t *__restrict__ rows,
                                                         uint32_t *__restrict__ bodies, int basebit, int t, double alpha,
                                                         const ChaChaKey *__restrict__ key_p, ChaChaKey seed) {
  static_assert(WG == 64, "one wave per row");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double2 *tile = reinterpret_cast<double2 *>(smem);
  const int lane = threadIdx.x;
  const uint32_t row = blockIdx.x;
  const int l = (int)(row % (uint32_t)t), i = (int)(row / (uint32_t)t);
  Twiddles tw;
  tw.load(twt, reinterpret_cast<double2 *>(smem + kTileBytes), lane);
  uint32_t *dst_a = rows + (size_t)row * 2 * kN;
  uint32_t a_lo[8], a_hi[8], b_lo[8], b_hi[8];
  pack_key_mask(seed, row, reinterpret_cast<uint32_t *>(smem), lane, dst_a, a_lo, a_hi);
  const ChaChaKey key = *key_p;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    uint32_t w[16];
    chacha20_block(key, (uint32_t)(lane * 2 + h), row, kPackNoiseStream, kSeedDomainPack, w);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      double g0, g1;
      gauss2(w + 4 * m, alpha, g0, g1);
      b_lo[4 * h + m] = dev_f64_to_torus(g0);
      b_hi[4 * h + m] = dev_f64_to_torus(g1);
    }
  }
  double re[8], im[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    re[m] = (double)(int32_t)a_lo[m];
    im[m] = (double)(int32_t)a_hi[m];
  }
  fft_forward(re, im, tw, tile, lane);
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const double2 sp = s1_spec[s * 64 + lane];
    const double pr = (re[s] * sp.x - im[s] * sp.y) * 0x1p-9;
    const double pi = (re[s] * sp.y + im[s] * sp.x) * 0x1p-9;
    re[s] = pr;
    im[s] = pi;
  }
  fft_inverse(re, im, tw, tile, lane);
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    b_lo[m] += round_to_torus<false>(re[m]);
    b_hi[m] += round_to_torus<false>(im[m]);
  }
  // the gadget s0[i] g_l on coefficient 0, after the product, wrapping
  if (lane == 0) b_lo[0] += key_lv0[i] * (1u << (32 - (l + 1) * basebit));
  uint32_t *dst_b = dst_a + kN, *dst_o = bodies + (size_t)row * kN;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    dst_b[lane + 64 * m] = b_lo[m];
    dst_b[lane + 64 * m + kN2] = b_hi[m];
    dst_o[lane + 64 * m] = b_lo[m];
    dst_o[lane + 64 * m + kN2] = b_hi[m];
  }
}

}  // namespace tfhe

// ---- packing key generation (packing_keygen.hpp) ---------------------------------------------------------------
namespace {
// ctx->mu held, ctx's device current, arguments validated
int gen_packing_key_locked(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha,
                           const ChaChaKey &rk, uint8_t mask_seed[32], uint32_t *bodies) {
  const tfhe_hip_params &P = ctx->P;
  // packing calls queued on the caller's streams may still read the planes this call overwrites
  HIPCHK(ctx, hipDeviceSynchronize());
  ctx->K->pk_loaded = false;
  if (!ctx->K->d_pk8) HIPCHK(ctx, hipMalloc((void **)&ctx->K->d_pk8, pk_plane_bytes(P.n, P.t)));
  // generator key at idx[0, 32), the mask seed derived from it at idx[32, 64)
  StagedSecrets s{{ctx}};  // (wiped on every exit path)
  CHK(stage_secrets(ctx, key_lv0, key_lv1, rk, 2 * sizeof(ChaChaKey), s));
  const uint32_t *d_k0 = s.d_k0;
  const double2 *d_spec = s.d_spec;
  const ChaChaKey *d_rk = s.d_rk;
  hipLaunchKernelGGL((k_derive_stream_seed<64, kPackSeedStream>), dim3(1), dim3(64), 0, ctx->stream, d_rk, s.d_rk + 1);
  HIPCHK(ctx, hipGetLastError());
  ChaChaKey seed;
  HIPCHK(ctx, hipMemcpyAsync(&seed, s.d_rk + 1, sizeof(seed), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t rows = (size_t)P.n * P.t, body_words = rows * kN;
  const size_t chunks = pk_plane_bytes(P.n, P.t) / 16;
  // the temporary: the rows [n t][2][N], then the bodies [n t][N]; drained and freed on every path
  CHK(upload_through_temp(ctx, "packing key generation", {}, (rows * 2 * kN + body_words) * 4, [&](void *tmp) {
    uint32_t *d_rows = (uint32_t *)tmp, *d_bodies = d_rows + rows * 2 * kN;
    hipLaunchKernelGGL(k_gen_packing_key<64>, dim3((unsigned)rows), dim3(64), kStageLdsBytes, ctx->stream, d_k0, d_spec,
                       ctx->d_tw, d_rows, d_bodies, P.basebit, P.t, alpha, d_rk, seed);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_pack_planes<256>, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, ctx->stream, d_rows,
                       ctx->K->d_pk8, P.n, P.t, chunks);
    if (const hipError_t e = hipGetLastError()) return e;
    if (bodies) return hipMemcpyAsync(bodies, d_bodies, body_words * 4, hipMemcpyDeviceToHost, ctx->stream);
    return hipSuccess;
  }));
  memcpy(mask_seed, seed.k, 32);
  ctx->K->pk_loaded = true;
  return TFHE_HIP_OK;
}
}  // namespace

int tfhe_hip_gen_packing_key(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha,
                             const uint8_t rng_key[32], uint8_t mask_seed[32], uint32_t *bodies) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  // validation first: a refused call leaves the old packing key answering
  if (!key_lv0 || !key_lv1 || !mask_seed) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  if (ctx->P.basebit > kPkMaxBasebit) return fail(ctx, TFHE_HIP_EINVAL, "packing needs basebit <= 7 (digits in one byte)");
  if (!(alpha >= 0.0)) return fail(ctx, TFHE_HIP_EINVAL, "negative noise parameter");
  ChaChaKey k;
  if (rng_key) {
    memcpy(k.k, rng_key, 32);
  } else if (const int err = os_random((uint8_t *)k.k, sizeof(k.k))) {
    return fail(ctx, TFHE_HIP_EHIP, os_random_text(err));
  }
  const int rc = gen_packing_key_locked(ctx, key_lv0, key_lv1, alpha, k, mask_seed, bodies);
  volatile uint32_t *wipe = k.k;
  for (int i = 0; i < 8; ++i) wipe[i] = 0;
  return rc;
}

// Generated on the first member; every other member loads the same (S, bodies).
int tfhe_hip_pool_gen_packing_key(tfhe_hip_pool *p, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha,
                                  const uint8_t rng_key[32], uint8_t mask_seed[32], uint32_t *bodies) {
  if (!p) return TFHE_HIP_EINVAL;
  std::lock_guard<FairMutex> plk(p->root()->own_mu);
  if (!mask_seed) return pool_fail(p, TFHE_HIP_EINVAL, "null pointer");
  tfhe_hip_ctx *first = p->ctxs[0];
  std::vector<uint32_t> own;  // the bodies the other members load when the caller keeps none
  if (!bodies && p->ctxs.size() > 1) {
    own.resize((size_t)first->P.n * first->P.t * kN);
    bodies = own.data();
  }
  CHK(pool_member_rc(p, first, tfhe_hip_gen_packing_key(first, key_lv0, key_lv1, alpha, rng_key, mask_seed, bodies)));
  for (size_t m = 1; m < p->ctxs.size(); ++m)
    CHK(pool_member_rc(p, p->ctxs[m], tfhe_hip_load_packing_key(p->ctxs[m], mask_seed, bodies)));
  return TFHE_HIP_OK;
}
