// cmux.hpp -- packed CMUX: the external product TRGSW (.) TRLWE with a selector the caller holds, and the CMUX on it.
//
// The format and the result are normative in include/tfhe_hip.h ("packed CMUX").  With x = d1 - d0 (or d1 alone) and
// sel the TRGSW [2t][2][N] of the caller,
//
//   out[m][c] = d0[m][c] + sum_{i<t} D_i(x[m].a) (*) sel[i][c] + sum_{i<t} D_i(x[m].b) (*) sel[t+i][c]
//
// is trgsw::cmux of the reference with the gadget (beta, t) of the call.  Like the TRLWE key switch
// (trlwe_switch.hpp) it is the plaintext polynomial product of matmul.hpp with the roles swapped: the digit polynomials
// are the int8 "weights" (rows = the ciphertexts of a chunk, cols = 2t) and the selector's 2t rows, shared by the whole
// batch, are the one group of "ciphertexts".  cmux_dev calls polymul_dev as it stands, so the result is exact in
// integers and the GEMM is not forked.  What this file adds:
//   k_cmux_digits     one wave (one workgroup) per ciphertext: the difference of the two inputs in registers and the
//                     signed digits of both halves as int8 planes [chunk][2t][N] -- plane i the digits d_i of the a
//                     half, plane t + i those of the b half, the selector's row order.  Not negated, no permutation.
//   k_cmux_addend     out += d0 behind the GEMM, in 16-byte accesses, as k_polymul_bias is for the b half.
//   k_encrypt_trgsw   one wave per row of a selector, from the row pieces of k_trlwe_rows: natural_mask under S,
//                     row_noise under K, add_ring_product against the spectrum of s1, then the gadget polynomial
//                     g_i mu(X) on the a half (rows below t) or the b half, store.
//
// Loads, LDS and stores of k_cmux_digits.  The pass reads 8 or 16 KiB a ciphertext and writes 2t KiB, so the loads
// decide.  Lane q loads 16-byte slot q + 64 r of a row (r < 4): every load instruction of the wave is one contiguous
// KiB, the widest coalesced form (a dword load would cover a quarter of that per instruction and take four times the
// instructions).  The difference is formed on those registers.  For a 16-byte store per plane lane q needs the sixteen
// coefficients 16 q .. 16 q + 15, which are slots 4 q .. 4 q + 3: the regrouping goes through LDS, as in
// k_trlwe_switch_digits -- the alternative without LDS, each lane keeping its four coefficients of every quarter and
// storing a dword per plane and quarter, writes the same bytes in four times the store instructions.  Two images of N
// words (x.a, x.b), 8 KiB: written linearly (slot q + 64 r by lane q: conflict-free), read back in the rotated slot
// order (r + (q >> 2)) & 3 that keeps the sixteen lanes of a ds_read_b128 group on different 16-byte slots of a bank
// row (see trlwe_switch.hpp), and put back in order by two select stages in registers.
#pragma once
#include "internal.hpp"
#include "trlwe_encrypt.hpp"  // aligned16
#include "trlwe_switch.hpp"   // kTsChunk, kTsMaxBasebit, kTsMaxBits: the switch's box of shapes

namespace tfhe {

constexpr size_t kCmuxChunk = kTsChunk;  // ciphertexts a pass: kCmuxChunk 2t N bytes of scratch, 12 MiB at t = 3
constexpr int kCmuxAddendThreads = 256;

// One wave per ciphertext of the chunk.  d0 (or NULL), d1: [chunk][2][N]; dig: [chunk][2t][N] int8, plane c t + i =
// d_i of half c of d1 - d0.  1 <= basebit <= 7, 1 <= t <= 32, basebit t <= 32.  rnd: 2^(31 - basebit t), or 0 (the
// reference's truncating decomposition, and basebit t = 32).
__global__ __launch_bounds__(64) void k_cmux_digits(const uint32_t *__restrict__ d0, const uint32_t *__restrict__ d1,
                                                     int basebit, int t, uint32_t rnd, int8_t *__restrict__ dig) {
  static_assert(kN == 16 * 64, "one wave per ciphertext, sixteen coefficients a lane");
  __shared__ __attribute__((aligned(16))) uint32_t sx[2][kN];
  const int lane = threadIdx.x;
  const size_t ct = blockIdx.x;
  const uint4 *p1 = reinterpret_cast<const uint4 *>(d1 + ct * 2 * kN);
  const uint4 *p0 = d0 ? reinterpret_cast<const uint4 *>(d0 + ct * 2 * kN) : nullptr;
#pragma unroll
  for (int r = 0; r < 8; ++r) {  // slots 0 .. 255 are the a half, 256 .. 511 the b half
    uint4 x = p1[lane + 64 * r];
    if (p0) {  // (wave-uniform)
      const uint4 y = p0[lane + 64 * r];
      x.x -= y.x, x.y -= y.y, x.z -= y.z, x.w -= y.w;
    }
    reinterpret_cast<uint4 *>(&sx[0][0])[lane + 64 * r] = x;
  }
  __syncthreads();
  const int bt = basebit * t;
  const uint32_t half = 1u << (basebit - 1), bmask = (1u << basebit) - 1u;
  const uint32_t btmask = bt < 32 ? (1u << bt) - 1u : 0xFFFFFFFFu;
  uint32_t off = 0;
  for (int q = 0; q < t; ++q) off += half << (basebit * q);
  // d_i = u_i - B/2 on four bytes at once: u < 128 and B/2 <= 64, so u + 128 - B/2 stays inside its byte, and ^ 0x80
  // makes it the i8 (from -B/2, -64 at beta = 7, to B/2 - 1)
  const uint32_t bias = (128u - half) * 0x01010101u;
  const int rot = (lane >> 2) & 3;
#pragma unroll 1
  for (int c = 0; c < 2; ++c) {
    // the lane's four slots in rotated order, then back in order (trlwe_switch.hpp)
    uint4 v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = reinterpret_cast<const uint4 *>(sx[c])[4 * lane + ((r + rot) & 3)];
    if (rot & 1) {
      const uint4 x = v[3];
      v[3] = v[2], v[2] = v[1], v[1] = v[0], v[0] = x;
    }
    if (rot & 2) {
      const uint4 x = v[0], y = v[1];
      v[0] = v[2], v[1] = v[3], v[2] = x, v[3] = y;
    }
    // (w + off g + rnd) >> (32 - bt): its plain base-B digits are the u_i (off has no bits below 2^(32 - bt))
    const uint32_t rnd_c = TFHE_MUT(kMut_cmux_rnd_b) ? (c == 1 ? 0u : rnd) : rnd;  // (the b half truncates)
    uint32_t ap[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t w[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) ap[4 * q + e] = (((w[e] + rnd_c) >> (32 - bt)) + off) & btmask;
    }
    uint4 *dst = reinterpret_cast<uint4 *>(dig + (ct * 2 + (size_t)c) * (size_t)t * kN) + lane;
#pragma unroll 1
    for (int i = 0; i < t; ++i) {
      const int sh = basebit * (t - 1 - i);
      uint32_t o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t u = ((ap[4 * q] >> sh) & bmask) | (((ap[4 * q + 1] >> sh) & bmask) << 8) |
                           (((ap[4 * q + 2] >> sh) & bmask) << 16) | (((ap[4 * q + 3] >> sh) & bmask) << 24);
        o[q] = (u + bias) ^ 0x80808080u;
      }
      dst[(size_t)i * (kN / 16)] = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
}

// out[m][c][i] += d0[m][c][i]: `quads` 16-byte pieces of both, one a thread
__global__ __launch_bounds__(kCmuxAddendThreads) void k_cmux_addend(const uint4 *__restrict__ d0, size_t quads,
                                                                     uint4 *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kCmuxAddendThreads + threadIdx.x;
  if (i >= quads) return;
  const uint4 a = d0[i];
  uint4 v = out[i];
  v.x += a.x, v.y += a.y, v.z += a.z, v.w += TFHE_MUT(kMut_cmux_addend_w) ? 0u : a.w;
  out[i] = v;
}

// One wave per row: blockIdx.x = m 2t + row.  mu: [count][N] int32; out: [count][2t][2][N].
__global__ __launch_bounds__(64) void k_encrypt_trgsw(const double2 *__restrict__ s1_spec, const double2 *__restrict__ twt,
                                                       const ChaChaKey *__restrict__ key_p, ChaChaKey seed,
                                                       uint64_t first_index, const int32_t *__restrict__ mu, int basebit,
                                                       int t, double alpha, uint32_t *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double2 *tile = reinterpret_cast<double2 *>(smem);
  const int lane = threadIdx.x;
  const size_t r = blockIdx.x;
  const int row = (int)(r % (size_t)(2 * t));
  const uint64_t g = first_index + (uint64_t)r;
  const uint32_t g_lo = (uint32_t)g, g_hi = TFHE_MUT(kMut_trgsw_index_hi) ? 0u : (uint32_t)(g >> 32);
  Twiddles tw;
  tw.load(twt, reinterpret_cast<double2 *>(smem + kTileBytes), lane);
  uint32_t *dst_a = out + r * (size_t)(2 * kN);
  uint32_t a_lo[8], a_hi[8], b_lo[8], b_hi[8];
  natural_mask<false>(seed, g_lo, g_hi, kSeedDomainTrgswMask, reinterpret_cast<uint32_t *>(smem), lane, nullptr, a_lo, a_hi);
  row_noise(*key_p, g_lo, g_hi, kSeedDomainTrgswNoise, alpha, lane, b_lo, b_hi);
  double are[8], aim[8];
  add_ring_product(a_lo, a_hi, s1_spec, tw, tile, lane, are, aim, b_lo, b_hi);
  // the gadget polynomial g_i mu(X), after the body is formed, wrapping: on the a half for rows below t, else on b
  const uint32_t gd = 1u << (32 - (row % t + 1) * basebit);
  const int32_t *mp = mu + (r / (size_t)(2 * t)) * (size_t)kN;
  const bool on_a = TFHE_MUT(kMut_trgsw_row_t) ? row <= t : row < t;  // (wave-uniform)
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const uint32_t lo = gd * (uint32_t)mp[lane + 64 * m], hi = gd * (uint32_t)mp[lane + 64 * m + kN2];
    if (on_a) a_lo[m] += lo, a_hi[m] += hi;
    else b_lo[m] += lo, b_hi[m] += hi;
  }
  store_row(dst_a, lane, a_lo, a_hi);
  store_row(dst_a + kN, lane, b_lo, b_hi);
}

}  // namespace tfhe

// ---- packed CMUX (cmux.hpp) -------------------------------------------------------------------------------------------
namespace {
constexpr int kCmuxKnownFlags = TFHE_HIP_CMUX_REFERENCE_DIGITS;

const char *cmux_shape_refusal(int basebit, int t) {
  if (basebit < 1 || basebit > kTsMaxBasebit) return "basebit out of range (1 .. 7: digits in one byte)";
  if (t < 1 || (size_t)(2 * (long long)t) > kPolymulMaxCols) return "t out of range (1 .. 32: 2t columns)";
  if (basebit * t > kTsMaxBits) return "basebit * t exceeds 32";
  return nullptr;
}

// d0 (or NULL), d1 [count][2][N] -> out [count][2][N] on stream s, kCmuxChunk ciphertexts a pass through the scratch
int cmux_dev(tfhe_hip_ctx *ctx, const uint32_t *sel, int basebit, int t, int flags, const uint32_t *d0, const uint32_t *d1,
             size_t count, uint32_t *out, hipStream_t s) {
  const size_t chunk = count < kCmuxChunk ? count : kCmuxChunk;
  const int bt = basebit * t;
  const uint32_t rnd = (flags & TFHE_HIP_CMUX_REFERENCE_DIGITS) || bt >= 32 ? 0u : 1u << (31 - bt);
  CHK(take(ctx, s, ctx->cm_dig, chunk * (size_t)(2 * t) * kN));
  int8_t *d_dig = (int8_t *)ctx->cm_dig.p;
  for (size_t c0 = 0; c0 < count; c0 += chunk) {
    const size_t n = count - c0 < chunk ? count - c0 : chunk;
    const uint32_t *p0 = d0 ? d0 + c0 * 2 * kN : nullptr;
    uint32_t *po = out + c0 * 2 * kN;
    {
      TimedScope timed(ctx->ev_cm_dig, s, ctx->profiling);  // (while profiling is on: tfhe_hip_get_cmux_times)
      CHK(hip_rc(ctx, timed.err));
      hipLaunchKernelGGL(k_cmux_digits, dim3((unsigned)n), dim3(64), 0, s, p0, d1 + c0 * 2 * kN, basebit, t, rnd, d_dig);
      CHK(launched(ctx));  // (the pair is closed whichever way the launch ended)
      CHK(hip_rc(ctx, timed.close()));
    }
    {
      TimedScope timed(ctx->ev_cm_mm, s, ctx->profiling);
      CHK(hip_rc(ctx, timed.err));
      CHK(polymul_dev(ctx, d_dig, nullptr, n, (size_t)(2 * t), sel, 1, po, s));
      CHK(hip_rc(ctx, timed.close()));
    }
    if (!p0) continue;
    TimedScope timed(ctx->ev_cm_add, s, ctx->profiling);
    CHK(hip_rc(ctx, timed.err));
    const size_t quads = n * (size_t)(2 * kN / 4);  // <= 2^20
    hipLaunchKernelGGL(k_cmux_addend, dim3((unsigned)((quads + kCmuxAddendThreads - 1) / kCmuxAddendThreads)),
                       dim3(kCmuxAddendThreads), 0, s, reinterpret_cast<const uint4 *>(p0), quads, reinterpret_cast<uint4 *>(po));
    CHK(launched(ctx));
    CHK(hip_rc(ctx, timed.close()));
  }
  return TFHE_HIP_OK;
}

// the checks both forms share (returns TFHE_HIP_OK with *run false for an empty batch)
int cmux_checks(tfhe_hip_ctx *ctx, const uint32_t *sel, int basebit, int t, int flags, const uint32_t *d1, size_t count,
                const uint32_t *out, bool *run) {
  *run = false;
  if (const char *why = cmux_shape_refusal(basebit, t)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (flags & ~kCmuxKnownFlags) return fail(ctx, TFHE_HIP_EINVAL, "unknown flag bit");
  if (count == 0) return TFHE_HIP_OK;
  if (!sel || !d1 || !out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  if (count > 0x7FFFFFFFull) return fail(ctx, TFHE_HIP_EINVAL, "count too large");
  *run = true;
  return TFHE_HIP_OK;
}

const char *trgsw_enc_refusal(const uint32_t *key_lv1, const int32_t *mu, size_t count, int basebit, int t, double alpha,
                              uint64_t first_index, const uint32_t *out) {
  if (const char *why = cmux_shape_refusal(basebit, t)) return why;
  if (!key_lv1) return "null pointer";
  if (count && (!mu || !out)) return "null pointer";
  if (!(alpha >= 0.0)) return "negative noise parameter";
  if (count > 0x7FFFFFFFull / (size_t)(2 * t)) return "count too large";
  if (count && first_index + (uint64_t)(count * (size_t)(2 * t) - 1) < first_index) return "the row indices run past 2^64";
  for (int x = 0; x < kN; ++x)
    if (key_lv1[x] > 1u) return "secret keys are binary";
  return nullptr;
}

// ctx->mu held: the secrets staged (and wiped on every path), S derived, the rows made on the context's stream, which
// is drained before this returns.  mu / out are device pointers.
int encrypt_trgsw_locked(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const int32_t *d_mu, size_t count, int basebit, int t,
                         double alpha, const ChaChaKey &rk, uint64_t first_index, uint8_t *mask_seed_out, uint32_t *d_out) {
  StagedSecrets s(ctx, (size_t)0);  // (no level-0 key: K, the seed slot, s1 and its spectrum)
  CHK(stage_secrets(ctx, key_lv1, key_lv1, rk, s));
  ChaChaKey seed;
  CHK(derive_public_seed<kStreamTrgswSeed>(ctx, s, seed));
  hipLaunchKernelGGL(k_encrypt_trgsw, dim3((unsigned)(count * (size_t)(2 * t))), dim3(64), kStageLdsBytes, ctx->stream, s.d_spec,
                     ctx->d_tw, (const ChaChaKey *)s.d_rk, seed, first_index, d_mu, basebit, t, alpha, d_out);
  CHK(launched(ctx));
  if (mask_seed_out) memcpy(mask_seed_out, seed.k, 32);
  return TFHE_HIP_OK;
}
}  // namespace

int tfhe_hip_batch_trlwe_cmux(tfhe_hip_ctx *ctx, const uint32_t *sel, int basebit, int t, int flags, const uint32_t *d0,
                              const uint32_t *d1, size_t count, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  bool run = false;
  CHK(cmux_checks(ctx, sel, basebit, t, flags, d1, count, out, &run));
  if (!run) return TFHE_HIP_OK;
  return host_call(ctx, false, {{sel, trlwe_bytes((size_t)(2 * t)), &ctx->a}, {d0, trlwe_bytes(count), &ctx->b}, {d1, trlwe_bytes(count), &ctx->c}},
                   out, trlwe_bytes(count), [&](const void *const *d, void *o) {
                     return cmux_dev(ctx, u32(d[0]), basebit, t, flags, u32(d[1]), u32(d[2]), count, (uint32_t *)o, ctx->stream);
                   });
}

int tfhe_hip_batch_trlwe_cmux_dev(tfhe_hip_ctx *ctx, const uint32_t *sel, int basebit, int t, int flags, const uint32_t *d0,
                                  const uint32_t *d1, size_t count, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  bool run = false;
  CHK(cmux_checks(ctx, sel, basebit, t, flags, d1, count, out, &run));
  if (!run) return TFHE_HIP_OK;
  if (!aligned16(d0) || !aligned16(d1) || !aligned16(out)) return fail(ctx, TFHE_HIP_EINVAL, "d0, d1 and out must be 16-byte aligned");
  return cmux_dev(ctx, sel, basebit, t, flags, d0, d1, count, out, pick(ctx, stream));
}

int tfhe_hip_batch_encrypt_trgsw(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const int32_t *mu, size_t count, int basebit, int t,
                                 double alpha, const uint8_t rng_key[32], uint64_t first_index, uint8_t mask_seed_out[32],
                                 uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (const char *why = trgsw_enc_refusal(key_lv1, mu, count, basebit, t, alpha, first_index, out)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  const size_t mu_bytes = count * (size_t)kN * 4;
  const int rc = host_call(ctx, false, {{mu, mu_bytes, &ctx->a}}, out, trlwe_bytes(count * (size_t)(2 * t)), [&](const void *const *d, void *o) {
    return encrypt_trgsw_locked(ctx, key_lv1, (const int32_t *)d[0], count, basebit, t, alpha, gk.k, first_index, mask_seed_out, (uint32_t *)o);
  });
  scrub(ctx->stream, {{&ctx->a, mu_bytes}});  // the selector's message does not stay behind in the staging buffer
  return rc;
}

int tfhe_hip_batch_encrypt_trgsw_dev(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const int32_t *mu, size_t count, int basebit,
                                     int t, double alpha, const uint8_t rng_key[32], uint64_t first_index,
                                     uint8_t mask_seed_out[32], uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (const char *why = trgsw_enc_refusal(key_lv1, mu, count, basebit, t, alpha, first_index, out)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  return encrypt_trgsw_locked(ctx, key_lv1, mu, count, basebit, t, alpha, gk.k, first_index, mask_seed_out, out);
}

int tfhe_hip_get_cmux_times(tfhe_hip_ctx *ctx, tfhe_hip_cmux_times *out) {
  if (!ctx || !out) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  memset(out, 0, sizeof(*out));
  CHK(hip_rc(ctx, ctx->ev_cm_dig.drain(out->digits_ms, &out->passes)));
  CHK(hip_rc(ctx, ctx->ev_cm_mm.drain(out->contraction_ms)));
  return hip_rc(ctx, ctx->ev_cm_add.drain(out->addend_ms));
}
