// trlwe_switch.hpp -- TRLWE key switch: a packed ciphertext under one ring key to psi_k of it under another.
//
// The format and the result are normative in include/tfhe_hip.h ("TRLWE key switch").  With psi_k the automorphism
// X -> X^k (k odd), a key whose row l encrypts g_l psi_k(s_from) under s_to takes ct = (a, b) under s_from to
//
//   out.a = - sum_l D_l (*) a_l,    out.b = psi_k(b) - sum_l D_l (*) b_l,    D_l = sum_j d_l(psi_k(a)[j]) X^j
//
// whose phase under s_to is psi_k(b - a (*) s_from) plus the rounding error and the key noise: k = 1 with two keys is
// packed proxy re-encryption, k != 1 with s_from = s_to = s1 a Galois key.  The contraction is the plaintext polynomial
// product of matmul.hpp with the roles swapped -- the negated digit polynomials are the int8 "weights" (rows = the
// ciphertexts of a chunk, cols = t), psi_k(b) is the bias polynomial and the key rows [t][2][N], shared by the whole
// batch, are the one group of "ciphertexts" -- so trlwe_switch_dev calls polymul_dev as it stands and the result is
// exact in integers.  What this file adds:
//   k_gen_trlwe_switch_key     one wave per row l, from the row pieces of the packing-key generator: natural_mask under
//                              S, row_noise under K, add_ring_product against the spectrum of s_to, then the gadget
//                              polynomial g_l psi_k(s_from) on every coefficient (the packing key's gadget sits on
//                              coefficient 0 alone), store_row.  Nonce row 64 k + l of streams 27 / 28, domain "TKS".
//   k_expand_trlwe_switch_key  the load path: the same natural_mask under S beside the uploaded bodies, so a handle
//                              that loaded (S, bodies) holds bit for bit the rows generation left on its handle.
//   k_trlwe_switch_digits      the new pass of the hot path, one wave (one workgroup) per ciphertext: psi_k of both
//                              rows through LDS, the rounding and signed decomposition of psi_k(a) (the packing key
//                              switch's, with this key's (beta, t)), the NEGATED digits as int8 planes [chunk][t][N]
//                              and psi_k(b) as [chunk][N] u32.
//
// LDS layout of k_trlwe_switch_digits.  Two natural-order images of N words (a', b'), 8 KiB.  Lane q reads words
// j = q + 64 m of the input rows (every global load instruction is one contiguous 256-byte segment) and writes word j,
// negated when bit 10 of j k is set, to position j k mod N: the 32 lanes of a half-wave -- the group that shares the 32
// banks of a ds_write_b32 -- hit positions k apart, and an odd k is a unit mod 32, so they hit 32 different banks: no
// conflict for ANY odd k.  k = N + 1 writes position j itself (the sign alternates with j) and k = 2N - 1 position
// N - j: stride +1 and -1, the same argument.  What a stride-k READ would cost is not paid: the reads are in output
// order.  b' is read back linearly (lane q, 16-byte slot q + 64 r) and stored as it is read.  For the digits lane q
// needs coefficients 16 q .. 16 q + 15, four slots 64 bytes from the next lane's: read in slot order the sixteen lanes
// of a ds_read_b128 group would meet on four 16-byte slots of the 256-byte bank row (4-way).  So lane q reads its
// slots in the rotated order (r + (q >> 2)) & 3: within every group of the instruction (each holds every residue of q
// mod 16 once) slot 4 (q & 3) + ((r + (q >> 2)) & 3) mod 16 is different for every lane -- conflict-free -- and two
// select stages in registers put the four slots back in order.  Both the digit planes and b' are written 16 bytes a
// lane, a wave's store of one plane (or one quarter of b') being one contiguous KiB; b' leaves as 16-byte store
// instructions, and so does the digit loop's remainder, but in its two-row unrolled body this compiler issues the same
// 16 bytes as four dword stores (the pass is 5 % of the switch: left as it is).
#pragma once
#include "internal.hpp"

namespace tfhe {

constexpr size_t kTsChunk = 2048;  // ciphertexts a pass: kTsChunk (t N + 4 N) bytes of scratch, 84 MB at t = 6
constexpr int kTsMaxBasebit = 7;   // the negated digits lie in (-B/2, B/2]: one signed byte
constexpr int kTsMaxBits = 32;     // beta t

// psi_k(p)[c] for a polynomial p of N words: coefficient j = c kinv mod 2N (kinv k = 1 mod 2N) lands on c, negated when
// it comes from the upper half (j >= N is coefficient j - N taken to position c + N).
__device__ __forceinline__ uint32_t ts_psi_at(const uint32_t *__restrict__ p, uint32_t c, uint32_t kinv) {
  const uint32_t j = (c * kinv) & (uint32_t)(2 * kN - 1);
  const uint32_t v = p[j & (uint32_t)(kN - 1)];
  return j & (uint32_t)kN ? 0u - v : v;
}

// One wave per row l < t.  rows: [t][2][N] (a half, b half), bodies: [t][N].
__global__ __launch_bounds__(64) void k_gen_trlwe_switch_key(const uint32_t *__restrict__ key_from,
                                                              const double2 *__restrict__ to_spec,
                                                              const double2 *__restrict__ twt, uint32_t *__restrict__ rows,
                                                              uint32_t *__restrict__ bodies, int k, uint32_t kinv,
                                                              int basebit, double alpha,
                                                              const ChaChaKey *__restrict__ key_p, ChaChaKey seed) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double2 *tile = reinterpret_cast<double2 *>(smem);
  const int lane = threadIdx.x;
  const int l = blockIdx.x;
  const uint32_t row = 64u * (uint32_t)k + (uint32_t)l;  // the nonce row: one K serves every k
  Twiddles tw;
  tw.load(twt, reinterpret_cast<double2 *>(smem + kTileBytes), lane);
  uint32_t *dst_a = rows + (size_t)l * 2 * kN;
  uint32_t a_lo[8], a_hi[8], b_lo[8], b_hi[8];
  natural_mask<true>(seed, row, kStreamTksMask, kSeedDomainTks, reinterpret_cast<uint32_t *>(smem), lane, dst_a, a_lo, a_hi);
  row_noise(*key_p, row, kStreamTksNoise, kSeedDomainTks, alpha, lane, b_lo, b_hi);
  double are[8], aim[8];
  add_ring_product(a_lo, a_hi, to_spec, tw, tile, lane, are, aim, b_lo, b_hi);
  // the gadget polynomial g_l psi_k(s_from), after the product, wrapping
  const uint32_t g = 1u << (32 - (l + 1) * basebit);
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    b_lo[m] += g * ts_psi_at(key_from, (uint32_t)(lane + 64 * m), kinv);
    b_hi[m] += g * ts_psi_at(key_from, (uint32_t)(lane + 64 * m + (TFHE_MUT(kMut_ts_gadget_hi) ? 0 : kN2)), kinv);  // (the low half's index: read above)
  }
  store_row(dst_a + kN, lane, b_lo, b_hi);
  store_row(bodies + (size_t)l * kN, lane, b_lo, b_hi);
}

// rows [t][2][N]: a_l regenerated from S (natural_mask, as generation made it), b_l from bodies [t][N].
// (WG stays a parameter: as a plain function the compiler orders this kernel's stores differently.)
template <int WG>
__global__ __launch_bounds__(WG) void k_expand_trlwe_switch_key(const uint32_t *__restrict__ bodies,
                                                                 uint32_t *__restrict__ rows, int k, ChaChaKey seed) {
  static_assert(WG == 64, "one wave per row");
  __shared__ __attribute__((aligned(16))) uint32_t s[kN];
  const int lane = threadIdx.x;
  const int l = blockIdx.x;
  uint32_t *dst_a = rows + (size_t)l * 2 * kN;
  uint32_t lo[8], hi[8];
  natural_mask<true>(seed, 64u * (uint32_t)k + (uint32_t)l, kStreamTksMask, kSeedDomainTks, s, lane, dst_a, lo, hi);
  load_row(bodies + (size_t)l * kN, lane, lo, hi);
  store_row(dst_a + kN, lane, lo, hi);
}

// One wave per ciphertext of the chunk.  in [chunk][2][N]; dig [chunk][t][N] int8 = -d_l(psi_k(a)[c]); bp [chunk][N]
// = psi_k(b).  1 <= basebit <= 7, 1 <= t, basebit t <= 32, k odd in [1, 2N).
__global__ __launch_bounds__(64) void k_trlwe_switch_digits(const uint32_t *__restrict__ in, int k, int basebit, int t,
                                                             int8_t *__restrict__ dig, uint32_t *__restrict__ bp) {
  static_assert(kN == 16 * 64, "one wave per ciphertext, sixteen coefficients a lane");
  __shared__ __attribute__((aligned(16))) uint32_t sa[kN];
  __shared__ __attribute__((aligned(16))) uint32_t sb[kN];
  const int lane = threadIdx.x;
  const size_t ct = blockIdx.x;
  const uint32_t *a = in + ct * 2 * kN, *b = a + kN;
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    const uint32_t j = (uint32_t)(lane + 64 * m);
    const uint32_t va = a[j], vb = b[j];
    const uint32_t p = (j * (uint32_t)k) & (uint32_t)(2 * kN - 1);
    const bool neg = (p & (uint32_t)kN) != 0;
    sa[p & (uint32_t)(kN - 1)] = neg ? 0u - va : va;
    sb[p & (uint32_t)(kN - 1)] = TFHE_MUT(kMut_ts_psi_sign_b) ? vb : (neg ? 0u - vb : vb);
  }
  __syncthreads();
  // b' as it lies
  uint4 *bp4 = reinterpret_cast<uint4 *>(bp + ct * kN);
#pragma unroll
  for (int r = 0; r < 4; ++r) bp4[lane + 64 * r] = reinterpret_cast<const uint4 *>(sb)[lane + 64 * r];
  // a': the lane's four slots in rotated order (see the file header), then back in order
  const int rot = (lane >> 2) & 3;
  uint4 v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = reinterpret_cast<const uint4 *>(sa)[4 * lane + ((r + rot) & 3)];
  // v[r] holds slot (r + rot) & 3: slot q is v[(q - rot) & 3]
  if (rot & 1) {
    const uint4 x = v[3];
    v[3] = v[2], v[2] = v[1], v[1] = v[0], v[0] = x;
  }
  if (TFHE_MUT(kMut_ts_rot3) ? rot == 2 : (rot & 2) != 0) {  // (registers change places, or do not)
    const uint4 x = v[0], y = v[1];
    v[0] = v[2], v[1] = v[3], v[2] = x, v[3] = y;
  }
  const int bt = basebit * t;
  const uint32_t half = 1u << (basebit - 1), bmask = (1u << basebit) - 1u;
  const uint32_t rnd = bt < 32 ? 1u << (31 - bt) : 0u, btmask = bt < 32 ? (1u << bt) - 1u : 0xFFFFFFFFu;
  uint32_t off = 0;
  for (int q = 0; q < t; ++q) off += half << (basebit * q);
  off = TFHE_MUT(kMut_ts_off_top) ? off - (half << (basebit * (t - 1))) : off;  // (the top digit's half left out)
  // (a_bar + off) mod 2^bt: its plain base-B digits u_l give the signed ones, d_l = u_l - B/2 (PackDigits, packing.hpp)
  uint32_t ap[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t w[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) ap[4 * q + e] = (((w[e] + rnd) >> (32 - bt)) + off) & btmask;
  }
  // -d_l = B/2 - u_l on four bytes at once: u < 128, so B/2 + 128 - u stays inside its byte, and ^ 0x80 makes it an i8
  const uint32_t bias = (128u + half) * 0x01010101u;
  uint4 *dst = reinterpret_cast<uint4 *>(dig + ct * (size_t)t * kN) + lane;
#pragma unroll 1
  for (int l = 0; l < t; ++l) {
    const int sh = basebit * (t - 1 - l);
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t u = ((ap[4 * q] >> sh) & bmask) | (((ap[4 * q + 1] >> sh) & bmask) << 8) |
                         (((ap[4 * q + 2] >> sh) & bmask) << 16) | (((ap[4 * q + 3] >> sh) & bmask) << 24);
      o[q] = (bias - u) ^ 0x80808080u;
    }
    dst[(size_t)l * (kN / 16)] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

}  // namespace tfhe

// ---- TRLWE key switch (trlwe_switch.hpp) -------------------------------------------------------------------------
namespace {
using TsKey = KeyState::TrlweSwitchKey;

const char *ts_shape_refusal(int k, int basebit, int t) {
  if (k < 1 || k >= 2 * kN || !(k & 1)) return "k must be odd, 1 <= k < 2N";
  if (basebit < 1 || basebit > kTsMaxBasebit) return "basebit out of range (1 .. 7: digits in one byte)";
  if (t < 1 || (size_t)t > kPolymulMaxCols) return "t out of range (1 .. 64)";
  if (basebit * t > kTsMaxBits) return "basebit * t exceeds 32";
  return nullptr;
}

TsKey *ts_find(KeyState &ks, int k) {
  for (TsKey &e : ks.tsk)
    if (e.loaded && e.k == k) return &e;
  return nullptr;
}

// the entry a key for k goes into: the one that answers for k now, else a free one; NULL: sixteen other keys are loaded
TsKey *ts_slot(KeyState &ks, int k) {
  if (TsKey *e = ts_find(ks, k)) return e;
  for (TsKey &e : ks.tsk)
    if (!e.loaded) return &e;
  return nullptr;
}

uint32_t ts_inverse(int k) {  // k kinv = 1 mod 2N (k odd)
  uint32_t x = 1;
  for (int i = 0; i < 4; ++i) x *= 2u - (uint32_t)k * x;  // Newton: 1 -> 2 -> 4 -> 8 -> 16 correct bits
  return x & (uint32_t)(2 * kN - 1);
}

size_t ts_row_bytes(int t) { return (size_t)t * 2 * kN * 4; }

// ctx->mu held, ctx's device current, arguments validated, `e` from ts_slot
int gen_trlwe_switch_key_locked(tfhe_hip_ctx *ctx, TsKey &e, const uint32_t *key_from, const uint32_t *key_to, int k,
                                int basebit, int t, double alpha, const ChaChaKey &rk, uint8_t mask_seed[32],
                                uint32_t *bodies) {
  CHK(begin_side_key(ctx, e.loaded, e.rows, ts_row_bytes(t)));
  StagedSecrets s(ctx, (size_t)kN);  // (wiped on every exit path)
  CHK(stage_secrets(ctx, key_from, key_to, rk, s));
  const uint32_t *d_from = s.d_k0;
  const double2 *d_spec = s.d_spec;  // of key_to
  const ChaChaKey *d_rk = s.d_rk;
  ChaChaKey seed;
  CHK(derive_public_seed<kStreamTksSeed>(ctx, s, seed));
  const size_t body_words = (size_t)t * kN;
  uint32_t *d_rows = e.rows;
  // the temporary: the bodies [t][N]; drained and freed on every path
  CHK(upload_through_temp(ctx, "TRLWE switching key generation", {}, body_words * 4, [&](void *tmp) {
    hipLaunchKernelGGL(k_gen_trlwe_switch_key, dim3((unsigned)t), dim3(64), kStageLdsBytes, ctx->stream, d_from, d_spec,
                       ctx->d_tw, d_rows, (uint32_t *)tmp, k, ts_inverse(k), basebit, alpha, d_rk, seed);
    if (const hipError_t err = hipGetLastError()) return err;
    if (bodies) return hipMemcpyAsync(bodies, tmp, body_words * 4, hipMemcpyDeviceToHost, ctx->stream);
    return hipSuccess;
  }));
  memcpy(mask_seed, seed.k, 32);
  e.k = k, e.basebit = basebit, e.t = t;
  commit_side_key(e.loaded);
  return TFHE_HIP_OK;
}

// in [count][2][N] -> out [count][2][N] on stream s, kTsChunk ciphertexts a pass through the context's scratch
int trlwe_switch_dev(tfhe_hip_ctx *ctx, const TsKey &e, const uint32_t *in, size_t count, uint32_t *out, hipStream_t s) {
  const size_t chunk = count < kTsChunk ? count : kTsChunk;
  const size_t dig_bytes = chunk * (size_t)e.t * kN;
  CHK(take(ctx, s, ctx->ts_dig, dig_bytes + chunk * (size_t)kN * 4));
  int8_t *d_dig = (int8_t *)ctx->ts_dig.p;
  uint32_t *d_bp = (uint32_t *)((unsigned char *)ctx->ts_dig.p + dig_bytes);
  for (size_t c0 = 0; c0 < count; c0 += chunk) {
    const size_t n = count - c0 < chunk ? count - c0 : chunk;
    {
      TimedScope timed(ctx->ev_ts_dig, s, ctx->profiling);  // (while profiling is on: tfhe_hip_get_trlwe_switch_times)
      CHK(hip_rc(ctx, timed.err));
      hipLaunchKernelGGL(k_trlwe_switch_digits, dim3((unsigned)n), dim3(64), 0, s, in + c0 * 2 * kN, e.k, e.basebit,
                         e.t, d_dig, d_bp);
      CHK(launched(ctx));  // (the pair is closed whichever way the launch ended)
      CHK(hip_rc(ctx, timed.close()));
    }
    TimedScope timed(ctx->ev_ts_mm, s, ctx->profiling);
    CHK(hip_rc(ctx, timed.err));
    CHK(polymul_dev(ctx, d_dig, d_bp, n, (size_t)e.t, e.rows, 1, out + c0 * 2 * kN, s));
    CHK(hip_rc(ctx, timed.close()));
  }
  return TFHE_HIP_OK;
}

// the checks both forms share: key, empty batch, pointers (returns TFHE_HIP_OK with *e NULL for an empty batch)
int trlwe_switch_checks(tfhe_hip_ctx *ctx, int k, const uint32_t *in, size_t count, const uint32_t *out, const TsKey **e) {
  *e = nullptr;
  const TsKey *found = ts_find(*ctx->K, k);
  if (!found) return fail(ctx, TFHE_HIP_ENOKEY, "no TRLWE switching key loaded for this k");
  if (count == 0) return TFHE_HIP_OK;
  if (!in || !out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  if (count > 0x7FFFFFFFull) return fail(ctx, TFHE_HIP_EINVAL, "count too large");
  *e = found;
  return TFHE_HIP_OK;
}
}  // namespace

int tfhe_hip_trlwe_switch_key_words(int t, size_t *body_words) {
  if (!body_words || t < 1 || (size_t)t > kPolymulMaxCols) return TFHE_HIP_EINVAL;
  *body_words = (size_t)t * kN;
  return TFHE_HIP_OK;
}

int tfhe_hip_gen_trlwe_switch_key(tfhe_hip_ctx *ctx, const uint32_t *key_from_lv1, const uint32_t *key_to_lv1, int k,
                                  int basebit, int t, double alpha, const uint8_t rng_key[32], uint8_t mask_seed[32],
                                  uint32_t *bodies) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  // validation first: a refused call leaves the old key for k answering
  if (!key_from_lv1 || !key_to_lv1 || !mask_seed) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  if (const char *why = ts_shape_refusal(k, basebit, t)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (!(alpha >= 0.0)) return fail(ctx, TFHE_HIP_EINVAL, "negative noise parameter");
  TsKey *e = ts_slot(*ctx->K, k);
  if (!e) return fail(ctx, TFHE_HIP_EINVAL, "sixteen TRLWE switching keys are loaded: drop one first");
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  return gen_trlwe_switch_key_locked(ctx, *e, key_from_lv1, key_to_lv1, k, basebit, t, alpha, gk.k, mask_seed, bodies);
}

int tfhe_hip_load_trlwe_switch_key(tfhe_hip_ctx *ctx, int k, int basebit, int t, const uint8_t mask_seed[32],
                                   const uint32_t *bodies) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (!mask_seed || !bodies) return fail(ctx, TFHE_HIP_EINVAL, "null key pointer");
  if (const char *why = ts_shape_refusal(k, basebit, t)) return fail(ctx, TFHE_HIP_EINVAL, why);
  TsKey *e = ts_slot(*ctx->K, k);
  if (!e) return fail(ctx, TFHE_HIP_EINVAL, "sixteen TRLWE switching keys are loaded: drop one first");
  CHK(begin_side_key(ctx, e->loaded, e->rows, ts_row_bytes(t)));
  uint32_t *d_rows = e->rows;
  CHK(upload_through_temp(ctx, "TRLWE switching key", {{bodies, (size_t)t * kN * 4}}, 0, [&](void *tmp) {
    hipLaunchKernelGGL(k_expand_trlwe_switch_key<64>, dim3((unsigned)t), dim3(64), 0, ctx->stream, (const uint32_t *)tmp,
                       d_rows, k, seed_key(mask_seed));
    return hipGetLastError();
  }));
  e->k = k, e->basebit = basebit, e->t = t;
  commit_side_key(e->loaded);
  return TFHE_HIP_OK;
}

// 0 / 1, never an error code, no device call and no lock (flag_is_loaded, key_change.hpp)
int tfhe_hip_trlwe_switch_key_is_loaded(tfhe_hip_ctx *ctx, int k) {
  if (!ctx) return 0;
  for (const TsKey &e : ctx->own.tsk)
    if (__atomic_load_n(&e.loaded, __ATOMIC_ACQUIRE) && e.k == k) return 1;
  return 0;
}

int tfhe_hip_drop_trlwe_switch_key(tfhe_hip_ctx *ctx, int k) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  TsKey *e = ts_find(*ctx->K, k);
  if (!e) return fail(ctx, TFHE_HIP_ENOKEY, "no TRLWE switching key loaded for this k");
  HIPCHK(ctx, hipDeviceSynchronize());  // calls queued on the caller's streams may still read the rows
  e->loaded = false;
  e->rows.release();
  return TFHE_HIP_OK;
}

int tfhe_hip_batch_trlwe_keyswitch(tfhe_hip_ctx *ctx, int k, const uint32_t *in, size_t count, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  const TsKey *e = nullptr;
  CHK(trlwe_switch_checks(ctx, k, in, count, out, &e));
  if (!e) return TFHE_HIP_OK;
  return host_call(ctx, false, {{in, trlwe_bytes(count), &ctx->a}}, out, trlwe_bytes(count), [&](const void *const *d, void *o) {
    return trlwe_switch_dev(ctx, *e, u32(d[0]), count, (uint32_t *)o, ctx->stream);
  });
}

int tfhe_hip_batch_trlwe_keyswitch_dev(tfhe_hip_ctx *ctx, int k, const uint32_t *in, size_t count, uint32_t *out,
                                       void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  const TsKey *e = nullptr;
  CHK(trlwe_switch_checks(ctx, k, in, count, out, &e));
  if (!e) return TFHE_HIP_OK;
  return trlwe_switch_dev(ctx, *e, in, count, out, pick(ctx, stream));
}

int tfhe_hip_get_trlwe_switch_times(tfhe_hip_ctx *ctx, tfhe_hip_trlwe_switch_times *out) {
  if (!ctx || !out) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  memset(out, 0, sizeof(*out));
  CHK(hip_rc(ctx, ctx->ev_ts_dig.drain(out->digits_ms, &out->passes)));
  return hip_rc(ctx, ctx->ev_ts_mm.drain(out->contraction_ms));
}
