// sym_encrypt.hpp -- symmetric (secret-key) TLWE lv0 encryption on the GPU, behind the C ABI: bulk ciphertexts, the
// public key's encryptions of zero and the symmetric proxy re-encryption key.
//
// The format is normative in include/tfhe_hip.h ("symmetric encryption").  All three are the row of
// TLWELv0::encrypt_f64 (tlwe.rs:37-53):
//
//   row g = (a, <a, s0> + plain + f64_to_torus(noise))      a: n keystream words, wrapping u32
//
// with the mask a under (mask key, g, mask domain) and the one noise sample under (K, g, noise domain).  A row has at
// most 80 keystream blocks, so ONE WAVE makes a row (k_gen_ksk spends a 256-thread workgroup and an LDS reduction on
// it): lane l makes block l (and l + 64 where n > 1024), multiplies its 16 words into s0 held in LDS, and the wave
// reduces with shuffles.  The lane just past the last mask block makes the row's noise block in the same pass -- under
// the other key and nonce, the same instructions -- and feeds f64_to_torus(g0) into the same reduction, so the noise
// costs no pass of its own.  Lane 0 adds the plaintext.
//
// Stores decide the speed (184 MB for 65,536 SECURITY_128_BIT rows).  A lane holds 16 consecutive words; stored from
// the registers, one store instruction of the wave would scatter 64 pieces of 64 bytes.  The row is staged in LDS
// instead (one word of padding per block: lane l's words start at 17 l, so the 64 writes of one instruction fall on
// distinct banks) and leaves in whole 16-byte chunks of the DESTINATION's alignment: rows are n + 1 words, so a row
// starts at any word of a chunk; the staged row is shifted by that and lane l stores chunk l, l + 64, ... -- one
// store instruction covers 1 KiB of contiguous bytes.  Only a row's first and last chunk are partial: word stores.
//
//   bulk TLWE        g = first_index + m, masks under the public seed S ("EWL": the seeded-TLWE masks), out [count][n+1]
//                    and / or bodies [count]; bodies-only mode stages and stores no mask.
//   public key       g = e < size, masks under K, plain 0, out [size][n+1]; k_pke_planes builds the byte planes from it.
//   re-encryption    g = base t i + base j + k, plain from (i, j, k) and key_from in the kernel, k = 0 rows zero, out
//                    in the engine layout of the key-switching key (rows of ksk_row_words(n), zero padding): what
//                    k_ksk_convert would have made, so no conversion pass follows.
//
// The kernel is a template: instantiations are emitted after the library's other kernels, whose code stays
// byte-identical.
#pragma once
#include "pk_encrypt.hpp"

namespace tfhe {

constexpr int kSymMaxN = 1279;                      // 80 keystream blocks: two passes of a wave
constexpr int kSymWaves = 4;                        // rows in flight per workgroup
constexpr int kSymRowsPerWave = 4;                  // rows a wave makes one after the other (s0 is loaded once)
constexpr int kSymKeyWords = 80 * 17;               // s0 in LDS: 17 words a block of 16
constexpr int kSymStageWords = 81 * 17;             // a row image: up to 3 words of shift + 1280 words, read in whole chunks

// word x of a row sits at x + x / 16 of its LDS image: 16 words, one of padding
__device__ __forceinline__ int sym_slot(int x) { return x + (x >> 4); }

// sec: [0] the mask key, [1] the noise key K (a device buffer the host wipes behind the launch), then s0 [n], then
// (re-encryption key) key_from [n].  Rows `rows`, row r of the launch is index g = first_index + r.
//   plain     != NULL: the plaintext torus words [rows]                                     (bulk)
//   from_key:          plain = f64_to_torus(((k key_from[i]) as u32 as f64) / 2^((j+1) basebit)), k = 0 rows zero
//   neither:           plain 0                                                               (public key)
//   out       != NULL: the rows, `stride` >= n + 1 words apart, words n + 1 .. stride - 1 zero
//   bodies    != NULL: the bodies [rows]
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_sym_encrypt(const uint32_t *__restrict__ sec, uint32_t dom_mask,
                                                             uint32_t dom_noise, uint64_t first_index, size_t rows, int n,
                                                             double alpha, const uint32_t *__restrict__ plain,
                                                             int from_key, int basebit, int t,
                                                             uint32_t *__restrict__ bodies, uint32_t *__restrict__ out,
                                                             int stride) {
  __shared__ uint32_t s_key[kSymKeyWords];
  __shared__ __attribute__((aligned(16))) uint32_t s_stage[WAVES][kSymStageWords];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = (n + 15) >> 4;  // mask blocks; block nb of the walk is the noise block
  ChaChaKey kmask, knoise;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    kmask.k[c] = sec[c];
    knoise.k[c] = sec[8 + c];
  }
  const uint32_t *s0 = sec + 16, *key_from = sec + 16 + n;
  for (int x = tid; x < n; x += 64 * WAVES) s_key[sym_slot(x)] = s0[x];
  __syncthreads();
  uint32_t *stage = s_stage[wave];
  const size_t row0 = ((size_t)blockIdx.x * WAVES + (size_t)wave) * kSymRowsPerWave;
#pragma unroll 1
  for (int it = 0; it < kSymRowsPerWave; ++it) {
    const size_t row = row0 + (size_t)it;
    if (row >= rows) break;  // (wave-uniform; nothing below synchronises across waves)
    const uint64_t g = first_index + (uint64_t)row;
    uint32_t *dst = out ? out + row * (size_t)stride : nullptr;
    // a row's image is shifted by the word its destination starts at within a 16-byte chunk
    const int shift = dst ? (int)(((uintptr_t)dst >> 2) & 3u) : 0;
    uint32_t pl = 0;
    bool zero_row = false;
    if (from_key) {
      const uint64_t base = (uint64_t)1 << basebit;
      const uint32_t k = (uint32_t)(g % base);
      const int j = (int)((g / base) % (uint64_t)t);
      const size_t i = (size_t)(g / (base * (uint64_t)t));
      zero_row = k == 0;  // never read by the re-encryption (proxy_reenc.rs:405-407): zero, its streams unused
      if (!zero_row) pl = dev_f64_to_torus((double)(uint32_t)(k * key_from[i]) * exp2(-(double)((j + 1) * basebit)));
    } else if (plain) {
      pl = plain[row];
    }
    uint32_t inner = 0;
    if (!zero_row) {
#pragma unroll 1
      for (int blk = lane; blk <= nb; blk += 64) {
        const bool noise = blk == nb;
        ChaChaKey key;
#pragma unroll
        for (int c = 0; c < 8; ++c) key.k[c] = noise ? knoise.k[c] : kmask.k[c];
        uint32_t w[16];
        chacha20_block(key, noise ? 0u : (uint32_t)blk, (uint32_t)g, (uint32_t)(g >> 32), noise ? dom_noise : dom_mask, w);
        if (noise) {
          double g0, g1;
          gauss2(w, alpha, g0, g1);
          inner += dev_f64_to_torus(g0);
        } else {
          const int at = 17 * blk;
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            if (16 * blk + c < n) {
              inner += s_key[at + c] * w[c];
              if (dst) stage[sym_slot(16 * blk + c + shift)] = w[c];
            }
          }
        }
      }
    }
    for (int off = 32; off > 0; off >>= 1) inner += __shfl_down(inner, off);
    const uint32_t body = zero_row ? 0u : inner + pl;
    if (lane == 0 && bodies) bodies[row] = body;
    if (!dst) continue;
    if (zero_row) {
      for (int x = lane; x < stride; x += 64) dst[x] = 0u;
      continue;
    }
    if (lane == 0) stage[sym_slot(n + shift)] = body;
    if (lane > 0 && n + lane < stride) stage[sym_slot(n + lane + shift)] = 0u;  // (stride - n - 1 <= 3)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // image words [shift, shift + stride) are the row; chunk q holds image words 4q .. 4q + 3
    const int end = shift + stride;
    uint32_t *dst0 = dst - shift;  // 16-byte aligned
    for (int q = lane; 4 * q < end; q += 64) {
      const int x0 = 4 * q;
      const uint4 v = make_uint4(stage[sym_slot(x0)], stage[sym_slot(x0 + 1)], stage[sym_slot(x0 + 2)], stage[sym_slot(x0 + 3)]);
      if (x0 >= shift && x0 + 4 <= end) {
        *reinterpret_cast<uint4 *>(dst0 + x0) = v;
      } else {
        const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (x0 + c >= shift && x0 + c < end) dst0[x0 + c] = e[c];
      }
    }
    // the next row's image is written by the same wave behind these reads (LDS operations of a wave stay in order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace tfhe

// ---- symmetric encryption (sym_encrypt.hpp) -----------------------------------------------------------------------
namespace {
inline size_t sym_blocks(size_t rows) {
  const size_t per = (size_t)kSymWaves * kSymRowsPerWave;
  return (rows + per - 1) / per;
}

// The secrets of one launch in the context's `sym_sec` buffer: mask key, K, s0 [n], key_from [n] (or nothing).  The
// copy has landed when this returns (the sources are the caller's and this frame's).
int sym_stage(tfhe_hip_ctx *ctx, const ChaChaKey &kmask, const ChaChaKey &knoise, const uint32_t *key_lv0,
              const uint32_t *key_from, hipStream_t s) {
  const int n = ctx->P.n;
  std::vector<uint32_t> h(16 + (size_t)n * (key_from ? 2 : 1));
  memcpy(h.data(), kmask.k, 32);
  memcpy(h.data() + 8, knoise.k, 32);
  memcpy(h.data() + 16, key_lv0, (size_t)n * 4);
  if (key_from) memcpy(h.data() + 16 + n, key_from, (size_t)n * 4);
  int rc = ensure(ctx, ctx->sym_sec, h.size() * 4);
  if (rc == TFHE_HIP_OK) {
    hipError_t e = hipMemcpyAsync(ctx->sym_sec.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(ctx, TFHE_HIP_EHIP, std::string("symmetric encryption: ") + hipGetErrorString(e));
  }
  volatile uint32_t *wipe = h.data();
  for (size_t i = 0; i < h.size(); ++i) wipe[i] = 0;
  return rc;
}

// zero the staged secrets behind whatever stream s has queued
int sym_wipe(tfhe_hip_ctx *ctx, hipStream_t s) {
  if (ctx->sym_sec.p) HIPCHK(ctx, hipMemsetAsync(ctx->sym_sec.p, 0, ctx->sym_sec.cap, s));
  return TFHE_HIP_OK;
}

struct SymJob {
  uint32_t dom_mask, dom_noise;
  uint64_t first_index;
  size_t rows;
  double alpha;
  const uint32_t *plain;  // device, or NULL
  bool from_key;
  uint32_t *bodies, *out;  // device, either may be NULL
  int stride;
};

int sym_launch(tfhe_hip_ctx *ctx, const SymJob &j, hipStream_t s) {
  const tfhe_hip_params &P = ctx->P;
  hipLaunchKernelGGL(k_sym_encrypt<kSymWaves>, dim3((unsigned)sym_blocks(j.rows)), dim3(64 * kSymWaves), 0, s,
                     (const uint32_t *)ctx->sym_sec.p, j.dom_mask, j.dom_noise, j.first_index, j.rows, P.n, j.alpha, j.plain,
                     j.from_key ? 1 : 0, P.basebit, P.t, j.bodies, j.out, j.stride);
  return launched(ctx);
}

const char *sym_refusal(const tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *plain, size_t count, double alpha,
                        const uint8_t *mask_seed, uint64_t first_index, const uint32_t *bodies, const uint32_t *out) {
  if (!key_lv0 || !mask_seed || !plain) return "null pointer";
  if (count && !bodies && !out) return "no output: bodies and out are both null";
  if (!(alpha >= 0.0)) return "negative noise parameter";
  if (count && first_index + (uint64_t)(count - 1) < first_index) return "the row indices run past 2^64";
  if (count > 0x7FFFFFFFull) return "count too large";
  if (ctx->P.n > kSymMaxN) return "n too large";
  return nullptr;
}

// on stream s: stage, launch, wipe.  plain / bodies / out are device pointers.
int sym_bulk(tfhe_hip_ctx *ctx, const ChaChaKey &seed, const ChaChaKey &k, const uint32_t *key_lv0, const uint32_t *plain,
             size_t count, double alpha, uint64_t first_index, uint32_t *bodies, uint32_t *out, hipStream_t s) {
  CHK(claim_scratch(ctx, s));  // sym_sec belongs to the context
  CHK(sym_stage(ctx, seed, k, key_lv0, nullptr, s));
  const int rc = sym_launch(ctx, {kSeedDomainTlwe, kSeedDomainSymNoise, first_index, count, alpha, plain, false, bodies, out,
                                  ctx->P.n + 1}, s);
  const int rc_wipe = sym_wipe(ctx, s);
  return rc != TFHE_HIP_OK ? rc : rc_wipe;
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
  // the primary output returns through host_call; with both asked for, the bodies ride in staging buffer b
  uint32_t *primary = out ? out : bodies;
  const size_t primary_bytes = out ? tlwe_bytes(ctx, count) : count * 4;
  if (out && bodies) CHK(ensure(ctx, ctx->b.dev, count * 4));
  int rc = host_call(ctx, false, {{plain, count * 4, &ctx->a}}, primary, primary_bytes, [&](const void *const *d, void *o) {
    uint32_t *d_out = out ? (uint32_t *)o : nullptr;
    uint32_t *d_bodies = out ? (bodies ? (uint32_t *)ctx->b.dev.p : nullptr) : (uint32_t *)o;
    return sym_bulk(ctx, seed, gk.k, key_lv0, u32(d[0]), count, alpha, first_index, d_bodies, d_out, ctx->stream);
  });
  if (rc == TFHE_HIP_OK && out && bodies) rc = to_host(ctx, bodies, ctx->b, count * 4);
  // neither the secrets nor the plaintexts stay behind on the device (best effort: the call's status is rc)
  (void)sym_wipe(ctx, ctx->stream);
  if (ctx->a.dev.p && ctx->a.dev.cap >= count * 4) (void)hipMemsetAsync(ctx->a.dev.p, 0, count * 4, ctx->stream);
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
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
  if (P.n > kSymMaxN) return fail(ctx, TFHE_HIP_EINVAL, "n too large");
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  KeyState &k = *ctx->K;
  const size_t bytes = pke_plane_bytes(P.n, (int)size), chunks = bytes / 16, enc_bytes = size * (size_t)(P.n + 1) * 4;
  CHK(begin_side_key(ctx, k.pke_loaded, k.d_pke8, k.pke_cap, bytes));
  CHK(claim_scratch(ctx, ctx->stream));
  int rc = sym_stage(ctx, gk.k, gk.k, key_lv0, nullptr, ctx->stream);
  if (rc == TFHE_HIP_OK)
    rc = upload_through_temp(ctx, "public key generation", {}, enc_bytes, [&](void *d_enc) -> hipError_t {
      if (sym_launch(ctx, {kSeedDomainPkMask, kSeedDomainPkNoise, 0, size, alpha, nullptr, false, nullptr, (uint32_t *)d_enc,
                           P.n + 1}, ctx->stream) != TFHE_HIP_OK)
        return hipErrorLaunchFailure;
      hipLaunchKernelGGL(k_pke_planes<256>, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, ctx->stream,
                         (const uint32_t *)d_enc, k.d_pke8, P.n, (int)size, chunks);
      if (const hipError_t e = hipGetLastError()) return e;
      if (encryptions_out) return hipMemcpyAsync(encryptions_out, d_enc, enc_bytes, hipMemcpyDeviceToHost, ctx->stream);
      return hipSuccess;
    });
  (void)sym_wipe(ctx, ctx->stream);
  (void)hipStreamSynchronize(ctx->stream);
  CHK(rc);
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
  CHK(claim_scratch(ctx, ctx->stream));
  int rc = sym_stage(ctx, gk.k, gk.k, key_to, key_from, ctx->stream);
  if (rc == TFHE_HIP_OK) {
    hipError_t e = hipMemsetAsync(ctx->K->d_ksk, 0, ksk_bytes(P), ctx->stream);
    if (e != hipSuccess) rc = fail(ctx, TFHE_HIP_EHIP, std::string("re-encryption key generation: ") + hipGetErrorString(e));
  }
  if (rc == TFHE_HIP_OK)
    rc = sym_launch(ctx, {kSeedDomainRkMask, kSeedDomainRkNoise, 0, rows, alpha, nullptr, true, nullptr, ctx->K->d_ksk,
                          ksk_row_words(P.n)}, ctx->stream);
  if (rc == TFHE_HIP_OK && key_out)
    rc = upload_through_temp(ctx, "re-encryption key export", {}, key_words * 4, [&](void *d_ref) -> hipError_t {
      hipLaunchKernelGGL(k_ksk_export, dim3((unsigned)rows), dim3(256), 0, ctx->stream, (const uint32_t *)ctx->K->d_ksk,
                         (uint32_t *)d_ref, P.n, rows);
      if (const hipError_t e = hipGetLastError()) return e;
      return hipMemcpyAsync(key_out, d_ref, key_words * 4, hipMemcpyDeviceToHost, ctx->stream);
    });
  (void)sym_wipe(ctx, ctx->stream);
  (void)hipStreamSynchronize(ctx->stream);
  CHK(rc);
  return commit_reenc_key(ctx);
}
