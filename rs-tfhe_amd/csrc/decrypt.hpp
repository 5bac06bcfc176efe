// decrypt.hpp -- decryption on the GPU, behind the C ABI: phases, booleans and messages of LWE rows (lv0 ciphertexts
// under key_lv0, or lv1 rows under key_lv1) and of the slots of packed TRLWE ciphertexts.
//
// The format is normative in include/tfhe_hip.h ("decryption"); rs-tfhe_amd/client.py (SecretKey.phase, decrypt_bool,
// decrypt_lwe_message, packed_phase) is the definition every word is held to.  All of it is exact integer arithmetic
// but the MESSAGE decode, which is the f64 expression of decrypt_decode.hpp.
//
//   k_lwe_phase     out[r] = decode(b_r - <a_r, s>) over rows of key_len + 1 words.  A read stream: 4 (key_len + 1) bytes
//                   in and 4 out per row.  The key is binary, so a mask word is added or not, and the key is held as
//                   bits in one register a lane: the host packs them in the order the lanes walk a row, a wave loads its
//                   register once and walks rows grid-stride (the grid is sized from the CU count, not from the rows).
//                   Per row: coalesced loads, an and-add per word, a wave shuffle reduction, lane 0 subtracts from the
//                   body, decodes and stores.  No LDS, no atomics.  The loads are dwords at lane stride 1, 256
//                   contiguous bytes an instruction.  The other shape that was written -- aligned dwordx4 chunks of the
//                   row's 16-byte image, the mirror of k_lwe_rows's store path, with four key registers for the four
//                   phases a row of key_len + 1 words can start at -- passed the same tests and was no faster:
//                   profiles/decrypt_bench.json (`variants`, `kernel_trace`) has both.  The dword form is kept; the
//                   source of the other is not in the tree.
//   k_trlwe_phase   one workgroup a TRLWE: [-A | A] (the `ext` of seeded.negacyclic_binary) and the list of set key
//                   indices in LDS, thread t sums ext[N + c - j] over the set j for c = t, t + 256, ... (consecutive
//                   lanes read consecutive words: no bank conflict) and decodes B[c] - sum.  Of the last group
//                   only the first count - g N coefficients are decoded and stored (the sums run for all four of a
//                   thread's coefficients: 1 M adds a group either way).
//
// Secrets travel as in sym_encrypt.hpp: the packed key bits (or the index list) go through a SecretStage (secrets.hpp)
// over the context's `sym_sec` buffer: the host copy is wiped, the buffer zeroed behind the kernel on the same stream.
#pragma once
#include "decrypt_decode.hpp"
#include "internal.hpp"

static_assert(kDecryptPhase == TFHE_HIP_DECRYPT_PHASE && kDecryptBool == TFHE_HIP_DECRYPT_BOOL &&
                  kDecryptMessage == TFHE_HIP_DECRYPT_MESSAGE,
              "decrypt_decode.hpp and include/tfhe_hip.h name the same modes");

namespace {
constexpr int kDecWaves = 4;        // waves a workgroup of k_lwe_phase
constexpr int kDecBlocksPerCu = 8;  // ... and workgroups a CU: 32 waves, every wave slot of the CU
// The staged key of k_lwe_phase: word l < 64 is lane l's register, bit k of it s[l + 64 k].  kLweMaxN words: 20 bits.
constexpr int kDecKeyWords = 64;
static_assert((kLweMaxN + 63) / 64 <= 32, "a lane's key bits fit a register");

__global__ __launch_bounds__(64 * kDecWaves) void k_lwe_phase(const uint32_t *__restrict__ in, const uint32_t *__restrict__ keybits,
                                                              int n, size_t rows, int mode, uint32_t modulus,
                                                              uint32_t *__restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t waves = (size_t)gridDim.x * kDecWaves;
  const uint32_t kb = keybits[lane];
  const int full = n & ~63;
#pragma unroll 1
  for (size_t row = (size_t)blockIdx.x * kDecWaves + (size_t)wave; row < rows; row += waves) {  // (wave-uniform)
    const uint32_t *p = in + row * (size_t)(n + 1);
    uint32_t acc = 0, bits = kb;
#pragma unroll 4
    for (int x0 = 0; x0 < full; x0 += 64, bits >>= 1) acc += p[x0 + lane] & (0u - (bits & 1u));
    if (full + lane < n) acc += p[full + lane] & (0u - ((TFHE_MUT(kMut_dec_tail_bit) ? kb : bits) & 1u));
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if (lane == 0) out[row] = decrypt_decode(p[n] - acc, mode, modulus);
  }
}

// idx: [0] the number of set bits of key_lv1, then their indices, ascending
__global__ __launch_bounds__(256) void k_trlwe_phase(const uint32_t *__restrict__ trlwe, const uint32_t *__restrict__ idx,
                                                     size_t count, int mode, uint32_t modulus, uint32_t *__restrict__ out) {
  __shared__ uint32_t s_ext[2 * kN];
  __shared__ uint16_t s_idx[kN];
  const int tid = threadIdx.x;
  const size_t g = blockIdx.x, first = g * (size_t)kN;
  const uint32_t *a = trlwe + g * (size_t)(2 * kN), *b = a + kN;
  const int set = (int)idx[0];
  for (int x = tid; x < kN; x += 256) {
    const uint32_t w = a[x];
    s_ext[x] = TFHE_MUT(kMut_dec_wrap) ? ~w : 0u - w;
    s_ext[kN + x] = w;
    if (x < set) s_idx[x] = (uint16_t)idx[1 + x];
  }
  __syncthreads();
  const size_t left = count - first;  // (the launch has no group past the last result: left >= 1)
  const int lim = left < (size_t)kN ? (int)left : kN;
  uint32_t sum[4] = {0u, 0u, 0u, 0u};
  const uint32_t *e = s_ext + kN + tid;
  for (int q = 0; q < set; ++q) {
    const int j = s_idx[q];
#pragma unroll
    for (int i = 0; i < 4; ++i) sum[i] += e[256 * i - j];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i;
    if (c < lim) out[first + (size_t)c] = decrypt_decode(b[c] - sum[i], mode, modulus);
  }
}

// the checks both forms share, in sym_refusal's style: why the call is TFHE_HIP_EINVAL, or nullptr
const char *dec_refusal(const uint32_t *key, size_t key_len, const uint32_t *in, size_t count, size_t capacity, int mode,
                        uint32_t modulus, const uint32_t *out) {
  if (!key || !in || !out) return "null pointer";
  if (mode != TFHE_HIP_DECRYPT_PHASE && mode != TFHE_HIP_DECRYPT_BOOL && mode != TFHE_HIP_DECRYPT_MESSAGE)
    return "mode must be TFHE_HIP_DECRYPT_PHASE, _BOOL or _MESSAGE";
  if (mode == TFHE_HIP_DECRYPT_MESSAGE && (modulus < 2 || modulus > 65536)) return "message modulus must be in [2, 65536]";
  if (count > 0x7FFFFFFFull) return "count too large";
  if (count > capacity) return "count exceeds the slots of the packed ciphertexts (groups * 1024)";
  for (size_t x = 0; x < key_len; ++x)
    if (key[x] > 1u) return "secret keys are binary";
  return nullptr;
}

// on stream s: stage, launch, wipe.  in / out are device pointers, key a host pointer.
int dec_lwe(tfhe_hip_ctx *ctx, const uint32_t *key, size_t key_len, const uint32_t *in, size_t count, int mode, uint32_t modulus,
            uint32_t *out, hipStream_t s) {
  SecretStage sec(ctx, ctx->sym_sec, s, kDecKeyWords * 4);
  uint32_t *h = (uint32_t *)sec.host(0);  // (zero so far)
  for (size_t x = 0; x < key_len; ++x)
    if (key[x]) h[x & 63] |= 1u << (x >> 6);
  int rc = sec.land("decryption: ");
  if (rc == TFHE_HIP_OK) {
    const size_t want = (count + kDecWaves - 1) / kDecWaves, cap = (size_t)(ctx->num_cus > 0 ? ctx->num_cus : 1) * kDecBlocksPerCu;
    const dim3 grid((unsigned)(want < cap ? want : cap)), block(64 * kDecWaves);
    hipLaunchKernelGGL(k_lwe_phase, grid, block, 0, s, in, sec.dev(0), (int)key_len, count, mode, modulus, out);
    rc = launched(ctx);
  }
  return sec.finish(rc);
}

int dec_trlwe(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const uint32_t *trlwe, size_t count, int mode, uint32_t modulus,
              uint32_t *out, hipStream_t s) {
  SecretStage sec(ctx, ctx->sym_sec, s, (1 + (size_t)kN) * 4);
  uint32_t *h = (uint32_t *)sec.host(0);  // (zero so far: the words past the last index stay so)
  uint32_t set = 0;
  for (uint32_t j = 0; j < (uint32_t)kN; ++j)
    if (key_lv1[j]) h[1 + set++] = j;
  h[0] = set;
  int rc = sec.land("decryption: ");
  if (rc == TFHE_HIP_OK) {
    const size_t groups = (count + kN - 1) / kN;  // groups past the last result are not touched
    hipLaunchKernelGGL(k_trlwe_phase, dim3((unsigned)groups), dim3(256), 0, s, trlwe, sec.dev(0), count, mode, modulus, out);
    rc = launched(ctx);
  }
  return sec.finish(rc);
}

bool dec_key_len_ok(const tfhe_hip_ctx *ctx, size_t key_len) { return key_len == (size_t)ctx->P.n || key_len == (size_t)kN; }

// the slots of `groups` packed ciphertexts (saturating: any count the checks let through fits)
size_t dec_slots(size_t groups) { return groups > SIZE_MAX / (size_t)kN ? SIZE_MAX : groups * (size_t)kN; }
}  // namespace

int tfhe_hip_batch_decrypt(tfhe_hip_ctx *ctx, const uint32_t *key, size_t key_len, const uint32_t *in, size_t count, int mode,
                           uint32_t modulus, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (!dec_key_len_ok(ctx, key_len)) return fail(ctx, TFHE_HIP_EINVAL, "key_len must be the parameter set's n or N = 1024");
  if (const char *why = dec_refusal(key, key_len, in, count, count, mode, modulus, out)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  const int rc = host_call(ctx, false, {{in, count * (key_len + 1) * 4, &ctx->a}}, out, count * 4, [&](const void *const *d, void *o) {
    return dec_lwe(ctx, key, key_len, u32(d[0]), count, mode, modulus, (uint32_t *)o, ctx->stream);
  });
  scrub(ctx->stream, {{&ctx->out, count * 4}});  // the decrypted words do not stay behind in the library's buffers
  return rc;
}

int tfhe_hip_batch_decrypt_dev(tfhe_hip_ctx *ctx, const uint32_t *key, size_t key_len, const uint32_t *in, size_t count, int mode,
                               uint32_t modulus, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (!dec_key_len_ok(ctx, key_len)) return fail(ctx, TFHE_HIP_EINVAL, "key_len must be the parameter set's n or N = 1024");
  if (const char *why = dec_refusal(key, key_len, in, count, count, mode, modulus, out)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  return dec_lwe(ctx, key, key_len, in, count, mode, modulus, out, pick(ctx, stream));
}

int tfhe_hip_batch_decrypt_trlwe(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const uint32_t *trlwe, size_t groups, size_t count,
                                 int mode, uint32_t modulus, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (const char *why = dec_refusal(key_lv1, kN, trlwe, count, dec_slots(groups), mode, modulus, out))
    return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  const size_t used = (count + kN - 1) / kN;  // the groups that hold results
  const int rc = host_call(ctx, false, {{trlwe, trlwe_bytes(used), &ctx->a}}, out, count * 4, [&](const void *const *d, void *o) {
    return dec_trlwe(ctx, key_lv1, u32(d[0]), count, mode, modulus, (uint32_t *)o, ctx->stream);
  });
  scrub(ctx->stream, {{&ctx->out, count * 4}});  // the decrypted words do not stay behind in the library's buffers
  return rc;
}

int tfhe_hip_batch_decrypt_trlwe_dev(tfhe_hip_ctx *ctx, const uint32_t *key_lv1, const uint32_t *trlwe, size_t groups,
                                     size_t count, int mode, uint32_t modulus, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (const char *why = dec_refusal(key_lv1, kN, trlwe, count, dec_slots(groups), mode, modulus, out))
    return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  return dec_trlwe(ctx, key_lv1, trlwe, count, mode, modulus, out, pick(ctx, stream));
}
