// pk_encrypt.hpp -- public-key encryption and the asymmetric proxy re-encryption key on the GPU, behind the C ABI.
//
// The format is normative in include/tfhe_hip.h ("public-key encryption and the asymmetric re-encryption key").  A
// public key is E [size][n+1], encryptions of zero (proxy_reenc.rs:95-99).  Ciphertext g is a signed subset sum
//
//   out[g] = sum_{e < size} c_e E[e]   (all n + 1 words, wrapping)   then   out[g].b += plain + f64_to_torus(noise)
//
// with c_e in {-1, 0, +1} read off two bits of a ChaCha20 keystream under a secret generator key K: the two gen_bool
// draws of proxy_reenc.rs:168-200.  That is ONE exact integer contraction, the shape of the packing key switch
// (packing.hpp): E is split once, at load, into four balanced signed byte planes (ks_plane_byte), every plane is an
// i8 x i8 -> i32 matrix-core product with |acc| <= 128 size <= 2^20 (size <= 8192), and sum_p acc_p << 8p wraps to the
// u32 result -- equal word for word.  The asymmetric re-encryption key (proxy_reenc.rs:271-326) is n t base such
// ciphertexts of k key_from[i] / 2^((j+1) basebit) in the layout [n][t][base][n+1], the k = 0 rows zero.
//
//   k_pke_planes     E -> byte planes [plane][column tile][step][lane][16 B] (k_pack_planes' layout): the K axis is
//                    the entry e in steps of 32, the columns are the n + 1 words padded to whole groups of kPkeNT tiles.
//   k_pke_selectors  the keystream pass: selector words [rows][2 steps] (a lane's A fragment of one K-step is exactly
//                    one word: 16 two-bit fields) and the body's addend plain + noise [rows].  The row's place in its
//                    batch, its plaintext and whether it is a zero row (k = 0) are decided HERE, so the contraction
//                    below is the same instantiation for ciphertexts and for key rows: output row = input row.
//   k_pke_mfma       grid (ceil(rows / 32), column groups), 4 waves = the 4 byte planes: the byte-plane K-walk of
//                    packing.hpp (plane_walk) with the selector words as the A side, no K split (steps <= 256).  The
//                    planes are summed (plane_merge) in a 32 x 32 kPkeNT LDS tile that goes out in coalesced row
//                    stores; column n receives the addend; columns past n are dropped.
#pragma once
#include "packing.hpp"

namespace tfhe {

constexpr int kPkeNT = 8;                            // column tiles per wave: the LDS tile is 32 x 256 words
constexpr int kPkeMaxSize = 8192;                    // |acc| <= 128 size <= 2^20; steps <= 256
constexpr size_t kPkeChunkRows = (size_t)1 << 16;    // rows per pass: bounds the selector scratch (23 MiB at size 1400)

__host__ __device__ __forceinline__ int pke_steps(int size) { return (size + 31) / 32; }  // K-steps of 32 entries
__host__ __device__ __forceinline__ int pke_tiles(int n) {  // 32-column tiles of n + 1 words, in whole groups
  return ((n + 1 + 32 * kPkeNT - 1) / (32 * kPkeNT)) * kPkeNT;
}
__host__ __device__ __forceinline__ size_t pke_plane_bytes(int n, int size) {
  return (size_t)4 * pke_tiles(n) * pke_steps(size) * 1024;
}
__host__ __device__ __forceinline__ size_t pke_sel_words(size_t rows, int size) {  // selectors, then the addends
  return rows * (size_t)(2 * pke_steps(size)) + rows;
}

// E [size][n+1] u32 -> byte planes [plane p][tile ct][step s][lane][16 B]: lane = (column 32 ct + (lane & 31),
// kb = lane >> 5), byte b = plane byte p of E[32 s + 16 kb + b] at that column; 0 for entries >= size and columns > n.
template <int WG>
__global__ __launch_bounds__(WG) void k_pke_planes(const uint32_t *__restrict__ enc, unsigned char *__restrict__ out,
                                                    int n, int size, size_t chunks) {
  const size_t idx = (size_t)blockIdx.x * WG + threadIdx.x;
  if (idx >= chunks) return;
  const int lane = (int)(idx & 63);
  size_t r = idx >> 6;
  const int S = pke_steps(size), T = pke_tiles(n);
  const int s = (int)(r % (size_t)S);
  r /= (size_t)S;
  const int ct = (int)(r % (size_t)T), p = (int)(r / (size_t)T);
  const int col = ct * 32 + (lane & 31), kb = lane >> 5;
  reinterpret_cast<uint4 *>(out)[idx] = ks_plane_fragment(p, [=](int q, int b) {
    const int e = 32 * s + 16 * kb + 4 * q + b;
    return (e < size && col <= n) ? enc[(size_t)e * (size_t)(n + 1) + col] : 0u;
  });
}

// One lane per (row, keystream block): blocks 0 .. nblk-1 of the selector stream give selector words 16 blk .. 16 blk + 15
// of the row (bits of entries >= size cleared), the lane past them makes the row's noise sample and writes
// addend[row] = plain + f64_to_torus(g0).  Row `row` of the launch is index g = first_index + row of its stream.
//   plain != NULL:  an encryption of plain[row]                                  (public-key encryption)
//   key_from != NULL: key row g = base t i + base j + k of key_from [n]: plain = f64_to_torus(((k key_from[i]) as u32
//                   as f64) / 2^((j+1) basebit)); a k = 0 row gets all-zero selectors and addend, its streams unused.
template <int WG>
__global__ __launch_bounds__(WG) void k_pke_selectors(ChaChaKey key, uint64_t first_index, size_t rows, int size,
                                                       double alpha, uint32_t dom_sel, uint32_t dom_noise,
                                                       const uint32_t *__restrict__ plain,
                                                       const uint32_t *__restrict__ key_from, int basebit, int t,
                                                       uint32_t *__restrict__ sel, uint32_t *__restrict__ addend) {
  const int words = 2 * pke_steps(size), nblk = (words + 15) / 16;
  const size_t idx = (size_t)blockIdx.x * WG + threadIdx.x;
  if (idx >= rows * (size_t)(nblk + 1)) return;
  const size_t row = idx / (size_t)(nblk + 1);
  const int blk = (int)(idx % (size_t)(nblk + 1));
  const uint64_t g = first_index + (uint64_t)row;
  uint32_t *srow = sel + row * (size_t)words;
  uint32_t pl = 0;
  if (key_from) {
    if (!key_row_plain(g, basebit, t, key_from, pl)) {  // never read by the re-encryption (proxy_reenc.rs:311-313): zero
      if (blk == nblk) addend[row] = 0u;
      else
        for (int q = 0; q < 16 && 16 * blk + q < words; ++q) srow[16 * blk + q] = 0u;
      return;
    }
  } else {
    pl = plain[row];
  }
  if (blk == nblk) {
    addend[row] = pl + noise_sample(key, (uint32_t)g, (uint32_t)(g >> 32), dom_noise, alpha);
    return;
  }
  uint32_t w[16];
  chacha20_block(key, (uint32_t)blk, (uint32_t)g, (uint32_t)(g >> 32), dom_sel, w);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int ws = 16 * blk + q;
    if (ws >= words) break;
    const int left = size - 16 * ws;  // entries of this word below size
    const uint32_t mask = left >= 16 ? 0xFFFFFFFFu : (left <= 0 ? 0u : (1u << (2 * left)) - 1u);
    srow[ws] = w[q] & mask;
  }
}

// 16 two-bit fields (take, sign) -> 16 signed bytes in {0, +1, -1}: bytes 4q .. 4q+3 of the fragment from bits 8q .. 8q+7
__device__ __forceinline__ uint32_t pke_expand4(uint32_t x) {
  const uint32_t take = (x & 1u) | ((x & 4u) << 6) | ((x & 16u) << 12) | ((x & 64u) << 18);
  const uint32_t y = x >> 1;
  const uint32_t sign = (y & 1u) | ((y & 4u) << 6) | ((y & 16u) << 12) | ((y & 64u) << 18);
  return take | ((take & sign) * 0xFEu);  // 1 -> 0x01, 1 with sign -> 0xFF, no carry between bytes
}

// grid (ceil(rows / 32), pke_tiles(n) / NT), 4 waves: wave w = byte plane w.  out [rows][n+1].
// Two workgroups per CU (at most 256 registers a lane, no spill), 32 KiB of LDS each at NT = 8.
template <int NT>
__global__ __launch_bounds__(256, 2) void k_pke_mfma(const uint32_t *__restrict__ sel,
                                                   const uint32_t *__restrict__ addend, size_t rows, int n, int steps,
                                                   const unsigned char *__restrict__ pke8, uint32_t *__restrict__ out) {
  constexpr int CG = 32 * NT;
  __shared__ uint32_t tile[32 * CG];
  const int tid = threadIdx.x, lane = tid & 63, kb = lane >> 5;
  const int plane = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int d = tid; d < 32 * CG; d += 256) tile[d] = 0u;
  const size_t row0 = (size_t)blockIdx.x * 32, row = row0 + (size_t)(lane & 31);
  const bool live = row < rows;
  // selector word 2 s + kb of the row is the lane's A fragment of step s (entries 32 s + 16 kb .. + 15)
  const uint32_t *srow = sel + (live ? row : 0) * (size_t)(2 * steps) + kb;
  const int ct0 = (int)blockIdx.y * NT, tiles = (int)gridDim.y * NT;
  km_i32x16 acc[NT];
  uint32_t wc = live ? srow[0] : 0u;  // a 0 word takes no entry
  plane_walk<NT>(pke8 + ((size_t)(plane * tiles + ct0) * steps) * 1024 + (size_t)lane * 16, (size_t)steps * 1024, 0, steps,
                 [&](int s) {
                   const uint32_t wn = live ? srow[2 * (s + 1 < steps ? s + 1 : s)] : 0u;  // one step ahead, as the tiles
                   km_u32x4 a;
#pragma unroll
                   for (int q = 0; q < 4; ++q) a[q] = pke_expand4((wc >> (8 * q)) & 0xFFu);
                   wc = wn;
                   return __builtin_bit_cast(km_i32x4, a);
                 },
                 acc);
  __syncthreads();  // (the tile is zeroed)
  plane_merge<NT>(acc, plane, lane, [&](int r) { return tile + r * CG; });
  __syncthreads();
  for (int r = 0; r < 32; ++r) {
    const size_t orow = row0 + (size_t)r;
    if (orow >= rows) break;
    uint32_t *o = out + orow * (size_t)(n + 1);
    for (int cc = tid; cc < CG; cc += 256) {
      const int col = ct0 * 32 + cc;
      if (col > n) continue;  // the padding of the last column group
      uint32_t v = tile[r * CG + cc];
      if (col == n) v += addend[orow];
      o[col] = v;
    }
  }
}

}  // namespace tfhe

// ---- public-key encryption (pk_encrypt.hpp) ---------------------------------------------------------------------
namespace {
int need_public_key(tfhe_hip_ctx *ctx) {
  if (!ctx->K->pke_loaded) return fail(ctx, TFHE_HIP_ENOKEY, "public key not loaded");
  return TFHE_HIP_OK;
}

// Selectors and addends of `rows` rows into `sel`, then the contraction into out [rows][n+1], on stream s; the
// selectors (whoever reads them can strip the masks) are zeroed behind the contraction.
int pke_rows_launch(tfhe_hip_ctx *ctx, const ChaChaKey &k, uint64_t first_index, size_t rows, double alpha,
                    const uint32_t *plain, const uint32_t *key_from, uint32_t *sel, uint32_t *out, hipStream_t s) {
  const tfhe_hip_params &P = ctx->P;
  const int size = ctx->K->pke_size, steps = pke_steps(size), nblk = (2 * steps + 15) / 16;
  uint32_t *addend = sel + rows * (size_t)(2 * steps);
  const size_t lanes = rows * (size_t)(nblk + 1);
  {
    TimedScope timed(ctx->ev_pke_sel, s, ctx->profiling);  // (while profiling is on: tfhe_hip_get_pk_encrypt_times)
    CHK(hip_rc(ctx, timed.err));
    hipLaunchKernelGGL(k_pke_selectors<256>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, k, first_index, rows,
                       size, alpha, key_from ? kSeedDomainRkeSel : kSeedDomainPkeSel,
                       key_from ? kSeedDomainRkeNoise : kSeedDomainPkeNoise, plain, key_from, P.basebit, P.t, sel, addend);
    CHK(launched(ctx));  // (the pair is closed whichever way the launch ended)
    CHK(hip_rc(ctx, timed.close()));
  }
  {
    TimedScope timed(ctx->ev_pke_mm, s, ctx->profiling);
    CHK(hip_rc(ctx, timed.err));
    hipLaunchKernelGGL(k_pke_mfma<kPkeNT>, dim3((unsigned)((rows + 31) / 32), (unsigned)(pke_tiles(P.n) / kPkeNT)), dim3(256),
                       0, s, sel, addend, rows, P.n, steps, (const unsigned char *)ctx->K->d_pke8, out);
    CHK(launched(ctx));
    CHK(hip_rc(ctx, timed.close()));
  }
  HIPCHK(ctx, hipMemsetAsync(sel, 0, pke_sel_words(rows, size) * 4, s));
  return TFHE_HIP_OK;
}

// plain [count] -> out [count][n+1] on stream s (device pointers), kPkeChunkRows rows a pass
int pke_launch(tfhe_hip_ctx *ctx, const ChaChaKey &k, uint64_t first_index, const uint32_t *plain, size_t count,
               double alpha, uint32_t *out, hipStream_t s) {
  const size_t first = count < kPkeChunkRows ? count : kPkeChunkRows;
  CHK(take(ctx, s, ctx->pke_sel, pke_sel_words(first, ctx->K->pke_size) * 4));  // (pke_sel belongs to the context)
  for (size_t lo = 0; lo < count; lo += kPkeChunkRows) {
    const size_t rows = count - lo < kPkeChunkRows ? count - lo : kPkeChunkRows;
    CHK(pke_rows_launch(ctx, k, first_index + lo, rows, alpha, plain + lo, nullptr, (uint32_t *)ctx->pke_sel.p,
                        out + lo * (size_t)(ctx->P.n + 1), s));
  }
  return TFHE_HIP_OK;
}

const char *pke_refusal(const uint32_t *plain, size_t count, double alpha, const uint32_t *out) {
  if (count && (!plain || !out)) return "null pointer";
  if (!(alpha >= 0.0)) return "negative noise parameter";
  if (count > 0x7FFFFFFFull) return "count too large";
  return nullptr;
}
}  // namespace

int tfhe_hip_load_public_key(tfhe_hip_ctx *ctx, const uint32_t *encryptions, size_t size) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  // validation first: a refused call leaves the old public key encrypting
  if (!encryptions) return fail(ctx, TFHE_HIP_EINVAL, "null key pointer");
  if (size < 1 || size > (size_t)kPkeMaxSize)
    return fail(ctx, TFHE_HIP_EINVAL, "public key size must be in [1, 8192] (exact i32 accumulation)");
  const tfhe_hip_params &P = ctx->P;
  KeyState &k = *ctx->K;
  const size_t bytes = pke_plane_bytes(P.n, (int)size), chunks = bytes / 16;
  CHK(begin_side_key(ctx, k.pke_loaded, k.d_pke8, bytes));
  CHK(upload_through_temp(ctx, "public key", {{encryptions, size * (size_t)(P.n + 1) * 4}}, 0, [&](void *d_enc) {
    hipLaunchKernelGGL(k_pke_planes<256>, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const uint32_t *)d_enc, k.d_pke8, P.n, (int)size, chunks);
    return hipGetLastError();
  }));
  k.pke_size = (int)size;
  commit_side_key(k.pke_loaded);
  return TFHE_HIP_OK;
}

int tfhe_hip_public_key_is_loaded(tfhe_hip_ctx *ctx) { return flag_is_loaded(ctx, &KeyState::pke_loaded); }

int tfhe_hip_batch_pk_encrypt(tfhe_hip_ctx *ctx, const uint32_t *plain, size_t count, double alpha,
                              const uint8_t rng_key[32], uint64_t first_index, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_public_key(ctx));
  if (const char *why = pke_refusal(plain, count, alpha, out)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  const int rc = host_call(ctx, false, {{plain, count * 4, &ctx->a}}, out, tlwe_bytes(ctx, count), [&](const void *const *d, void *o) {
    return pke_launch(ctx, gk.k, first_index, u32(d[0]), count, alpha, (uint32_t *)o, ctx->stream);
  });
  scrub(ctx->stream, {{&ctx->a, count * 4}});  // the plaintexts do not stay behind in the staging buffer
  return rc;
}

int tfhe_hip_batch_pk_encrypt_dev(tfhe_hip_ctx *ctx, const uint32_t *plain, size_t count, double alpha,
                                  const uint8_t rng_key[32], uint64_t first_index, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_public_key(ctx));
  if (const char *why = pke_refusal(plain, count, alpha, out)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  return pke_launch(ctx, gk.k, first_index, plain, count, alpha, out, pick(ctx, stream));
}

int tfhe_hip_get_pk_encrypt_times(tfhe_hip_ctx *ctx, tfhe_hip_pk_encrypt_times *out) {
  if (!ctx || !out) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  memset(out, 0, sizeof(*out));
  CHK(hip_rc(ctx, ctx->ev_pke_sel.drain(out->selectors_ms, &out->passes)));
  return hip_rc(ctx, ctx->ev_pke_mm.drain(out->contraction_ms));
}

// ---- the asymmetric re-encryption key (proxy_reenc.rs:271-326) --------------------------------------------------
// Rows [n][t][base][n+1] into a device temporary, then the conversion tfhe_hip_load_reenc_key runs: the handle holds
// bit for bit what tfhe_hip_load_reenc_key(key_out) would build.
int tfhe_hip_gen_reenc_key_asymmetric(tfhe_hip_ctx *ctx, const uint32_t *key_from, double alpha, const uint8_t rng_key[32],
                                      uint32_t *key_out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  // validation first: a refused call leaves the handle's keys as they were
  if (!key_from) return fail(ctx, TFHE_HIP_EINVAL, "null key pointer");
  const tfhe_hip_params &P = ctx->P;
  if (P.n > kN) return fail(ctx, TFHE_HIP_EINVAL, "proxy re-encryption needs n <= N = 1024 (this parameter set's n is larger)");
  if (!(alpha >= 0.0)) return fail(ctx, TFHE_HIP_EINVAL, "negative noise parameter");
  CHK(need_public_key(ctx));
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  SecretStage sec(ctx, ctx->sym_sec, ctx->stream, (size_t)P.n * 4, true);  // key_from does not outlive the call on the device
  sec.put(key_from, (size_t)P.n * 4, 0);
  CHK(sec.land("re-encryption key generation: "));
  const uint32_t *d_from = sec.dev(0);
  CHK(begin_key_change(ctx, KEY_BUF_KSK));  // (both flags go: the buffer is shared with a cloud key's key-switching key)
  const int base = 1 << P.basebit;
  const size_t rows = (size_t)P.n * P.t * base, key_words = rows * (size_t)(P.n + 1);
  if (const hipError_t e = hipMemsetAsync(ctx->K->d_ksk, 0, ksk_bytes(P), ctx->stream))
    return fail(ctx, TFHE_HIP_EHIP, std::string("re-encryption key generation: ") + hipGetErrorString(e));
  // the temporary: the rows in the reference layout, then the selectors and addends of every row
  const size_t tmp_bytes = (key_words + pke_sel_words(rows, ctx->K->pke_size)) * 4;
  CHK(upload_through_temp(ctx, "re-encryption key generation", {}, tmp_bytes, [&](void *tmp) -> hipError_t {
    uint32_t *d_rows = (uint32_t *)tmp, *d_sel = d_rows + key_words;
    if (pke_rows_launch(ctx, gk.k, 0, rows, alpha, nullptr, d_from, d_sel, d_rows, ctx->stream) != TFHE_HIP_OK)
      return hipErrorLaunchFailure;
    if (const hipError_t e = ksk_convert_launch(ctx, d_rows, rows)) return e;
    if (key_out) return hipMemcpyAsync(key_out, d_rows, key_words * 4, hipMemcpyDeviceToHost, ctx->stream);
    return hipSuccess;
  }));
  return commit_reenc_key(ctx);
}
