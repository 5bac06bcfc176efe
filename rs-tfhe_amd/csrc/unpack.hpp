// unpack.hpp -- unpacking key switch: slots of TRLWE lv1 ciphertexts back to TLWE lv0 ciphertexts under s0.
//
// The result is normative in include/tfhe_hip.h ("unpacking key switch"): output m takes slot s (group G = s / N,
// coefficient j = s % N), the lv1 row of that slot is trlwe::sample_extract_index(trlwe_G, j) (trlwe.rs:106-120)
//
//   r[i] = a_G[j - i]  (i <= j),   r[i] = Torus::MAX - a_G[N + j - i] = ~a_G[N + j - i]  (i > j),   r[N] = b_G[j]
//
// (the reference's negation, one LSB below 0 - a: k_sample_extract does the same) and out[m] is
// trgsw::identity_key_switching(r) under the handle's cloud key.  Both steps are integer-exact.
//
// k_unpack_extract builds the rows on the device, in the lv1 scratch of the bootstrap path ([rows][N + 1] u32, whole
// 256-row groups allocated); launch_key_switch then runs over them exactly as it does behind a blind rotation, so the
// kernel choice (TFHE_HIP_KS_KERNEL, the automatic crossovers) is that path's.  A workgroup takes kUpRows consecutive
// outputs and keeps the a row of the current group in LDS (4 KiB), staged again only when the group changes: with
// slots == NULL that is once per workgroup (twice across a group boundary).  Lane L writes the 16-byte-aligned quad
// i = h + 4 L .. + 3 of its row (h: the words before the row's first aligned one -- a row is N + 1 words, so rows
// start at every alignment), a few lanes the h head words and the tail.  The LDS reads of a quad are descending
// dwords 4 apart between lanes, a 4-way bank conflict: 4 waves x 4 reads x 8 LDS cycles = 128 cycles per row against
// the ~560 clocks a CU's share of HBM bandwidth takes to write the row's 4,100 bytes -- the stores are the cost.
#pragma once
#include "internal.hpp"

namespace tfhe {

constexpr int kUpRows = 8;  // outputs per workgroup

// grid ceil(count / ROWS), WG = N / 4 lanes.  A slot >= groups * N (the *_dev forms leave the range to the caller; the
// host forms refuse it before the launch) reads nothing and leaves an all-zero row.
template <int WG, int ROWS>
__global__ __launch_bounds__(WG) void k_unpack_extract(const uint32_t *__restrict__ trlwe, size_t groups,
                                                        const uint32_t *__restrict__ slots, size_t count,
                                                        uint32_t *__restrict__ lv1) {
  static_assert(WG * 4 == kN, "a lane stages four words of the a row and stores one quad of the lv1 row");
  __shared__ uint32_t a[kN];
  const int tid = threadIdx.x;
  const size_t m0 = (size_t)blockIdx.x * ROWS, total = groups * (size_t)kN;
  size_t cur = ~(size_t)0;  // the group whose a row the LDS holds
#pragma unroll 1
  for (int r = 0; r < ROWS; ++r) {
    const size_t m = m0 + (size_t)r;
    if (m >= count) break;  // (workgroup-uniform, as is everything derived from m alone)
    const size_t s = slots ? (size_t)slots[m] : m;
    const bool ok = s < total;
    const size_t G = s / (size_t)kN;
    const int j = (int)(s % (size_t)kN);
    if (ok && G != cur) {
      __syncthreads();  // the previous row's reads are done
      const uint32_t *src = trlwe + G * (size_t)(2 * kN);
#pragma unroll
      for (int q = 0; q < 4; ++q) a[tid + WG * q] = src[tid + WG * q];
      __syncthreads();
      cur = G;
    }
    const uint32_t bj = ok ? trlwe[(G * 2 + 1) * (size_t)kN + (size_t)j] : 0u;
    auto val = [&](int i) -> uint32_t {
      if (!ok) return 0u;
      if (i == kN) return bj;
      const uint32_t v = a[(j - i) & (kN - 1)];
      return (TFHE_MUT(kMut_unpack_diag) ? i >= j : i > j) ? ~v : v;  // Torus::MAX - v
    };
    const size_t w0 = m * (size_t)(kN + 1);
    uint32_t *row = lv1 + w0;
    const int h = (int)((0 - w0) & 3);                        // head words before the first 16-byte-aligned one
    const int nq = (kN + 1 - h) >> 2, t0 = h + 4 * nq;        // aligned quads (255 or 256), first tail word
    if (tid < nq) {
      const int i = h + 4 * tid;
      *reinterpret_cast<uint4 *>(row + i) = make_uint4(val(i), val(i + 1), val(i + 2), val(i + 3));
    }
    if (tid < h) row[tid] = val(tid);
    const int tt = WG - 1 - tid;  // (the tail on the last wave: the first one has the head)
    if (t0 + tt <= kN) row[t0 + tt] = val(t0 + tt);
  }
}

}  // namespace tfhe

// ---- unpacking key switch ---------------------------------------------------------------------------------------------
namespace {
// extraction into the context's lv1 scratch, then the key switch of the bootstrap path over `count` rows
int unpack_dev(tfhe_hip_ctx *ctx, const uint32_t *trlwe, size_t groups, const uint32_t *slots, size_t count,
               uint32_t *out, hipStream_t s) {
  CHK(take(ctx, s, ctx->lv1, lv1_bytes(count)));
  uint32_t *lv1 = (uint32_t *)ctx->lv1.p;
  hipLaunchKernelGGL((k_unpack_extract<kN / 4, kUpRows>), dim3((unsigned)((count + kUpRows - 1) / kUpRows)), dim3(kN / 4), 0, s,
                     trlwe, groups, slots, count, lv1);
  CHK(launched(ctx));
  return launch_key_switch(ctx, s, lv1, out, count);
}

// the checks both forms share, in one order: key, empty batch, pointers, count against the groups
// (returns TFHE_HIP_OK with *run = false for an empty batch)
int unpack_checks(tfhe_hip_ctx *ctx, const uint32_t *trlwe, size_t groups, const uint32_t *slots, size_t count,
                  const uint32_t *out, bool *run) {
  *run = false;
  CHK(need_key(ctx));
  if (count == 0) return TFHE_HIP_OK;
  if (!trlwe || !out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  if (!slots && count > groups * (size_t)kN) return fail(ctx, TFHE_HIP_EINVAL, "count exceeds the groups * N slots of the input");
  if (slots && groups == 0) return fail(ctx, TFHE_HIP_EINVAL, "slot out of range");
  *run = true;
  return TFHE_HIP_OK;
}
}  // namespace

int tfhe_hip_batch_unpack_trlwe(tfhe_hip_ctx *ctx, const uint32_t *trlwe, size_t groups, const uint32_t *slots,
                                size_t count, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  bool run = false;
  CHK(unpack_checks(ctx, trlwe, groups, slots, count, out, &run));
  if (!run) return TFHE_HIP_OK;
  if (slots)
    for (size_t m = 0; m < count; ++m)
      if ((size_t)slots[m] >= groups * (size_t)kN) return fail(ctx, TFHE_HIP_EINVAL, "slot out of range");
  // with slots == NULL only the groups the outputs come from travel
  const size_t used = slots ? groups : (count + kN - 1) / kN;
  return host_call(ctx, false, {{trlwe, trlwe_bytes(used), &ctx->a}, {slots, count * 4, &ctx->idx}}, out, tlwe_bytes(ctx, count),
                   [&](const void *const *d, void *o) { return unpack_dev(ctx, u32(d[0]), used, u32(d[1]), count, (uint32_t *)o, ctx->stream); });
}

int tfhe_hip_batch_unpack_trlwe_dev(tfhe_hip_ctx *ctx, const uint32_t *trlwe, size_t groups, const uint32_t *slots,
                                    size_t count, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  bool run = false;
  CHK(unpack_checks(ctx, trlwe, groups, slots, count, out, &run));
  if (!run) return TFHE_HIP_OK;
  return unpack_dev(ctx, trlwe, groups, slots, count, out, pick(ctx, stream));
}
