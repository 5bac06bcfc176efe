// table.hpp -- encrypted-table key switch and the tree (bivariate) bootstrap built on it.
//
// The result is normative in include/tfhe_hip.h ("encrypted-table key switch").  m TLWE lv0 ciphertexts c_x, x < m, of
// one output become ONE TRLWE lv1 under s1 whose phase is the test vector Generator._assemble builds from their
// phases: with P_x the packing key switch of c_x alone at slot 0, W = N / m and off = W / 2,
//
//   Q = sum_x X^(x W) P_x,     out = X^(-off) (1 + X + ... + X^(W-1)) Q        (negacyclic, mod 2^32, both rows)
//
// so a blind rotation of `out` by an encrypted x selects c_x: a function of two encrypted digits from m + 1 bootstraps
// (tfhe_hip_batch_bootstrap_bivariate below).  The key, the digits, the contraction and its kernel are the packing key
// switch's (packing.hpp, k_box_mfma): packing is this key switch at m = N, where the box width is W = 1 and the input
// is read row-major.  Here rows are numbered R = c m + x and read at in + (x count + c)(n+1); they land W apart and in
// different outputs.  The four byte planes are merged in an LDS line per ciphertext of the block, indexed by the
// target's distance from the ciphertext's first row: rows of one ciphertext whose targets col + x W coincide are
// summed there too.  One integer atomicAdd per non-zero word of the line then reaches out[c][h][(col + x W) mod N],
// negated past the wrap (order-free: the words are deterministic).  k_table_window turns Q into the windowed sum in
// place, one workgroup per (c, row).
#pragma once
#include "packing.hpp"

namespace tfhe {

constexpr int kTbMaxM = 512;  // W = N / m >= 2: the half-box rotation off = W / 2 is at least one

__host__ __device__ __forceinline__ int tb_log2(int m) {  // m a power of two in [2, kTbMaxM], else -1
  for (int s = 1; (1 << s) <= kTbMaxM; ++s)
    if (m == (1 << s)) return s;
  return -1;
}

// One workgroup per (c, row): out[y] = sum_{r < W} Q~[y + off - r] in place, Q~ the negacyclic extension.  With the
// wrapping prefix sums S[i] = Q[0] + ... + Q[i] and hi = y + off, lo = hi - W:
//   0 <= lo, hi < N:  S[hi] - S[lo]
//   lo < 0:           S[hi] - (S[N-1] - S[lo + N])          (the terms below 0 are -Q[i + N])
//   hi >= N:          S[N-1] - S[lo] - S[hi - N]            (the terms from N on are -Q[i - N])
template <int WG>
__global__ __launch_bounds__(WG) void k_table_window(uint32_t *__restrict__ out, int lm) {
  static_assert(WG * 4 == kN, "four words a lane");
  __shared__ uint32_t S[kN];
  __shared__ uint32_t part[WG];
  uint32_t *q = out + (size_t)blockIdx.x * kN;
  const int tid = threadIdx.x;
  // out is the caller's: word by word (a wave reads 256 consecutive bytes), through S to the lane that sums words
  // 4 tid .. 4 tid + 3 -- no 16-byte access whose alignment would be taken from the index
#pragma unroll
  for (int e = 0; e < 4; ++e) S[tid + WG * e] = q[tid + WG * e];
  __syncthreads();
  const uint32_t p0 = S[4 * tid], p1 = p0 + S[4 * tid + 1], p2 = p1 + S[4 * tid + 2], p3 = p2 + S[4 * tid + 3];
  part[tid] = p3;
  __syncthreads();
  for (int d = 1; d < WG; d <<= 1) {  // inclusive scan of the lanes' sums
    const uint32_t add = tid >= d ? part[tid - d] : 0u;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  const uint32_t base = tid ? part[tid - 1] : 0u;
  S[4 * tid] = base + p0;
  S[4 * tid + 1] = base + p1;
  S[4 * tid + 2] = base + p2;
  S[4 * tid + 3] = base + p3;
  __syncthreads();
  const int W = kN >> lm, off = W >> 1;
  const uint32_t total = S[kN - 1];
#pragma unroll
  for (int e = 0; e < 4; ++e) {  // coefficient y = tid + WG e: consecutive lanes store consecutive words
    const int y = tid + WG * e, hi = y + off, lo = hi - W;
    uint32_t r;
    if (lo < 0) r = S[hi] - (total - S[lo + kN]);
    else if (hi >= kN) r = total - S[lo] - S[hi - kN];
    else r = S[hi] - S[lo];
    q[y] = r;
  }
}

}  // namespace tfhe

// ---- encrypted-table key switch ---------------------------------------------------------------------------------
namespace {
// in [m][count][n+1] -> out [count][2][N] on stream s (arguments checked by the callers)
int table_launch(tfhe_hip_ctx *ctx, const uint32_t *in, int m, size_t count, uint32_t *out, hipStream_t s) {
  const tfhe_hip_params &P = ctx->P;
  const int lm = tb_log2(m);
  const size_t words = count * 2 * kN, rows = count << lm;
  hipLaunchKernelGGL(k_box_init<256>, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, in, rows, lm, count, (size_t)1,
                     P.n, out, words);
  CHK(launched(ctx));
  const size_t rblocks = (rows + 31) / 32;
  hipLaunchKernelGGL((k_box_mfma<kPkNT, kBoxLmArg>), dim3((unsigned)rblocks, kPkTiles / kPkNT, (unsigned)pack_kchunks(ctx, rblocks)),
                     dim3(256), 0, s, in, rows, lm, count, (size_t)1, P.n, P.basebit, P.t,
                     (const unsigned char *)ctx->K->d_pk8, out);
  CHK(launched(ctx));
  hipLaunchKernelGGL(k_table_window<256>, dim3((unsigned)(count * 2)), dim3(256), 0, s, out, lm);
  return launched(ctx);
}

const char *table_refusal(const uint32_t *in, int m, size_t count, const uint32_t *out) {
  if (tb_log2(m) < 0) return "m must be a power of two in [2, 512]";
  if (count && (!in || !out)) return "null pointer";
  if (count > (0x7FFFFFFFull >> tb_log2(m))) return "m * count too large";
  return nullptr;
}
}  // namespace

int tfhe_hip_batch_pack_table(tfhe_hip_ctx *ctx, const uint32_t *in, int m, size_t count, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_packing_key(ctx));
  if (const char *why = table_refusal(in, m, count, out)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  return host_call(ctx, false, {{in, (size_t)m * count * (size_t)(ctx->P.n + 1) * 4, &ctx->a}}, out, count * 2 * kN * 4,
                   [&](const void *const *d, void *o) { return table_launch(ctx, u32(d[0]), m, count, (uint32_t *)o, ctx->stream); });
}

int tfhe_hip_batch_pack_table_dev(tfhe_hip_ctx *ctx, const uint32_t *in, int m, size_t count, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_packing_key(ctx));
  if (const char *why = table_refusal(in, m, count, out)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  return table_launch(ctx, in, m, count, out, pick(ctx, stream));
}

// ---- tree bootstrap: any function of two encrypted digits ---------------------------------------------------------
namespace {
constexpr size_t kBivScratchBytes = (size_t)256 << 20;  // the stage-1 scratch [m][chunk][n+1] never grows past this

// a scratch of the composite: exactly `bytes` (the quarter of slack is what the bound above excludes)
int biv_take(tfhe_hip_ctx *ctx, hipStream_t s, ScratchBuf &b, size_t bytes) {
  return take(ctx, s, b, bytes, true, "hipMalloc (bivariate scratch): ");
}

// ciphertexts per pass: what the stage-1 scratch bound allows, lowered by TFHE_HIP_BIVARIATE_CHUNK (read at every call: tests)
size_t biv_chunk(const tfhe_hip_ctx *ctx, int m) {
  const size_t row = (size_t)m * (size_t)(ctx->P.n + 1) * 4;
  size_t chunk = kBivScratchBytes / row;  // >= 1: m (n+1) 4 is far below the bound
  if (const char *env = getenv("TFHE_HIP_BIVARIATE_CHUNK")) {
    const long v = atol(env);
    if (v > 0 && (size_t)v < chunk) chunk = (size_t)v;
  }
  return chunk;
}

}  // namespace

// (declared in internal.hpp: the pool form of pool.hpp runs the same checks)
const char *bivariate_refusal(const uint32_t *x, const uint32_t *y, const uint32_t *testvecs, int m, int n_luts,
                              const uint32_t *out, size_t count) {
  if (tb_log2(m) < 0) return "m must be a power of two in [2, 512]";
  if (lut_shift_of(n_luts) < 0) return "n_luts must be 1, 2, 4 or 8";
  if (n_luts > m) return "n_luts must not exceed m";
  if (!testvecs) return "bivariate bootstrap needs its tables";
  if (count && (!x || !y || !out)) return "null pointer";
  if (count > (0x7FFFFFFFull >> tb_log2(m))) return "m * count too large";
  return nullptr;
}

namespace {
// device pointers, keys and arguments checked: m / k many-LUT bootstraps of y, the table build, the bootstrap of x
int bivariate_launch(tfhe_hip_ctx *ctx, const uint32_t *x, const uint32_t *y, const uint32_t *testvecs, int m, int k,
                     bool keyswitch, uint32_t *out, size_t count, hipStream_t s) {
  const size_t w = (size_t)(ctx->P.n + 1), chunk0 = biv_chunk(ctx, m), first = count < chunk0 ? count : chunk0;
  CHK(biv_take(ctx, s, ctx->biv_s1, (size_t)m * first * w * 4));
  CHK(biv_take(ctx, s, ctx->biv_tv, trlwe_bytes(first)));
  uint32_t *S = (uint32_t *)ctx->biv_s1.p, *T = (uint32_t *)ctx->biv_tv.p;
  for (size_t lo = 0; lo < count; lo += chunk0) {
    const size_t cc = count - lo < chunk0 ? count - lo : chunk0;
    for (int j = 0; j < m / k; ++j)  // S[j k + r][c]: output r of table j, function-major
      CHK(run_bootstrap(ctx, s, {.in_a = y + lo * w, .testvec = testvecs + (size_t)j * 2 * kN, .count = cc, .lut_shift = lut_shift_of(k)},
                        S + (size_t)j * k * cc * w, true));
    CHK(table_launch(ctx, S, m, cc, T, s));
    CHK(run_bootstrap(ctx, s, {.in_a = x + lo * w, .testvec = T, .per_ct = 1, .count = cc}, out + lo * w, keyswitch));
  }
  return TFHE_HIP_OK;
}
}  // namespace

int tfhe_hip_batch_bootstrap_bivariate(tfhe_hip_ctx *ctx, const uint32_t *x, const uint32_t *y, const uint32_t *testvecs,
                                       int m, int n_luts, int keyswitch, uint32_t *out, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_key(ctx));
  CHK(need_packing_key(ctx));
  if (const char *why = bivariate_refusal(x, y, testvecs, m, n_luts, out, count)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  const size_t bytes = tlwe_bytes(ctx, count);
  const HostIn in[] = {{x, bytes, &ctx->a}, {y, bytes, &ctx->b}, {testvecs, trlwe_bytes((size_t)(m / n_luts)), &ctx->tv}};
  return host_call(ctx, false, in, out, bytes, [&](const void *const *d, void *o) {
    return bivariate_launch(ctx, u32(d[0]), u32(d[1]), u32(d[2]), m, n_luts, keyswitch != 0, (uint32_t *)o, count, ctx->stream);
  });
}

int tfhe_hip_batch_bootstrap_bivariate_dev(tfhe_hip_ctx *ctx, const uint32_t *x, const uint32_t *y,
                                           const uint32_t *testvecs, int m, int n_luts, int keyswitch, uint32_t *out,
                                           size_t count, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_key(ctx));
  CHK(need_packing_key(ctx));
  if (const char *why = bivariate_refusal(x, y, testvecs, m, n_luts, out, count)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  return bivariate_launch(ctx, x, y, testvecs, m, n_luts, keyswitch != 0, out, count, pick(ctx, stream));
}
