// table.hpp -- encrypted-table key switch and the tree (bivariate) bootstrap built on it.
//
// The result is normative in include/tfhe_hip.h ("encrypted-table key switch").  m TLWE lv0 ciphertexts c_x, x < m, of
// one output become ONE TRLWE lv1 under s1 whose phase is the test vector Generator._assemble builds from their
// phases: with P_x the packing key switch of c_x alone at slot 0, W = N / m and off = W / 2,
//
//   Q = sum_x X^(x W) P_x,     out = X^(-off) (1 + X + ... + X^(W-1)) Q        (negacyclic, mod 2^32, both rows)
//
// so a blind rotation of `out` by an encrypted x selects c_x: a function of two encrypted digits from m + 1 bootstraps
// (tfhe_hip_batch_bootstrap_bivariate below).  The key, the digits and the contraction are the packing key switch's
// (packing.hpp): k_table_mfma is k_pack_mfma with rows numbered R = c m + x, read at in + (x count + c)(n+1), and another
// epilogue -- rows land W apart and in different outputs, so the anti-diagonal line does not apply.  The four byte
// planes are merged in an LDS line per ciphertext of the block, indexed by the target's distance from the ciphertext's
// first row: rows of one ciphertext whose targets col + x W coincide are summed there too.  One integer atomicAdd per
// non-zero word of the line then reaches out[c][h][(col + x W) mod N], negated past the wrap (order-free: the words
// are deterministic).  k_table_window turns Q into the windowed sum in place, one workgroup per (c, row).
//
// Every kernel here is a template: instantiations are emitted after the library's other kernels, so the code of every
// existing kernel stays byte-identical.
#pragma once
#include "packing.hpp"

namespace tfhe {

constexpr int kTbMaxM = 512;              // W = N / m >= 2: the half-box rotation off = W / 2 is at least one
constexpr int kTbLine = 32 * 32 * kPkNT;  // LDS words of a block's lines: a 32 x (32 kPkNT) tile at the most (below)

__host__ __device__ __forceinline__ int tb_log2(int m) {  // m a power of two in [2, kTbMaxM], else -1
  for (int s = 1; (1 << s) <= kTbMaxM; ++s)
    if (m == (1 << s)) return s;
  return -1;
}

// out [count][2][N]: a rows 0, b rows b_x at coefficient x W (k_table_mfma's atomics add the rest)
template <int WG>
__global__ __launch_bounds__(WG) void k_table_init(const uint32_t *__restrict__ in, size_t count, int n, int lm,
                                                    uint32_t *__restrict__ out, size_t words) {
  const size_t idx = (size_t)blockIdx.x * WG + threadIdx.x;
  if (idx >= words) return;
  const size_t c = idx / (2 * kN);
  const int rem = (int)(idx % (2 * kN));
  const int W = kN >> lm;
  uint32_t v = 0u;
  if (rem >= kN && ((rem - kN) & (W - 1)) == 0) {
    const size_t x = (size_t)((rem - kN) / W);
    v = in[(x * count + c) * (size_t)(n + 1) + n];
  }
  out[idx] = v;
}

// grid (ceil(count m / 32), kPkTiles / NT, K chunks), 4 waves: wave w = byte plane w.  out holds k_table_init's words.
// A block's 32 rows are rpc = min(m, 32) consecutive x of each of 32 / rpc ciphertexts.  Line of one ciphertext: word
// d = col + xr Wc for column col < 32 NT of the group and row xr < rpc of the ciphertext, Wc = min(W, 32 NT): for
// W <= 32 NT that is the target's distance from (first column, first row), so coinciding targets share a word; wider
// boxes cannot coincide inside a column group and keep a word each.  32 / rpc lines of 32 NT + (rpc - 1) Wc words are
// at most 32 * 32 NT words for every m.
template <int NT>
__global__ __launch_bounds__(256, 2) void k_table_mfma(const uint32_t *__restrict__ in, size_t count, int lm, int n,
                                                     int basebit, int t, const unsigned char *__restrict__ pk8,
                                                     uint32_t *__restrict__ out) {
  static_assert(32 % NT == 0, "a column group stays inside the a or the b half");
  constexpr int CG = 32 * NT;
  static_assert(32 * CG == kTbLine, "the lines of a block fit a 32 x CG tile");
  __shared__ uint32_t line[32 * CG];
  const int nib = pk_blocks(n), per = (nib + (int)gridDim.z - 1) / (int)gridDim.z;
  const int ib0 = (int)blockIdx.z * per, ib1 = ib0 + per < nib ? ib0 + per : nib;
  if (ib0 >= ib1) return;  // (workgroup-uniform) an empty K chunk
  const int tid = threadIdx.x, lane = tid & 63, kb = lane >> 5;
  const int plane = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = 1 << lm, W = kN >> lm;
  const int lr = lm < 5 ? lm : 5, rpc = 1 << lr, ncb = 32 >> lr;  // (all powers of two: shifts, no divisions)
  const int lwc = W < CG ? 10 - lm : __builtin_ctz(CG), Wc = 1 << lwc, span = CG + (rpc - 1) * Wc;
  for (int d = tid; d < ncb * span; d += 256) line[d] = 0u;
  const size_t rows = count << lm;
  const size_t row0 = (size_t)blockIdx.x * 32, row = row0 + (size_t)(lane & 31);
  const bool live = row < rows;
  const size_t rc = live ? row >> lm : 0, rx = live ? row & (size_t)(m - 1) : 0;
  const uint32_t *arow = in + (rx * count + rc) * (size_t)(n + 1);
  const int ct0 = (int)blockIdx.y * NT, S = nib * t;
  // digits: as k_pack_mfma builds them
  const int bt = basebit * t;
  const uint32_t rnd = 1u << (31 - bt), bmask = (1u << basebit) - 1u, half = 1u << (basebit - 1);
  const uint32_t btmask = (1u << bt) - 1u;
  uint32_t off = 0;
  for (int q = 0; q < t; ++q) off += half << (basebit * q);
  const uint32_t bias = (128u - half) * 0x01010101u;
  auto load_a = [&](int ib, uint32_t(&w)[16]) {
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const int i = 32 * ib + 16 * kb + b;
      w[b] = (live && i < n) ? arow[i] : 0u;  // a 0 word has all-zero digits
    }
  };
  auto round_a = [&](const uint32_t(&w)[16], uint32_t(&ap)[16]) {
#pragma unroll
    for (int b = 0; b < 16; ++b) ap[b] = (((w[b] + rnd) >> (32 - bt)) + off) & btmask;
  };
  const unsigned char *kp = pk8 + ((size_t)(plane * kPkTiles + ct0) * S) * 1024 + (size_t)lane * 16;
  const size_t tstride = (size_t)S * 1024;
  auto load_b = [&](int s, km_i32x4(&B)[NT]) {
#pragma unroll
    for (int c = 0; c < NT; ++c) B[c] = *reinterpret_cast<const km_i32x4 *>(kp + c * tstride + (size_t)s * 1024);
  };
  km_i32x16 acc[NT];
#pragma unroll
  for (int c = 0; c < NT; ++c) acc[c] = km_i32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t w[16], ap[16];
  load_a(ib0, w);
  round_a(w, ap);
  load_a(ib0 + 1, w);  // the next block's words (0 past n)
  km_i32x4 Bc[NT];
  const int s0 = ib0 * t, s1 = ib1 * t;
  load_b(s0, Bc);
  int l = 0;
#pragma unroll 1
  for (int s = s0; s < s1; ++s) {
    km_i32x4 Bn[NT];
    load_b(s + 1 < s1 ? s + 1 : s, Bn);  // one step ahead (the last step reloads its own tiles)
    const int sh = basebit * (t - 1 - l);
    km_u32x4 a;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t v = ((ap[4 * q] >> sh) & bmask) | (((ap[4 * q + 1] >> sh) & bmask) << 8) |
                         (((ap[4 * q + 2] >> sh) & bmask) << 16) | (((ap[4 * q + 3] >> sh) & bmask) << 24);
      a[q] = (v + bias) ^ 0x80808080u;
    }
    const km_i32x4 A = __builtin_bit_cast(km_i32x4, a);
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, Bc[c], acc[c], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < NT; ++c) Bc[c] = Bn[c];
    if (++l == t) {  // the next step starts block s / t + 1
      l = 0;
      round_a(w, ap);
      load_a(s / t + 2, w);
    }
  }
  __syncthreads();  // (the lines are zeroed)
  // C element e of the lane: row (e & 3) + 8 (e >> 2) + 4 kb of the block, column lane & 31 of its tile
  const uint32_t sh8 = 8u * (uint32_t)plane;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int r = (e & 3) + 8 * (e >> 2) + 4 * kb;
    uint32_t *ln = line + (r >> lr) * span + ((r & (rpc - 1)) << lwc) + (lane & 31);
#pragma unroll
    for (int c = 0; c < NT; ++c) atomicAdd(&ln[32 * c], (uint32_t)acc[c][e] << sh8);
  }
  __syncthreads();
  const int x0 = (ct0 * 32) & (kN - 1), h = ct0 >= kPkTiles / 2 ? 1 : 0;
  for (int cb = 0; cb < ncb; ++cb) {
    const size_t first = row0 + (size_t)(cb << lr);  // the ciphertext's first row of this block
    if (first >= rows) break;
    const size_t c = first >> lm;
    const int xf = (int)(first & (size_t)(m - 1));
    uint32_t *o = out + (c * 2 + (size_t)h) * (size_t)kN;
    for (int d = tid; d < span; d += 256) {
      const uint32_t v = line[cb * span + d];
      if (!v) continue;
      const int y = x0 + xf * W + d + (d >> lwc) * (W - Wc);  // col + x W < 2N
      if (y < kN) atomicAdd(&o[y], 0u - v);  // A = -sum, B = sum_x b_x X^(x W) - sum
      else atomicAdd(&o[y - kN], v);         // X^y = -X^(y - N)
    }
  }
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
  const uint4 v = reinterpret_cast<const uint4 *>(q)[tid];
  const uint32_t p0 = v.x, p1 = p0 + v.y, p2 = p1 + v.z, p3 = p2 + v.w;
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
  uint32_t r[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int hi = 4 * tid + e + off, lo = hi - W;
    if (lo < 0) r[e] = S[hi] - (total - S[lo + kN]);
    else if (hi >= kN) r[e] = total - S[lo] - S[hi - kN];
    else r[e] = S[hi] - S[lo];
  }
  reinterpret_cast<uint4 *>(q)[tid] = make_uint4(r[0], r[1], r[2], r[3]);
}

}  // namespace tfhe

// ---- encrypted-table key switch ---------------------------------------------------------------------------------
namespace {
// in [m][count][n+1] -> out [count][2][N] on stream s (arguments checked by the callers)
int table_launch(tfhe_hip_ctx *ctx, const uint32_t *in, int m, size_t count, uint32_t *out, hipStream_t s) {
  const tfhe_hip_params &P = ctx->P;
  const int lm = tb_log2(m);
  const size_t words = count * 2 * kN, rows = count << lm;
  hipLaunchKernelGGL(k_table_init<256>, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, in, count, P.n, lm, out, words);
  CHK(launched(ctx));
  const size_t rblocks = (rows + 31) / 32;
  hipLaunchKernelGGL(k_table_mfma<kPkNT>, dim3((unsigned)rblocks, kPkTiles / kPkNT, (unsigned)pack_kchunks(ctx, rblocks)),
                     dim3(256), 0, s, in, count, lm, P.n, P.basebit, P.t, (const unsigned char *)ctx->K->d_pk8, out);
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

// a scratch of the composite: exactly `bytes` (ensure() over-allocates by a quarter, which the bound above excludes)
int biv_ensure(tfhe_hip_ctx *ctx, DevBuf &b, size_t bytes) {
  if (bytes <= b.cap) return TFHE_HIP_OK;
  if (b.p) HIPCHK(ctx, hipFree(b.p));
  b.p = nullptr;
  b.cap = 0;
  const hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) {
    b.p = nullptr;
    return fail(ctx, TFHE_HIP_ENOMEM, std::string("hipMalloc (bivariate scratch): ") + hipGetErrorString(e));
  }
  b.cap = bytes;
  return TFHE_HIP_OK;
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

// device pointers, keys and arguments checked: m / k many-LUT bootstraps of y, the table build, the bootstrap of x
int bivariate_launch(tfhe_hip_ctx *ctx, const uint32_t *x, const uint32_t *y, const uint32_t *testvecs, int m, int k,
                     bool keyswitch, uint32_t *out, size_t count, hipStream_t s) {
  const size_t w = (size_t)(ctx->P.n + 1), chunk0 = biv_chunk(ctx, m), first = count < chunk0 ? count : chunk0;
  CHK(claim_scratch(ctx, s));
  CHK(biv_ensure(ctx, ctx->biv_s1, (size_t)m * first * w * 4));
  CHK(biv_ensure(ctx, ctx->biv_tv, trlwe_bytes(first)));
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

// the pool form: the batch is cut by count over the members, the tables go whole to each (every member holds both keys)
int tfhe_hip_pool_batch_bootstrap_bivariate(tfhe_hip_pool *p, const uint32_t *x, const uint32_t *y, const uint32_t *testvecs,
                                            int m, int n_luts, int keyswitch, uint32_t *out, size_t count) {
  if (!p) return TFHE_HIP_EINVAL;
  std::lock_guard<FairMutex> plk(p->root()->own_mu);
  // a member's checks of the keys and of m, n_luts and the tables, in a context's order (count 0: nothing runs)
  CHK(pool_member_rc(p, p->ctxs[0], tfhe_hip_batch_bootstrap_bivariate(p->ctxs[0], x, y, testvecs, m, n_luts, keyswitch, out, 0)));
  if (count == 0) return TFHE_HIP_OK;
  if (const char *why = bivariate_refusal(x, y, testvecs, m, n_luts, out, count)) return pool_fail(p, TFHE_HIP_EINVAL, why);
  const size_t w = pool_tlwe_bytes(p);
  return pool_map(p, count, [&](tfhe_hip_ctx *c, size_t lo, size_t hi) {
    const size_t words = lo * (w / 4);
    return tfhe_hip_batch_bootstrap_bivariate(c, x + words, y + words, testvecs, m, n_luts, keyswitch, out + words, hi - lo);
  });
}
