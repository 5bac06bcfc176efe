// packing.hpp -- packing key switch: up to N = 1024 TLWE lv0 results in ONE TRLWE lv1 under s1.
//
// The format and the result are normative in include/tfhe_hip.h ("packing key switch").  For a group of inputs
// c_j = (a_j, b_j), j < N, with d_l(x) the signed digits of the identity key switch's rounding of x:
//
//   A = - sum_{i,l} D_{i,l} (*) a_{i,l},   B = sum_j b_j X^j - sum_{i,l} D_{i,l} (*) b_{i,l},   D_{i,l} = sum_j d_l(a_j[i]) X^j
//
// computed as ONE integer contraction P[j][x] = sum_{(i,l)} d_l(a_j[i]) * K[(i,l)][x] over the 2N columns of the key
// rows (a row, then b row), followed by the rotate-and-sum out[x + j] += P[j][x] (negacyclic: a term past N changes
// sign).  The u32 key words are split ONCE, at load, into four balanced signed byte planes (ks_plane_byte of
// key_switch_mfma.hpp), so every plane is an exact i8 x i8 -> i32 matrix-core product: |d| <= B/2 <= 64, so
// |acc| <= n t (B/2) 128 < 2^25 on every supported set (< 2^21 on SECURITY_128_BIT), and sum_p acc_p << 8p wraps to
// the u32 result -- equal word for word, not approximately.
//
// The byte-plane K-walk, shared by the three contractions of this shape -- the packing key switch, the encrypted-table
// key switch (table.hpp) and the public-key subset sum (pk_encrypt.hpp): a workgroup is 4 waves = the 4 byte planes of
// ONE (32-row block, NT-tile column group, K chunk).  The planes are laid out [plane][column tile][step][lane][16 B]
// (k_pack_planes, k_pke_planes): a tile of a step is one contiguous KiB, read straight into registers one step ahead of
// its matrix instructions (plane_walk); the A fragment of a step comes from the caller (PackDigits here, the selector
// words there); plane_merge adds every accumulator, shifted by its plane, into LDS words the caller addresses by row.
//
// k_box_mfma is both key switches.  The K axis runs over steps s = ib * t + l (ib: the 32 coefficients
// i = 32 ib + 16 kb + byte, l: the digit position), so a lane keeps its 16 rounded a-words of block ib in registers and
// builds the t digit fragments of the block from them by shifts (PackDigits).  Row R of a launch is entry x = R mod m of
// ciphertext c = R / m, and its product lands at coefficient x W of output c, W = N / m the box width.  The packing key
// switch is the table key switch at m = N: W = 1, c the group, x the slot j, the input read row-major, and the LDS
// line indexed by the target's distance from the block's first -- the anti-diagonals x + j of the 32 x 32 tiles, the
// group's kPkNT tiles side by side.  The packing launch is the instantiation with m fixed at compile time (its shifts
// fold and its LDS is the one line; one group of 1,024 measured 4 us slower with m at run time), the table launch the
// one that takes m as an argument: one source.  The line is merged into the output with integer atomics (order-free:
// the words are deterministic).  Small batches cut K over workgroups (blockIdx.z), merged the same way.
#pragma once
#include "internal.hpp"

namespace tfhe {

constexpr int kPkTiles = 2 * kN / 32;            // 32-column tiles of a key row: a = 0..31, b = 32..63
constexpr int kPkNT = 8;                         // tiles per wave (divides 32: a column group never straddles a and b)
constexpr int kPkMaxBasebit = 7;                 // digits in [-64, 64): one signed byte

__host__ __device__ __forceinline__ int pk_blocks(int n) { return (n + 31) / 32; }         // 32-coefficient blocks
__host__ __device__ __forceinline__ int pk_steps(int n, int t) { return pk_blocks(n) * t; }  // K-steps of 32
__host__ __device__ __forceinline__ size_t pk_plane_bytes(int n, int t) {
  return (size_t)4 * kPkTiles * pk_steps(n, t) * 1024;
}

// Key rows r = i t + l as [n t][2][N] u32: a from the keystream (r, 24, "PKS") under the mask seed, b from `bodies`.
// One wave per row; lane q makes keystream block q (coefficients 16q .. 16q+15).
__global__ __launch_bounds__(64) void k_pack_expand_key(const uint32_t *__restrict__ bodies, uint32_t *__restrict__ rows,
                                                         ChaChaKey seed) {
  const uint32_t r = blockIdx.x;
  const int lane = threadIdx.x;
  uint32_t w[16];
  chacha20_block(seed, (uint32_t)lane, r, kStreamPackMask, kSeedDomainPack, w);
  uint4 *dst = reinterpret_cast<uint4 *>(rows + (size_t)r * 2 * kN + 16 * lane);
#pragma unroll
  for (int q = 0; q < 4; ++q) dst[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  const uint4 *src = reinterpret_cast<const uint4 *>(bodies + (size_t)r * kN + 16 * lane);
  uint4 *dstb = reinterpret_cast<uint4 *>(rows + (size_t)r * 2 * kN + kN + 16 * lane);
#pragma unroll
  for (int q = 0; q < 4; ++q) dstb[q] = src[q];
}

// [n t][2N] u32 -> byte planes [plane p][tile ct][step s][lane][16 B]: lane = (column 32 ct + (lane & 31), kb = lane >> 5),
// byte b = plane byte p of key row (i = 32 ib + 16 kb + b, l) at that column, s = ib t + l; 0 for i >= n.
template <int WG>
__global__ __launch_bounds__(WG) void k_pack_planes(const uint32_t *__restrict__ rows, unsigned char *__restrict__ out,
                                                     int n, int t, size_t chunks) {
  const size_t idx = (size_t)blockIdx.x * WG + threadIdx.x;
  if (idx >= chunks) return;
  const int lane = (int)(idx & 63);
  size_t r = idx >> 6;
  const int S = pk_steps(n, t);
  const int s = (int)(r % (size_t)S);
  r /= (size_t)S;
  const int ct = (int)(r % kPkTiles), p = (int)(r / kPkTiles);
  const int col = ct * 32 + (lane & 31), kb = lane >> 5;
  const int ib = s / t, l = s % t;
  reinterpret_cast<uint4 *>(out)[idx] = ks_plane_fragment(p, [=](int q, int e) {
    const int i = 32 * ib + 16 * kb + 4 * q + e;
    return i < n ? rows[((size_t)i * t + l) * 2 * kN + col] : 0u;
  });
}

// The B side and the matrix instructions of a workgroup's walk over K-steps [s0, s1): kp is the lane's 16 bytes of the
// plane's first tile at step 0, tstride the bytes between column tiles.  Every step takes the A fragment frag(s) --
// called once per step, in ascending order; it may carry state --, issues the NT matrix instructions on the tiles
// loaded a step ago, and reloads each tile register for the next step (the last step reloads its own tiles) behind the
// instruction that read it.  One register set, not two: that is where the compiler put the loads of a second set
// anyway, and with a second set live across frag's block step the kernel spills.
template <int NT, class Frag>
__device__ __forceinline__ void plane_walk(const unsigned char *kp, size_t tstride, int s0, int s1, Frag &&frag,
                                           km_i32x16 (&acc)[NT]) {
  auto load_b = [&](int s, km_i32x4(&B)[NT]) {
#pragma unroll
    for (int c = 0; c < NT; ++c) B[c] = *reinterpret_cast<const km_i32x4 *>(kp + c * tstride + (size_t)s * 1024);
  };
#pragma unroll
  for (int c = 0; c < NT; ++c) acc[c] = km_i32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  km_i32x4 Bc[NT];
  load_b(s0, Bc);
#pragma unroll 1
  for (int s = s0; s < s1; ++s) {
    const km_i32x4 A = frag(s);
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, Bc[c], acc[c], 0, 0, 0);
    load_b(s + 1 < s1 ? s + 1 : s, Bc);
  }
}

// acc[c][e] << 8 plane into base(r)[32 c + (lane & 31)]: C element e of the lane is row r = (e & 3) + 8 (e >> 2) + 4 kb
// of the block, column lane & 31 of tile c.  The four waves of a workgroup meet in the same LDS words.
template <int NT, class Base>
__device__ __forceinline__ void plane_merge(const km_i32x16 (&acc)[NT], int plane, int lane, Base &&base) {
  const uint32_t sh8 = 8u * (uint32_t)plane;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    uint32_t *ln = base((e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)) + (lane & 31);
#pragma unroll
    for (int c = 0; c < NT; ++c) atomicAdd(&ln[32 * c], (uint32_t)acc[c][e] << sh8);
  }
}

// A lane's signed-digit fragments of one input row, step after step from block ib0 on: the call for step s = ib t + l
// returns digits l of the coefficients i = 32 ib + 16 kb + b, b < 16, as 16 signed bytes.
// a_bar = (a + 2^(31 - bt)) >> (32 - bt); adding B/2 at every digit position (off) turns the plain base-B digits of
// (a_bar + off) mod 2^bt into the signed ones of the definition (carries included): d = digit - B/2.  The subtraction
// is done on four bytes at once: bytes u < B <= 128, so (u + 128 - B/2) ^ 0x80 = (u - B/2) as an i8 (bias).
// ap holds the rounded words of the current block, w the raw words of the next (0 past n and on a dead row: a 0 word
// has all-zero digits); at l == t the next block is rounded and the one after is loaded.
struct PackDigits {
  const uint32_t *arow;
  bool live;
  int n, basebit, t, kb, l, ib;  // ib: the block w holds
  uint32_t rnd, off, btmask, bias, ap[16], w[16];

  __device__ __forceinline__ PackDigits(const uint32_t *arow, bool live, int n, int basebit, int t, int kb, int ib0)
      : arow(arow), live(live), n(n), basebit(basebit), t(t), kb(kb), l(0), ib(ib0) {
    const int bt = basebit * t;
    const uint32_t half = 1u << (basebit - 1);
    rnd = 1u << (31 - bt);
    btmask = (1u << bt) - 1u;
    off = 0;
    for (int q = 0; q < t; ++q) off += half << (basebit * q);
    bias = (128u - half) * 0x01010101u;
    load();
    next_block();
  }
  __device__ __forceinline__ void load() {
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const int i = 32 * ib + 16 * kb + b;
      w[b] = (live && i < n) ? arow[i] : 0u;
    }
  }
  __device__ __forceinline__ void next_block() {
    const int bt = basebit * t;
#pragma unroll
    for (int b = 0; b < 16; ++b) ap[b] = (((w[b] + rnd) >> (32 - bt)) + off) & btmask;
    ++ib;
    load();
  }
  __device__ __forceinline__ km_i32x4 operator()(int) {
    const int sh = basebit * (t - 1 - l);
    const uint32_t bmask = (1u << basebit) - 1u;
    km_u32x4 a;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t v = ((ap[4 * q] >> sh) & bmask) | (((ap[4 * q + 1] >> sh) & bmask) << 8) |
                         (((ap[4 * q + 2] >> sh) & bmask) << 16) | (((ap[4 * q + 3] >> sh) & bmask) << 24);
      a[q] = (v + bias) ^ 0x80808080u;
    }
    if (++l == t) {  // the next step starts the next block
      l = 0;
      next_block();
    }
    return __builtin_bit_cast(km_i32x4, a);
  }
};

constexpr int kBoxLmArg = -1;              // k_box_mfma's LM: log2 m is the run-time argument
constexpr int kBoxLine = 32 * 32 * kPkNT;  // LDS words of a block's lines: a 32 x (32 kPkNT) tile at the most (below)

// The input map of a launch: row R < rows is entry rx = R & (m - 1) of ciphertext rc = R >> lm, m = 2^lm, read at
// in + (rx xs + rc cs)(n + 1).  Table: lm = log2 m, rows = count m, xs = count, cs = 1 (in is [m][count][n+1]).
// Packing: lm = 10, rows = count, xs = 1, cs = N (in is [count][n+1]; the last group may be partial).
//
// out [ceil(rows / m)][2][N]: a rows 0, b rows b_x at coefficient x W (k_box_mfma's atomics add the rest)
template <int WG>
__global__ __launch_bounds__(WG) void k_box_init(const uint32_t *__restrict__ in, size_t rows, int lm, size_t xs,
                                                  size_t cs, int n, uint32_t *__restrict__ out, size_t words) {
  const size_t idx = (size_t)blockIdx.x * WG + threadIdx.x;
  if (idx >= words) return;
  const size_t c = idx / (2 * kN);
  const int rem = (int)(idx % (2 * kN));
  const int W = kN >> lm;
  uint32_t v = 0u;
  if (rem >= kN && ((rem - kN) & (W - 1)) == 0) {
    const size_t x = (size_t)((rem - kN) >> (10 - lm));
    if ((c << lm) + x < rows) v = in[(x * xs + c * cs) * (size_t)(n + 1) + n];
  }
  out[idx] = v;
}

// grid (ceil(rows / 32), kPkTiles / NT, K chunks), 4 waves: wave w = byte plane w.  out holds k_box_init's words.
// A block's 32 rows are rpc = min(m, 32) consecutive x of each of 32 / rpc ciphertexts.  Line of one ciphertext: word
// d = col + xr Wc for column col < 32 NT of the group and row xr < rpc of the ciphertext, Wc = min(W, 32 NT): for
// W <= 32 NT that is the target's distance from (first column, first row), so coinciding targets share a word; wider
// boxes cannot coincide inside a column group and keep a word each.  32 / rpc lines of 32 NT + (rpc - 1) Wc words are
// at most 32 * 32 NT words for every m (one line of 32 NT + 31 at W = 1).
// Two workgroups per CU (at most 256 registers a lane, no spill): 5.8 against 7.6 ms for 65,536 SECURITY_128_BIT
// results at one (profiles/packing_bench.json).
// LM: log2 m known at compile time (10, the packing launch: the shifts fold and the one line is 32 NT + 31 words), or
// kBoxLmArg for the argument lm_arg (the table launch).
template <int NT, int LM>
__global__ __launch_bounds__(256, 2) void k_box_mfma(const uint32_t *__restrict__ in, size_t rows, int lm_arg, size_t xs,
                                                   size_t cs, int n, int basebit, int t,
                                                   const unsigned char *__restrict__ pk8, uint32_t *__restrict__ out) {
  static_assert(32 % NT == 0, "a column group stays inside the a or the b half");
  static_assert(LM == 10 || LM == kBoxLmArg, "the line is sized for W = 1 or for any m");
  constexpr int CG = 32 * NT;
  static_assert(32 * CG == kBoxLine, "the lines of a block fit a 32 x CG tile");
  __shared__ uint32_t line[LM == 10 ? CG + 31 : 32 * CG];
  const int lm = LM == kBoxLmArg ? lm_arg : LM;
  const int nib = pk_blocks(n), per = (nib + (int)gridDim.z - 1) / (int)gridDim.z;
  const int ib0 = (int)blockIdx.z * per, ib1 = ib0 + per < nib ? ib0 + per : nib;
  if (ib0 >= ib1) return;  // (workgroup-uniform) an empty K chunk
  const int tid = threadIdx.x, lane = tid & 63;
  const int plane = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = 1 << lm, W = kN >> lm;
  const int lr = lm < 5 ? lm : 5, rpc = 1 << lr, ncb = 32 >> lr;  // (all powers of two: shifts, no divisions)
  const int lwc = W < CG ? 10 - lm : __builtin_ctz(CG), Wc = 1 << lwc, span = CG + (rpc - 1) * Wc;
  for (int d = tid; d < ncb * span; d += 256) line[d] = 0u;
  const size_t row0 = (size_t)blockIdx.x * 32, row = row0 + (size_t)(lane & 31);
  const bool live = row < rows;
  const size_t rc = live ? row >> lm : 0, rx = live ? row & (size_t)(m - 1) : 0;
  const int ct0 = (int)blockIdx.y * NT, S = nib * t;
  km_i32x16 acc[NT];
  plane_walk<NT>(pk8 + ((size_t)(plane * kPkTiles + ct0) * S) * 1024 + (size_t)lane * 16, (size_t)S * 1024, ib0 * t, ib1 * t,
                 PackDigits(in + (rx * xs + rc * cs) * (size_t)(n + 1), live, n, basebit, t, lane >> 5, ib0), acc);
  __syncthreads();  // (the lines are zeroed)
  plane_merge<NT>(acc, plane, lane, [&](int r) { return line + (r >> lr) * span + ((r & (rpc - 1)) << lwc); });
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

}  // namespace tfhe

// ---- packing key switch (packing.hpp) -------------------------------------------------------------------------
namespace {
bool packing_supported(const tfhe_hip_params *p) { return params_supported(p) && p->basebit <= kPkMaxBasebit; }
const char *const kPackingRefusal = "packing needs basebit <= 7 (digits in one byte)";
}  // namespace

int tfhe_hip_packing_key_words(const tfhe_hip_params *params, size_t *body_words) {
  if (!params || !body_words || !packing_supported(params)) return TFHE_HIP_EINVAL;
  *body_words = (size_t)params->n * params->t * kN;
  return TFHE_HIP_OK;
}

namespace {
int need_packing_key(tfhe_hip_ctx *ctx) {
  if (!ctx->K->pk_loaded) return fail(ctx, TFHE_HIP_ENOKEY, "packing key not loaded");
  return TFHE_HIP_OK;
}

// K chunks of one launch: enough workgroups for every CU four times over, at most one chunk per coefficient block
int pack_kchunks(const tfhe_hip_ctx *ctx, size_t rblocks) {
  const size_t wgs = rblocks * (size_t)(kPkTiles / kPkNT), want = (size_t)(ctx->num_cus > 0 ? ctx->num_cus : 256) * 4;
  const int nib = pk_blocks(ctx->P.n);
  if (wgs >= want) return 1;
  const size_t k = (want + wgs - 1) / wgs;
  return k < (size_t)nib ? (int)k : nib;
}

// in [count][n+1] -> out [ceil(count / N)][2][N] on stream s: the box launch at W = 1 (m = N), the input row-major
int pack_launch(tfhe_hip_ctx *ctx, const uint32_t *in, size_t count, uint32_t *out, hipStream_t s) {
  const tfhe_hip_params &P = ctx->P;
  const size_t groups = (count + kN - 1) / kN, words = groups * 2 * kN;
  hipLaunchKernelGGL(k_box_init<256>, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, in, count, 10, (size_t)1,
                     (size_t)kN, P.n, out, words);
  CHK(launched(ctx));
  const size_t rblocks = (count + 31) / 32;
  hipLaunchKernelGGL((k_box_mfma<kPkNT, 10>), dim3((unsigned)rblocks, kPkTiles / kPkNT, (unsigned)pack_kchunks(ctx, rblocks)),
                     dim3(256), 0, s, in, count, 10, (size_t)1, (size_t)kN, P.n, P.basebit, P.t,
                     (const unsigned char *)ctx->K->d_pk8, out);
  return launched(ctx);
}
}  // namespace

int tfhe_hip_load_packing_key(tfhe_hip_ctx *ctx, const uint8_t mask_seed[32], const uint32_t *bodies) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (!mask_seed || !bodies) return fail(ctx, TFHE_HIP_EINVAL, "null key pointer");
  const tfhe_hip_params &P = ctx->P;
  if (!packing_supported(&P)) return fail(ctx, TFHE_HIP_EINVAL, kPackingRefusal);
  KeyState &k = *ctx->K;
  CHK(begin_side_key(ctx, k.pk_loaded, k.d_pk8, pk_plane_bytes(P.n, P.t)));
  const size_t rows = (size_t)P.n * P.t, body_words = rows * kN;
  const size_t chunks = pk_plane_bytes(P.n, P.t) / 16;
  // the temporary: bodies [n t][N], then the rows [n t][2][N]
  CHK(upload_through_temp(ctx, "packing key", {{bodies, body_words * 4}}, rows * 2 * kN * 4, [&](void *tmp) {
    uint32_t *d_tmp = (uint32_t *)tmp;
    hipLaunchKernelGGL(k_pack_expand_key, dim3((unsigned)rows), dim3(64), 0, ctx->stream, d_tmp, d_tmp + body_words,
                       seed_key(mask_seed));
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_pack_planes<256>, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, ctx->stream,
                       d_tmp + body_words, k.d_pk8, P.n, P.t, chunks);
    return hipGetLastError();
  }));
  commit_side_key(k.pk_loaded);
  return TFHE_HIP_OK;
}

int tfhe_hip_packing_key_is_loaded(tfhe_hip_ctx *ctx) { return flag_is_loaded(ctx, &KeyState::pk_loaded); }

int tfhe_hip_batch_pack_tlwe(tfhe_hip_ctx *ctx, const uint32_t *in, size_t count, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_packing_key(ctx));
  if (count == 0) return TFHE_HIP_OK;
  if (!in || !out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  const size_t groups = (count + kN - 1) / kN;
  return host_call(ctx, false, {{in, count * (size_t)(ctx->P.n + 1) * 4, &ctx->a}}, out, groups * 2 * kN * 4,
                   [&](const void *const *d, void *o) { return pack_launch(ctx, u32(d[0]), count, (uint32_t *)o, ctx->stream); });
}

int tfhe_hip_batch_pack_tlwe_dev(tfhe_hip_ctx *ctx, const uint32_t *in, size_t count, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_packing_key(ctx));
  if (count && (!in || !out)) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  if (count == 0) return TFHE_HIP_OK;
  return pack_launch(ctx, in, count, out, pick(ctx, stream));
}
