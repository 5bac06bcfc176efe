// matmul.hpp -- encrypted linear layers: a plaintext int8 matrix times LWE ciphertexts or the slots of a TRLWE.
//
// The results are normative in include/tfhe_hip.h ("encrypted linear layers").  Both forms are one exact integer GEMM
//
//   out[g][r][x] = sum_{j < cols} (int32)w[r][j] * B_g[j][x]  +  bias[r] * (x == last column)        (mod 2^32)
//
// with M = rows, K = cols and the ciphertext WORDS as columns: B_g[j] is row j of group g of `in` (dense form) or the
// exact lv1 extraction E_g[j] of slot j of TRLWE g (packed form).  As in key_switch_mfma.hpp a u32 word is split into
// four balanced signed byte planes, w = sum_p s_p 256^p (mod 2^32), s_p in [-128, 127], each plane is an
// i8 x i8 -> i32 product on the matrix cores (v_mfma_i32_32x32x32_i8) and the planes recombine as sum_p acc_p << 8p
// in wrapping u32 arithmetic: bit-exact.  Here the A operand is the dense weight matrix instead of a one-hot.
// Accumulator bound: |acc_p| <= cols * 128 * 128 = cols * 2^14 <= 2^30 for cols <= 65,536 (kMmMaxCols): no overflow.
//
// Packed form: E[j][i] = a[j - i] (i <= j), 0 - a[N + j - i] (i > j), E[j][N] = b[j], with the EXACT wrapping
// negation -- not the reference's Torus::MAX - a of k_unpack_extract / k_sample_extract, which is one LSB low per
// negated word: times the weights that would be a deterministic phase offset sum_i s1[i] * sum_{j<i} w[r][j], up to
// 2^26 LSB (1/64 of the torus) at cols = 1024 and weights of 127.
//
// The convolution ("encrypted 2-D convolution") and the polynomial product on packed ciphertexts ("plaintext
// polynomial products": TRLWE in, TRLWE out, K = cols N weights per output word, the 2N words of a ciphertext for
// columns, the same exact negation) are the same GEMM with their own B loaders, MmConv and MmNegacyclic below.
//
// Tiling: a workgroup of kMmWaves = 4 waves owns kMmBM = 64 rows x kMmBN = 128 columns of ONE group and all four
// planes; wave v owns column tile v (32 columns) of both 32-row fragments: 2 x 4 planes = 8 accumulator tiles of
// 16 registers (128), + 4 B fragments (16) + 2 x 2 A fragments, current and next (16) + the 16 staged words of the
// next K-step (16): about 200 VGPRs, two waves per SIMD, two workgroups per CU (LDS 32 KiB, packed form 44 KiB).
// One K-step is K = 32 weights:
//   * A (weights) is already int8 and K-contiguous: a lane's 16 bytes of a fragment are one 16-byte load from global
//     memory (w is small and lives in L1 / L2), issued one step ahead.  Rows past `rows`, K past `cols` and weight
//     rows off 16-byte boundaries (cols % 16 != 0 or an unaligned w) are filled bytewise, zeros outside.
//   * B (ciphertext words) is loaded coalesced along a row -- thread t takes column t & 127 and the 16 K-rows of
//     lane half t >> 7, so a wave's load of one K-row is 256 contiguous bytes --, split into the four plane bytes
//     (mm_planes: the digits of ks_plane_byte, all four at once) and transposed in registers (v_perm_b32) into fragment
//     order: one ds_write_b128 per plane at [plane][tile][lane half][column][16 B], which a wave reads back as its B
//     fragment with one linear ds_read_b128 per plane: conflict-free both ways.  Two buffers, one barrier per step; the
//     loads of a step are issued before the matrix instructions of the step ahead of it.
//   * The B loader is a template parameter: MmDense reads rows of `in`; MmToeplitz generates B[j][i] = ext[j - i]
//     from the one TRLWE of the group, held in LDS already split (ext[t] = a[t], t >= 0; 0 - a[N + t], t < 0: 2N
//     packed words = 8 KiB, + 4 KiB for b, the last column).  The packed form's ninth column block holds the b column
//     alone (N + 1 = 8 * 128 + 1).  MmConv is the 2-D convolution as an implicit GEMM: a group is one output position
//     and K-row (ky, kx, ic) is the input ciphertext under that tap, or zero in the padding -- no im2col buffer.
//     MmNegacyclic is the plaintext polynomial product on packed ciphertexts ("plaintext polynomial products" in the
//     header): K-row j N + m is coefficient m of weight polynomial j, the columns are the 2N words of an output
//     TRLWE, and B[j N + m][c N + i] = ext[i - m] of component c of input polynomial j.  It loads straight from
//     global memory / L2 (kLdsBytes = 0), not from split words staged in LDS as MmToeplitz does: a workgroup walks
//     `cols` different 4 KiB polynomials, not one, so staging would mean a reload and a barrier every 32 K-steps, or
//     cols x 8 KiB of LDS (512 KiB at cols = 64); the 16 words a thread fetches are consecutive descending words of
//     one polynomial and a wave's lanes read consecutive ascending words, so every load is one coalesced 256-byte
//     row segment that hits L1 / L2 after the first touch.  The per-lane work is the index mask and the sign select.
//   * Epilogue: sum_p acc_p << 8p in registers, + bias in the last column, one store per element: a wave writes
//     128-byte row segments.  No atomics, no zeroed output.
// Expected bound: at rows = cols = 1024, n + 1 = 701, 64 groups the product is 2 * 1024 * 1024 * 701 * 64 * 4 planes
// = 3.8e11 int8 ops against 184 MB of `in` read from HBM once (each of the 16 row blocks re-reads it L2 -> LDS: 2.9 GB;
// the grid mapping below keeps those 16 on one XCD) and 184 MB written.  Per K-step a wave issues 8 matrix
// instructions (256 matrix-pipe cycles) against ~100 vector instructions of loading, splitting and transposing its 16
// words (~400 issue cycles, overlapping the other wave of the SIMD at best): the split, paid once per 64 rows, is
// the expected limiter -- not the matrix pipes, and not the L2 -> LDS stream (the packed form, whose B never leaves
// LDS, is little faster per operation).  A taller row block would halve it at 256 accumulator registers (one
// wave per SIMD); interleaving the split of step s + 2 with the matrix instructions of step s is the other way on.
// Measured: DESIGN.md section 9, profiles/matmul_bench.json (the convolution: profiles/conv2d_bench.json).
#pragma once
#include "internal.hpp"

namespace tfhe {

constexpr int kMmWaves = 4;
constexpr int kMmBM = 64;            // rows per workgroup: two 32-row A fragments per wave
constexpr int kMmBN = 32 * kMmWaves; // columns per workgroup: one 32-column tile per wave
constexpr int kMmBufBytes = 4 * kMmWaves * 1024;  // one K-step of B: [plane][tile][64 lanes][16 B]
constexpr size_t kMmMaxCols = 65536;  // accumulator bound, see above
constexpr size_t kMmUnitsPerLaunch = (size_t)1 << 19;  // (group, row block) pairs per launch: x <= 16 column blocks (the polynomial product's 2N / 128) x 256 threads = 2^31 < 2^32
static_assert(kPolymulMaxCols == kMmMaxCols / kN, "polynomial product: K = cols N <= kMmMaxCols, so cols <= 64 (internal.hpp)");
constexpr unsigned kMmXcds = 8;      // accelerator dies a launch's workgroups are dealt to, round-robin

// The four balanced plane bytes of w, byte p = ks_plane_byte(w, p): with u = w + 0x80808080 (the carries of the
// balanced digits are the carries of this addition) s_p = byte_p(u) - 128, as a signed byte byte_p(u) ^ 0x80.
__host__ __device__ __forceinline__ uint32_t mm_planes(uint32_t w) {
  return TFHE_MUT(kMut_mm_plane_carry)  // the two halves added apart: nothing carries out of plane 1 into plane 2
             ? ((((w & 0xFFFFu) + 0x8080u) & 0xFFFFu) | ((w & 0xFFFF0000u) + 0x80800000u)) ^ 0x80808080u
             : (w + 0x80808080u) ^ 0x80808080u;
}

// 4 x 4 byte transpose: x[q] = packed planes of word q -> y[p] = plane p of words 0..3 (word q in byte q).  v_perm_b32
// picks result byte i by selector byte i: 0-3 from the second operand, 4-7 from the first.
__device__ __forceinline__ void mm_transpose4(const uint32_t (&x)[4], uint32_t (&y)[4]) {
  const uint32_t lo01 = __builtin_amdgcn_perm(x[1], x[0], 0x05010400u);  // [q0.p0, q1.p0, q0.p1, q1.p1]
  const uint32_t hi01 = __builtin_amdgcn_perm(x[1], x[0], 0x07030602u);  // [q0.p2, q1.p2, q0.p3, q1.p3]
  const uint32_t lo23 = __builtin_amdgcn_perm(x[3], x[2], 0x05010400u);
  const uint32_t hi23 = __builtin_amdgcn_perm(x[3], x[2], 0x07030602u);
  y[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
  y[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
  y[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
  y[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
}

// ---- B loaders: fetch16 reads the operands of K-rows kb .. kb + 15 at column col as fetched (zero past `cols` and past
// the last column), planes() gives the four plane bytes of one; `setup` runs once per workgroup before the first fetch
// (all threads, ends synchronised; the loader is the kernel's own copy, so `setup` may keep what it decodes in it).  kb is
// wave-uniform: a whole wave takes the unguarded path together. ------------------------------------------------------
struct MmDense {
  static constexpr int kLdsBytes = 0;
  const uint32_t *in;  // [groups][cols][ncol]
  __device__ __forceinline__ void setup(unsigned char *, size_t, int) const {}
  __device__ __forceinline__ void fetch16(uint32_t (&raw)[16], const unsigned char *, size_t g, size_t cols, int ncol,
                                          size_t kb, int col) const {
    // Every lane loads (a lane past the last column reads column 0, a row past `cols` reads the last row) and what
    // is out of range is zeroed afterwards: no divergent branches, and an address is a wave-uniform row base in
    // scalar registers plus the lane's 32-bit column offset.
    const bool col_ok = col < ncol;
    const uint32_t c = col_ok ? (uint32_t)col : 0u;
    if (kb + 16 <= cols) {
      const uint32_t *row = in + (g * cols + kb) * (size_t)ncol;
#pragma unroll
      for (int j = 0; j < 16; ++j, row += ncol) raw[j] = row[c];
    } else {
      const uint32_t *grp = in + g * cols * (size_t)ncol;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const size_t k = kb + (size_t)j;
        const uint32_t v = grp[(k < cols ? k : cols - 1) * (size_t)ncol + c];
        raw[j] = k < cols ? v : 0u;
      }
    }
    if (!col_ok) {
#pragma unroll
      for (int j = 0; j < 16; ++j) raw[j] = 0u;
    }
  }
  __device__ __forceinline__ static uint32_t planes(uint32_t v) { return mm_planes(v); }
};

struct MmToeplitz {
  static constexpr int kLdsBytes = 3 * kN * 4;  // ext (2N packed words, index t + N) + b (N packed words)
  const uint32_t *trlwe;  // [groups][2][N]
  __device__ __forceinline__ void setup(unsigned char *lds, size_t g, int tid) const {
    uint32_t *ext = reinterpret_cast<uint32_t *>(lds);
    const uint32_t *a = trlwe + g * (size_t)(2 * kN), *b = a + kN;
    for (int t = tid; t < kN; t += 64 * kMmWaves) {
      const uint32_t v = a[t];
      ext[kN + t] = mm_planes(v);   // ext[t] = a[t]
      ext[t] = mm_planes(TFHE_MUT(kMut_mm_toeplitz_wrap) ? ~v : 0u - v);   // ext[t - N] = 0 - a[t]   (index 0, t = -N, is never read)
      ext[2 * kN + t] = mm_planes(b[t]);
    }
    __syncthreads();
  }
  // ncol == N + 1, cols <= N: B[k][col] = ext[k - col] for col < N, b[k] for col == N; consecutive words for the 16 rows
  __device__ __forceinline__ void fetch16(uint32_t (&raw)[16], const unsigned char *lds, size_t, size_t cols, int,
                                          size_t kb, int col) const {
    const uint32_t *ext = reinterpret_cast<const uint32_t *>(lds);
    const int k = (int)kb, lim = (int)cols;
    // every lane reads (clamped in range: column > N reads b, a row past `cols` the last row), zeroed afterwards
    const uint32_t *src = col < kN ? ext + (kN - col) : ext + 2 * kN;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int kk = k + j < lim ? k + j : lim - 1;
      const uint32_t v = src[kk];
      raw[j] = (k + j < lim && col <= kN) ? v : 0u;
    }
  }
  __device__ __forceinline__ static uint32_t planes(uint32_t v) { return v; }  // split once, in setup
};

// floor(n / d) for n < 2^17 (a K index: K <= kMmMaxCols, + one K-step) by a multiplication: with m = ceil(2^34 / d),
// e = m d - 2^34 < d <= 2^16 and n e < 2^33 < 2^34, so floor(n m / 2^34) = floor(n / d) (Granlund & Montgomery 1994).
// On wave-uniform operands this is scalar arithmetic: no division in the K loop.
__host__ __device__ __forceinline__ uint64_t mm_div_magic(uint32_t d) { return (((uint64_t)1 << 34) + d - 1) / d; }
__device__ __forceinline__ uint32_t mm_div(uint32_t n, uint64_t magic) { return (uint32_t)(((uint64_t)n * magic) >> 34); }

// 2-D convolution as an implicit GEMM (include/tfhe_hip.h, "encrypted 2-D convolution"): the kernel's group is the
// virtual group vg = (g out_h + oy) out_w + ox, one output position; rows = out_c, cols = K = k_h k_w in_c, and K-row
// k = (ky k_w + kx) in_c + ic of that position is the input ciphertext at (oy s_h + ky - p_h, ox s_w + kx - p_w, ic),
// or zero in the padding.  With rows = out_c the epilogue's out[(vg rows + r) ncol + col] is the channels-last output.
// `setup` decodes vg once per workgroup (scalar registers) and keeps the image and the position's top-left input
// coordinate in the loader, which is the kernel's own copy.  fetch16 finds the tap of its first row with mm_div and
//   * in_c % 16 == 0: the 16 rows lie inside one tap (kb is a multiple of 16): one wave-uniform base address, rows
//     ncol words apart -- MmDense's unguarded path -- or no loads at all for a padding tap or past K;
//   * any in_c: walks (ky, kx, ic) across the 16 rows; every lane loads from an in-range address (word 0 of the
//     image stands in for padding and for rows past K) and what is not there is zeroed afterwards: no divergent
//     branches.
struct MmConv {
  static constexpr int kLdsBytes = 0;
  const uint32_t *in;      // [groups][in_h][in_w][in_c][ncol]
  size_t img_words;        // in_h in_w in_c ncol
  uint64_t magic_c, magic_kw;  // mm_div_magic(in_c), mm_div_magic(k_w)
  uint32_t in_h, in_w, in_c, k_w, stride_h, stride_w, pad_h, pad_w, out_h, out_w;
  int iy0, ix0;            // set by setup: input coordinate of tap (0, 0) of this workgroup's position
  __device__ __forceinline__ void setup(unsigned char *, size_t vg, int) {
    const uint32_t v = (uint32_t)vg, t = v / out_w, ox = v - t * out_w, g = t / out_h, oy = t - g * out_h;
    in += (size_t)g * img_words;
    iy0 = (int)(oy * stride_h) - (int)pad_h;
    // (the mutant's column is another tap of the same map: the ix < in_w guards below stand)
    ix0 = (int)(ox * (TFHE_MUT(kMut_mm_conv_stride) ? stride_h : stride_w)) - (int)pad_w;
  }
  __device__ __forceinline__ void fetch16(uint32_t (&raw)[16], const unsigned char *, size_t, size_t cols, int ncol,
                                          size_t kb, int col) const {
    const bool col_ok = col < ncol;
    const uint32_t c = col_ok ? (uint32_t)col : 0u;
    const uint32_t k = (uint32_t)kb, K = (uint32_t)cols;
    const uint32_t tap = mm_div(k, magic_c), ky0 = mm_div(tap, magic_kw);
    uint32_t ic = k - tap * in_c, kx = tap - ky0 * k_w, ky = ky0;
    if ((in_c & 15u) == 0u) {
      const uint32_t iy = (uint32_t)(iy0 + (int)ky), ix = (uint32_t)(ix0 + (int)kx);  // (negative: above every bound)
      if (k < K && iy < in_h && ix < in_w) {
        const uint32_t *row = in + (size_t)((iy * in_w + ix) * in_c + ic) * (size_t)ncol;
#pragma unroll
        for (int j = 0; j < 16; ++j, row += ncol) raw[j] = row[c];
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) raw[j] = 0u;
      }
    } else {
      // the tap's state -- inside the map?  word offset of its row ic -- is worked out where the tap changes only
      bool inside;
      size_t off;
      auto enter_tap = [&]() {
        const uint32_t iy = (uint32_t)(iy0 + (int)ky), ix = (uint32_t)(ix0 + (int)kx);
        inside = iy < in_h && ix < in_w;
        off = inside ? (size_t)((iy * in_w + ix) * in_c + ic) * (size_t)ncol : (size_t)0;
      };
      enter_tap();
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const bool ok = inside && k + (uint32_t)j < K;
        const uint32_t v = in[(ok ? off : (size_t)0) + c];
        raw[j] = TFHE_MUT(kMut_mm_conv_pad) ? (ok || k + (uint32_t)j < K ? v : 0u) : (ok ? v : 0u);  // (a padding tap keeps its stand-in word)
        off += (size_t)ncol;
        if (++ic == in_c) {
          ic = 0u;
          if (++kx == k_w) kx = 0u, ++ky;
          enter_tap();
        }
      }
    }
    if (!col_ok) {
#pragma unroll
      for (int j = 0; j < 16; ++j) raw[j] = 0u;
    }
  }
  __device__ __forceinline__ static uint32_t planes(uint32_t v) { return mm_planes(v); }
};

// Plaintext polynomial product on packed ciphertexts (include/tfhe_hip.h, "plaintext polynomial products"): the kernel's
// `cols` is K = (weight polynomials per output) x N and ncol = 2N.  K-row k = j N + m is coefficient m of weight
// polynomial j, column x = c N + i is coefficient i of component c (0: a, 1: b) of the output, and
//   B[k][x] = ext[i - m] of in[g][j][c]:  p[i - m] for i >= m,  0 - p[N + i - m] for i < m   (exact wrapping negation).
// A workgroup's 128 columns lie inside one component (N % kMmBN == 0) and a 16-row fetch inside one j (kb and N are
// multiples of 16): the polynomial's base address is wave-uniform.  K is a multiple of 32 and ncol of kMmBN, so there
// is no K tail and no column tail: kb + 16 <= K and col < ncol on every call, and every index is masked into the
// polynomial.  No divergent branches: the sign is a select.
struct MmNegacyclic {
  static constexpr int kLdsBytes = 0;
  const uint32_t *trlwe;  // [groups][K / N][2][N]
  __device__ __forceinline__ void setup(unsigned char *, size_t, int) const {}
  __device__ __forceinline__ void fetch16(uint32_t (&raw)[16], const unsigned char *, size_t g, size_t cols, int,
                                          size_t kb, int col) const {
    const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)col / (uint32_t)kN));  // (workgroup-uniform)
    const size_t j = kb / (size_t)kN;
    const uint32_t *p = trlwe + ((g * (cols / (size_t)kN) + j) * 2 + c) * (size_t)kN;
    uint32_t t = (uint32_t)(col & (kN - 1)) - (uint32_t)(kb & (size_t)(kN - 1));  // i - m, in (-N, N) as an int32
#pragma unroll
    for (int e = 0; e < 16; ++e, --t) {
      const uint32_t v = p[t & (uint32_t)(kN - 1)];
      raw[e] = (int32_t)t < 0 ? (TFHE_MUT(kMut_mm_nega_wrap) ? ~v : 0u - v) : v;
    }
  }
  __device__ __forceinline__ static uint32_t planes(uint32_t v) { return mm_planes(v); }
};

// The bias polynomial of the polynomial product: out[u][1][i] += bias[u % rows][i] for the `units` = groups x rows
// output ciphertexts from u0 on, one workgroup per ciphertext, four words a thread (word by word: neither pointer need
// be 16-byte aligned).  (k_tlwe_matmul's own bias is one word in the last column.)
constexpr int kPolymulBiasThreads = kN / 4;
__global__ __launch_bounds__(kPolymulBiasThreads) void k_polymul_bias(const uint32_t *__restrict__ bias, size_t rows, size_t u0,
                                                           uint32_t *__restrict__ out) {
  const size_t u = u0 + blockIdx.x;
  const uint32_t *src = bias + (TFHE_MUT(kMut_mm_polymul_bias) ? (u < rows ? u : 0) : u % rows) * (size_t)kN;  // (a row inside the bias this launch reads either way)
  uint32_t *dst = out + (2 * u + 1) * (size_t)kN;
#pragma unroll
  for (int i = threadIdx.x; i < kN; i += kPolymulBiasThreads) dst[i] += src[i];
}

// One launch covers groups g0 .. and row blocks rb0 .. rb0 + nrb - 1 of each (nrb < all row blocks only with one group a
// launch) in a 1-D grid of groups x column blocks x nrb workgroups.  Workgroups are handed to the 8 XCDs round-robin in
// dispatch order, so the dispatch index is first turned into a virtual index whose consecutive values share an XCD, and
// that is decoded row block fastest: the workgroups that read the same ciphertext words (one group, one column block,
// every row block) run on ONE XCD at about the same time and its L2 fetches those words once, not once per XCD.
// out is [groups][rows][ncol]; bias (or NULL) is added in column ncol - 1.
template <class Loader>
__global__ __launch_bounds__(64 * kMmWaves, 2) void k_tlwe_matmul(Loader ld, const int8_t *__restrict__ w,
                                                                   const uint32_t *__restrict__ bias, size_t rows,
                                                                   size_t cols, int ncol, size_t g0, unsigned rb0,
                                                                   unsigned nrb, uint32_t *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kMmBufBytes + Loader::kLdsBytes];
  unsigned char *lds_ld = smem + 2 * kMmBufBytes;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned total = gridDim.x, xcd = blockIdx.x % kMmXcds, slot = blockIdx.x / kMmXcds;
  const unsigned per = total / kMmXcds, rem = total % kMmXcds;  // XCD x runs per + (x < rem) of the workgroups
  // (the mutant's index is xcd per + slot: below (xcd + 1) per <= total where slot < per, and slot == per only on an
  // XCD below rem <= 7, where it is (xcd + 1) per <= 7 per < total: a tile of this launch, some taken twice)
  const unsigned virt = TFHE_MUT(kMut_mm_xcd_rem) ? xcd * per + slot : xcd * per + (xcd < rem ? xcd : rem) + slot;
  const unsigned col_blocks = (unsigned)((ncol + kMmBN - 1) / kMmBN);
  const size_t g = g0 + (size_t)(virt / (nrb * col_blocks)), row0 = (size_t)(rb0 + virt % nrb) * (size_t)kMmBM;
  const int col0 = (int)((virt / nrb) % col_blocks) * kMmBN;
  ld.setup(lds_ld, g, tid);

  // B staging: this thread's column and lane half; its 16 K-rows of a step are k0 + 16 bh + (0..15)
  const int bcol = col0 + (tid & (kMmBN - 1)), bh = __builtin_amdgcn_readfirstlane(tid >> 7);  // (bh: wave-uniform)
  const uint32_t b_store = (uint32_t)(((tid & (kMmBN - 1)) >> 5) * 1024 + bh * 512 + (tid & 31) * 16);
  // A fragments: row row0 + 32 f + (lane & 31), K bytes k0 + 16 (lane >> 5) + (0..15)
  const bool w_aligned = (cols & 15) == 0 && ((size_t)w & 15) == 0;  // every fragment start is 16-byte aligned
  const int ah = lane >> 5;
  const int8_t *a_row[2];  // this lane's two weight rows at its K offset (row 0 stands in for rows past the end: never read)
  bool a_ok[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const size_t r = row0 + (size_t)(32 * f + (lane & 31));
    a_ok[f] = r < rows;
    a_row[f] = w + (a_ok[f] ? r : 0) * cols + (size_t)(16 * ah);
  }
  auto load_a = [&](size_t k0, int f) -> km_i32x4 {
    const size_t k = k0 + (size_t)(16 * ah);
    km_u32x4 v = {0u, 0u, 0u, 0u};
    if (a_ok[f] && k < cols) {
      const int8_t *src = a_row[f] + k0;
      if (w_aligned) {  // (cols % 16 == 0: a fragment that starts inside the row ends inside it)
        v = *reinterpret_cast<const km_u32x4 *>(src);
      } else {
        const int m = cols - k < 16 ? (int)(cols - k) : 16;
        uint32_t d[4] = {0u, 0u, 0u, 0u};
        for (int j = 0; j < m; ++j) {
          const uint32_t byte = TFHE_MUT(kMut_mm_a_sign) ? (uint32_t)(int32_t)src[j] : (uint32_t)(uint8_t)src[j];
          d[j >> 2] |= (TFHE_MUT(kMut_mm_a_tail) ? (m < 16 && j == m - 1 ? 0u : byte) : byte) << (8 * (j & 3));
        }
        v = km_u32x4{d[0], d[1], d[2], d[3]};
      }
    }
    return __builtin_bit_cast(km_i32x4, v);
  };
  uint32_t braw[16];
  auto fetch_b = [&](size_t k0) {
    ld.fetch16(braw, lds_ld, g, cols, ncol, k0 + (size_t)(16 * bh), bcol);
  };
  auto store_b = [&](unsigned char *buf) {
    uint32_t y[4][4];  // [q][p]: plane p, fragment bytes 4q .. 4q + 3
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t x[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = Loader::planes(braw[4 * q + e]);
      mm_transpose4(x, y[q]);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
      *reinterpret_cast<km_u32x4 *>(buf + p * (kMmWaves * 1024) + b_store) = km_u32x4{y[0][p], y[1][p], y[2][p], y[3][p]};
  };

  km_i32x16 acc[2][4];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[f][p] = km_i32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

  const size_t steps = (cols + 31) / 32;
  km_i32x4 A[2] = {load_a(0, 0), load_a(0, 1)};
  fetch_b(0);
  store_b(smem);
  __syncthreads();
#pragma unroll 1
  for (size_t s = 0; s < steps; ++s) {
    unsigned char *cur = smem + (s & 1) * kMmBufBytes, *nxt = smem + ((s + 1) & 1) * kMmBufBytes;
    const bool more = s + 1 < steps;  // workgroup-uniform
    km_i32x4 An[2] = {A[0], A[1]};
    if (more) {  // the next step's operands are fetched under this step's matrix instructions
      An[0] = load_a((s + 1) * 32, 0);
      An[1] = load_a((s + 1) * 32, 1);
      fetch_b((s + 1) * 32);
    }
    km_i32x4 B[4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
      B[p] = *reinterpret_cast<const km_i32x4 *>(cur + p * (kMmWaves * 1024) + wave * 1024 + lane * 16);
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int f = 0; f < 2; ++f) acc[f][p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[f], B[p], acc[f][p], 0, 0, 0);
    if (more) store_b(nxt);  // (nobody reads nxt before the barrier; its readers of step s - 1 passed the last one)
    A[0] = An[0];
    A[1] = An[1];
    __syncthreads();
  }

  // C tile element e of lane: row 32 f + (e & 3) + 8 (e >> 2) + 4 (lane >> 5), column lane & 31
  const int col = col0 + 32 * wave + (lane & 31);
  if (col < ncol) {
    const bool last = col == ncol - 1 && bias != nullptr;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const size_t r = row0 + (size_t)(32 * f + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5));
        if (r < rows) {
          uint32_t v = (uint32_t)acc[f][0][e] + ((uint32_t)acc[f][1][e] << 8) + ((uint32_t)acc[f][2][e] << 16) +
                       ((uint32_t)acc[f][3][e] << 24);
          if (last) v += bias[r];
          out[(g * rows + r) * (size_t)ncol + (size_t)col] = v;
        }
      }
  }
}

}  // namespace tfhe

// ---- encrypted linear layers ------------------------------------------------------------------------------------------
namespace {
template <class Loader>
int launch_matmul(tfhe_hip_ctx *ctx, Loader ld, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols, int ncol,
                  size_t groups, uint32_t *out, hipStream_t s) {
  const size_t row_blocks = (rows + kMmBM - 1) / kMmBM;
  const unsigned col_blocks = (unsigned)((ncol + kMmBN - 1) / kMmBN);
  auto launch = [&](size_t g0, size_t ng, size_t rb0, size_t nrb) -> int {
    hipLaunchKernelGGL((k_tlwe_matmul<Loader>), dim3((unsigned)(ng * nrb) * col_blocks), dim3(64 * kMmWaves), 0, s, ld, w, bias,
                       rows, cols, ncol, g0, (unsigned)rb0, (unsigned)nrb, out);
    return launched(ctx);
  };
  if (row_blocks <= kMmUnitsPerLaunch) {  // whole groups per launch
    const size_t step = kMmUnitsPerLaunch / row_blocks;
    for (size_t g0 = 0; g0 < groups; g0 += step) CHK(launch(g0, groups - g0 < step ? groups - g0 : step, 0, row_blocks));
  } else {  // more than 2^25 rows: one group a launch, in chunks of row blocks
    for (size_t g = 0; g < groups; ++g)
      for (size_t rb0 = 0; rb0 < row_blocks; rb0 += kMmUnitsPerLaunch)
        CHK(launch(g, 1, rb0, row_blocks - rb0 < kMmUnitsPerLaunch ? row_blocks - rb0 : kMmUnitsPerLaunch));
  }
  return TFHE_HIP_OK;
}

int matmul_dev(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols, const uint32_t *in,
               size_t groups, uint32_t *out, hipStream_t s) {
  return launch_matmul(ctx, MmDense{in}, w, bias, rows, cols, ctx->P.n + 1, groups, out, s);
}

// the lv1 rows straight into `out`, or into the context's lv1 scratch and through the key switch of the bootstrap path
int matmul_packed_dev(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols,
                      const uint32_t *trlwe, size_t groups, int keyswitch, uint32_t *out, hipStream_t s) {
  if (!keyswitch) return launch_matmul(ctx, MmToeplitz{trlwe}, w, bias, rows, cols, kN + 1, groups, out, s);
  const size_t count = rows * groups;
  CHK(take(ctx, s, ctx->lv1, lv1_bytes(count)));
  uint32_t *lv1 = (uint32_t *)ctx->lv1.p;
  CHK(launch_matmul(ctx, MmToeplitz{trlwe}, w, bias, rows, cols, kN + 1, groups, lv1, s));
  return launch_key_switch(ctx, s, lv1, out, count);
}

// the checks all four calls share, in one order: key (key-switched packed form), shape, empty batch, pointers, count
// (returns TFHE_HIP_OK with *run = false for an empty batch)
int matmul_checks(tfhe_hip_ctx *ctx, bool need_cloud_key, const int8_t *w, size_t rows, size_t cols, size_t max_cols,
                  const uint32_t *in, size_t groups, const uint32_t *out, bool *run) {
  *run = false;
  if (need_cloud_key) CHK(need_key(ctx));
  if (rows == 0) return fail(ctx, TFHE_HIP_EINVAL, "rows must be at least 1");
  if (cols == 0 || cols > max_cols) return fail(ctx, TFHE_HIP_EINVAL, "cols out of range");
  if (groups == 0) return TFHE_HIP_OK;
  if (!w || !in || !out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  if (rows > 0x7FFFFFFFull || groups > 0x7FFFFFFFull / rows) return fail(ctx, TFHE_HIP_EINVAL, "rows * groups too large");
  *run = true;
  return TFHE_HIP_OK;
}
}  // namespace

int tfhe_hip_batch_tlwe_matmul(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols,
                               const uint32_t *in, size_t groups, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  bool run = false;
  CHK(matmul_checks(ctx, false, w, rows, cols, kMmMaxCols, in, groups, out, &run));
  if (!run) return TFHE_HIP_OK;
  return host_call(ctx, false, {{w, rows * cols, &ctx->a}, {bias, rows * 4, &ctx->b}, {in, tlwe_bytes(ctx, groups * cols), &ctx->c}},
                   out, tlwe_bytes(ctx, groups * rows), [&](const void *const *d, void *o) {
                     return matmul_dev(ctx, (const int8_t *)d[0], u32(d[1]), rows, cols, u32(d[2]), groups, (uint32_t *)o, ctx->stream);
                   });
}

int tfhe_hip_batch_tlwe_matmul_dev(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols,
                                   const uint32_t *in, size_t groups, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  bool run = false;
  CHK(matmul_checks(ctx, false, w, rows, cols, kMmMaxCols, in, groups, out, &run));
  if (!run) return TFHE_HIP_OK;
  return matmul_dev(ctx, w, bias, rows, cols, in, groups, out, pick(ctx, stream));
}

int tfhe_hip_batch_trlwe_matmul(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols,
                                const uint32_t *trlwe, size_t groups, int keyswitch, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  bool run = false;
  CHK(matmul_checks(ctx, keyswitch != 0, w, rows, cols, (size_t)kN, trlwe, groups, out, &run));
  if (!run) return TFHE_HIP_OK;
  const size_t out_bytes = keyswitch ? tlwe_bytes(ctx, groups * rows) : groups * rows * (size_t)(kN + 1) * 4;
  return host_call(ctx, false, {{w, rows * cols, &ctx->a}, {bias, rows * 4, &ctx->b}, {trlwe, trlwe_bytes(groups), &ctx->c}}, out,
                   out_bytes, [&](const void *const *d, void *o) {
                     return matmul_packed_dev(ctx, (const int8_t *)d[0], u32(d[1]), rows, cols, u32(d[2]), groups, keyswitch,
                                              (uint32_t *)o, ctx->stream);
                   });
}

int tfhe_hip_batch_trlwe_matmul_dev(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols,
                                    const uint32_t *trlwe, size_t groups, int keyswitch, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  bool run = false;
  CHK(matmul_checks(ctx, keyswitch != 0, w, rows, cols, (size_t)kN, trlwe, groups, out, &run));
  if (!run) return TFHE_HIP_OK;
  return matmul_packed_dev(ctx, w, bias, rows, cols, trlwe, groups, keyswitch, out, pick(ctx, stream));
}

// ---- plaintext polynomial products on packed ciphertexts: the same GEMM with K = cols N and 2N columns (MmNegacyclic) --
// (declared in internal.hpp: the TRLWE key switch of rings.hip runs on it)
int polymul_dev(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols, const uint32_t *trlwe,
                size_t groups, uint32_t *out, hipStream_t s) {
  CHK(launch_matmul(ctx, MmNegacyclic{trlwe}, w, nullptr, rows, cols * (size_t)kN, 2 * kN, groups, out, s));
  if (!bias) return TFHE_HIP_OK;
  constexpr size_t per_launch = (size_t)1 << 23;  // workgroups a launch: x 256 threads = 2^31 < 2^32
  const size_t units = groups * rows;
  for (size_t u0 = 0; u0 < units; u0 += per_launch) {
    hipLaunchKernelGGL(k_polymul_bias, dim3((unsigned)(units - u0 < per_launch ? units - u0 : per_launch)),
                       dim3(kPolymulBiasThreads), 0, s, bias, rows, u0, out);
    CHK(launched(ctx));
  }
  return TFHE_HIP_OK;
}

int tfhe_hip_batch_trlwe_polymul(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols,
                                 const uint32_t *trlwe, size_t groups, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  bool run = false;
  CHK(matmul_checks(ctx, false, w, rows, cols, kPolymulMaxCols, trlwe, groups, out, &run));
  if (!run) return TFHE_HIP_OK;
  return host_call(ctx, false, {{w, rows * cols * (size_t)kN, &ctx->a}, {bias, rows * (size_t)kN * 4, &ctx->b}, {trlwe, trlwe_bytes(groups * cols), &ctx->c}},
                   out, trlwe_bytes(groups * rows), [&](const void *const *d, void *o) {
                     return polymul_dev(ctx, (const int8_t *)d[0], u32(d[1]), rows, cols, u32(d[2]), groups, (uint32_t *)o, ctx->stream);
                   });
}

int tfhe_hip_batch_trlwe_polymul_dev(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols,
                                     const uint32_t *trlwe, size_t groups, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  bool run = false;
  CHK(matmul_checks(ctx, false, w, rows, cols, kPolymulMaxCols, trlwe, groups, out, &run));
  if (!run) return TFHE_HIP_OK;
  return polymul_dev(ctx, w, bias, rows, cols, trlwe, groups, out, pick(ctx, stream));
}

// ---- encrypted 2-D convolution: the same GEMM with output positions for groups (MmConv) ------------------------------
namespace {
struct ConvGeom {
  size_t K, out_h, out_w, positions;  // positions = groups * out_h * out_w, saturated at SIZE_MAX
  size_t in_cts, out_cts;             // ciphertexts of `in` and of `out`
};

// The checks both calls share, in one order: shape (NULL, a zero field, a filter larger than the padded map, K), then
// matmul_checks on the equivalent product -- rows = out_c, cols = K, one group per output position: out_c == 0, K out of
// range, the empty batch, the pointers, out_c * positions too large -- and last the size of the input.
int conv2d_checks(tfhe_hip_ctx *ctx, const tfhe_hip_conv2d_shape *sh, const int8_t *w, const uint32_t *in, size_t groups,
                  const uint32_t *out, ConvGeom *geo, bool *run) {
  *run = false;
  if (!sh) return fail(ctx, TFHE_HIP_EINVAL, "null shape");
  if (!sh->in_h || !sh->in_w || !sh->in_c || !sh->k_h || !sh->k_w) return fail(ctx, TFHE_HIP_EINVAL, "conv2d: a zero dimension");
  if (!sh->stride_h || !sh->stride_w) return fail(ctx, TFHE_HIP_EINVAL, "conv2d: stride must be at least 1");
  const uint64_t ph = (uint64_t)sh->in_h + 2 * (uint64_t)sh->pad_h, pw = (uint64_t)sh->in_w + 2 * (uint64_t)sh->pad_w;
  if (ph > 0x7FFFFFFFull || pw > 0x7FFFFFFFull) return fail(ctx, TFHE_HIP_EINVAL, "conv2d: padded map too large");
  if (sh->k_h > ph || sh->k_w > pw) return fail(ctx, TFHE_HIP_EINVAL, "conv2d: filter larger than the padded map");
  const uint64_t taps = (uint64_t)sh->k_h * sh->k_w;  // < 2^62
  const uint64_t K = taps > kMmMaxCols ? kMmMaxCols + 1 : taps * sh->in_c;  // (<= 2^48; out of range either way)
  geo->K = (size_t)K;
  geo->out_h = (size_t)((ph - sh->k_h) / sh->stride_h + 1);
  geo->out_w = (size_t)((pw - sh->k_w) / sh->stride_w + 1);
  const size_t per = geo->out_h * geo->out_w;  // < 2^62
  geo->positions = groups > SIZE_MAX / per ? SIZE_MAX : groups * per;
  CHK(matmul_checks(ctx, false, w, sh->out_c, geo->K, kMmMaxCols, in, geo->positions, out, run));
  if (!*run) return TFHE_HIP_OK;
  *run = false;
  const uint64_t pix = (uint64_t)sh->in_h * sh->in_w;  // <= 2^62
  if (pix > 0x7FFFFFFFull || pix * sh->in_c > 0x7FFFFFFFull || groups > 0x7FFFFFFFull / (pix * sh->in_c))
    return fail(ctx, TFHE_HIP_EINVAL, "conv2d: groups * in_h * in_w * in_c too large");
  geo->in_cts = groups * (size_t)(pix * sh->in_c);
  geo->out_cts = geo->positions * sh->out_c;
  *run = true;
  return TFHE_HIP_OK;
}

int conv2d_dev(tfhe_hip_ctx *ctx, const tfhe_hip_conv2d_shape &sh, const ConvGeom &geo, const int8_t *w, const uint32_t *bias,
               const uint32_t *in, uint32_t *out, hipStream_t s) {
  const int ncol = ctx->P.n + 1;
  MmConv ld{};
  ld.in = in;
  ld.img_words = (size_t)sh.in_h * sh.in_w * sh.in_c * (size_t)ncol;
  ld.magic_c = mm_div_magic(sh.in_c);
  ld.magic_kw = mm_div_magic(sh.k_w);
  ld.in_h = sh.in_h, ld.in_w = sh.in_w, ld.in_c = sh.in_c, ld.k_w = sh.k_w;
  ld.stride_h = sh.stride_h, ld.stride_w = sh.stride_w, ld.pad_h = sh.pad_h, ld.pad_w = sh.pad_w;
  ld.out_h = (uint32_t)geo.out_h, ld.out_w = (uint32_t)geo.out_w;
  return launch_matmul(ctx, ld, w, bias, sh.out_c, geo.K, ncol, geo.positions, out, s);
}
}  // namespace

int tfhe_hip_batch_tlwe_conv2d(tfhe_hip_ctx *ctx, const tfhe_hip_conv2d_shape *shape, const int8_t *w, const uint32_t *bias,
                               const uint32_t *in, size_t groups, uint32_t *out) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  bool run = false;
  ConvGeom geo{};
  CHK(conv2d_checks(ctx, shape, w, in, groups, out, &geo, &run));
  if (!run) return TFHE_HIP_OK;
  const tfhe_hip_conv2d_shape sh = *shape;
  return host_call(ctx, false, {{w, sh.out_c * geo.K, &ctx->a}, {bias, (size_t)sh.out_c * 4, &ctx->b}, {in, tlwe_bytes(ctx, geo.in_cts), &ctx->c}},
                   out, tlwe_bytes(ctx, geo.out_cts), [&](const void *const *d, void *o) {
                     return conv2d_dev(ctx, sh, geo, (const int8_t *)d[0], u32(d[1]), u32(d[2]), (uint32_t *)o, ctx->stream);
                   });
}

int tfhe_hip_batch_tlwe_conv2d_dev(tfhe_hip_ctx *ctx, const tfhe_hip_conv2d_shape *shape, const int8_t *w, const uint32_t *bias,
                                   const uint32_t *in, size_t groups, uint32_t *out, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  bool run = false;
  ConvGeom geo{};
  CHK(conv2d_checks(ctx, shape, w, in, groups, out, &geo, &run));
  if (!run) return TFHE_HIP_OK;
  return conv2d_dev(ctx, *shape, geo, w, bias, in, out, pick(ctx, stream));
}
