// tfhe_hip.hip -- C ABI (include/tfhe_hip.h) over the gfx950 kernels: the core translation unit of libtfhe_hip.so.
// (The feature units, planes.hip and rings.hip, reach it through internal.hpp and nothing else.)
//
// Host side of the engine: context (device, stream, converted cloud key,
// scratch), launch geometry, and the batched entry points that compose
//   gate prep + blind rotate (one persistent kernel)  ->  key switch (one kernel)
// exactly as gates::batch_* composes them in the reference
// (src/gates.rs:357-383: prepare, batch_blind_rotate, extract + key switch).
#include <hip/hip_runtime.h>

#include <errno.h>
#include <sys/random.h>

// This unit owns the kernels of these headers; every other unit sees them with internal linkage (internal.hpp).
#define TFHE_HIP_CORE_UNIT
#include "blind_rotate.hpp"
#include "blind_rotate_wide.hpp"
#include "key_switch.hpp"
#include "key_switch_mfma.hpp"
#include "keygen.hpp"
#include "twiddles_host.hpp"

#include "internal.hpp"

namespace {

thread_local std::string g_create_error = "";

// Error text is kept PER (calling thread, handle): the header promises Send + Sync use of a handle
// (src/bootstrap/mod.rs:23), so two threads may fail on one context at the same time, and each must read its own
// message -- not a string another thread is assigning or has freed.  Every context and pool carries an id that is
// never reused; the text lives in a thread-local table keyed by it, and tfhe_hip_last_error() returns the calling
// thread's entry (valid until that thread's next failing call on the same handle).
// A handle's entry is erased by the thread that destroys it; entries other threads made for it would stay for those
// threads' lifetimes (a long-lived worker that fails once on each of many short-lived contexts), so the table is bounded:
// when a thread's table has grown past kErrTableSoftCap entries, the next failure on that thread drops the entries of
// handles that no longer exist (g_live_handles).  Reading never inserts.
std::atomic<uint64_t> g_next_handle_id{1};
// The table is reached through a plain pointer: a thread's thread_local objects are destroyed before the process's
// static ones, so a handle destroyed from a static destructor at exit (the C++ mirror's engine registry) after a
// failing call on the main thread would otherwise erase from a destroyed map.  The pointer is null before the
// thread's first failure and again once the thread's table is gone.
typedef std::unordered_map<uint64_t, std::string> ErrTable;
thread_local ErrTable *t_errors = nullptr;
struct ErrTableOwner {
  ~ErrTableOwner() {
    delete t_errors;
    t_errors = nullptr;
  }
};
std::mutex g_live_mu;
std::unordered_set<uint64_t> g_live_handles;
constexpr size_t kErrTableSoftCap = 64;
}  // namespace
uint64_t new_handle_id() {  // never reused
  const uint64_t id = g_next_handle_id.fetch_add(1);
  std::lock_guard<std::mutex> lk(g_live_mu);
  g_live_handles.insert(id);
  return id;
}
void handle_gone(uint64_t id) {
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    g_live_handles.erase(id);
  }
  if (t_errors) t_errors->erase(id);
}
// the slot a FAILING call writes its text into (references survive rehashing)
std::string &err_slot(uint64_t id) {
  thread_local ErrTableOwner owner;  // frees the table when the thread ends
  (void)owner;
  if (!t_errors) t_errors = new ErrTable();
  ErrTable &t = *t_errors;
  if (t.size() >= kErrTableSoftCap && !t.count(id)) {
    std::lock_guard<std::mutex> lk(g_live_mu);
    for (auto it = t.begin(); it != t.end();) it = g_live_handles.count(it->first) ? std::next(it) : t.erase(it);
  }
  return t[id];
}
namespace {
// the calling thread's last failure text on handle `id`, "" if it never failed there (no entry is made)
inline const char *err_text(uint64_t id) {
  static const std::string none;
  if (!t_errors) return none.c_str();
  const auto it = t_errors->find(id);
  return it == t_errors->end() ? none.c_str() : it->second.c_str();
}

constexpr int kKsG = 32;  // ciphertexts per key-switch workgroup

}  // namespace

// ---- errors, buffers, scratch (declared in internal.hpp and secrets.hpp) -------------------------------------------------
int fail(tfhe_hip_ctx *ctx, int code, const std::string &msg) {
  err_slot(ctx->id) = msg;
  return code;
}

// a runtime call that resources.hpp made for this context
int hip_rc(tfhe_hip_ctx *ctx, const HipErr &r) {
  return r ? fail(ctx, TFHE_HIP_EHIP, std::string(r.what) + ": " + hipGetErrorString(r.e)) : TFHE_HIP_OK;
}

int ensure(tfhe_hip_ctx *ctx, DevBuf &b, size_t bytes) {
  if (const hipError_t e = b.grow(bytes)) return fail(ctx, TFHE_HIP_ENOMEM, std::string("hipMalloc scratch: ") + hipGetErrorString(e));
  return TFHE_HIP_OK;
}

// A buffer of exactly `bytes` that is allocated once; `call` is how that allocation reads in the text of its failure.
int alloc_exact(tfhe_hip_ctx *ctx, DevBuf &b, size_t bytes, const char *call) {
  return hip_rc(ctx, {b.grow(bytes, true), call});
}

// The intermediate buffers (lv1, u1, u2, the key switch's ks_out and ks_dig, the tree bootstrap's biv_s1 and
// biv_tv) belong to the context, not to a call.  Work queued on one stream may still be using them when the
// next call arrives on another stream: drain the previous owner first (same-stream calls are ordered by the
// stream itself and pay nothing).  take() (below) claims and then sizes; SecretStage claims in its constructor.
int claim_scratch(tfhe_hip_ctx *ctx, hipStream_t s) { return hip_rc(ctx, ctx->scratch.claim(s)); }

namespace {
// Waits for the stream that owns the scratch (`unless_own`: not where that is the context's stream, which the caller
// drains next).
HipErr sync_scratch_owner(tfhe_hip_ctx *ctx, bool unless_own = false) {
  const Scratch &sc = ctx->scratch;
  if (!sc.owned || (unless_own && sc.owner == ctx->stream)) return {};
  return {hipStreamSynchronize(sc.owner), "hipStreamSynchronize(ctx->scratch_owner)"};
}
}  // namespace

// The scratch buffers are sized here and nowhere else: the claim, then the growth.  `what`
// names the buffer in the text of a failed allocation.
int take(tfhe_hip_ctx *ctx, hipStream_t s, ScratchBuf &b, size_t bytes, bool exact, const char *what) {
  const HipErr r = ctx->scratch.take(s, b, bytes, exact);
  if (r && !r.what) return fail(ctx, TFHE_HIP_ENOMEM, std::string(what) + hipGetErrorString(r.e));
  return hip_rc(ctx, r);
}

namespace {
// launches with per-ciphertext gate codes: placeholders, the kernel reads the codes; cb != 0 keeps in_b attached
constexpr GatePrep kCodesPrep{1u, 1u, 0u};

bool gate_prep(int gate, GatePrep &g) {
  if (gate < 0 || (uint32_t)gate >= kGateCount) return false;
  g = kGateTable[gate];
  return true;
}

// Small calls are arriving at this context's front end (combine.hpp; defined after it): bulk launches then go out in
// chunks, so that a merged launch waits for a chunk boundary and not for the whole batch.
bool comb_interactive(const tfhe_hip_ctx *ctx);
// A one-ciphertext call made while a 65,536-ciphertext launch holds every CU waits for all of it (median 13 ms, p90 308 ms:
// the latency kernel's workgroup needs a whole CU and the batch kernel refills every slot the moment it frees; stream
// priority changes nothing).  Cut into launches of 8,192 ciphertexts the batch costs 1.7 % more (190.6 vs 193.9 k
// bootstraps/s) and the small call waits 39 ms in the median, 50 ms at p90 (16,384: 0.6 %, 70 / 90 ms; 4,096: 5 %, 19 / 23 ms
// -- profiles/exp/logs/r6r_bulk_chunks.log).  Done only while small calls have arrived within the last 250 ms.
constexpr size_t kYieldChunk = 8192;
constexpr int64_t kYieldWindowNs = 250 * 1000 * 1000;

typedef void (*br_kernel_t)(BlindRotateArgs);

// ---- which blind-rotation kernels a batch of `count` runs on ----------------------------------------
// Three kernels, one arithmetic (the same per-element operations in the same order: results are the same bits
// whichever runs, tests/test_gpu_parity.py::test_dispatch_crossovers_bit_exact):
//   BATCH   k_blind_rotate        one wave per ciphertext, four per workgroup: the throughput kernel
//   SINGLE  k_blind_rotate_wide2  one eight-wave workgroup per ciphertext: the latency kernel
//   PAIR    k_blind_rotate_pair   two ciphertexts per eight-wave workgroup, half a step apart
// A plan is at most two launches over contiguous parts of the batch.
enum BrKind { BR_BATCH = 0, BR_SINGLE = 1, BR_PAIR = 2 };
const char *const kBrKindName[3] = {"batch", "single", "pair"};

// many: the many-LUT instantiation (BlindRotateArgs::lut_shift / n_luts / out_fn_stride) of the same kernel
br_kernel_t br_kernel(const tfhe_hip_ctx *ctx, BrKind kind, bool many = false) {
  return kernel_inst(ctx, many, [&](auto inst) -> br_kernel_t {
    constexpr int L = decltype(inst)::L;
    constexpr bool F = decltype(inst)::FAST, M = decltype(inst)::MANY;
    switch (kind) {
      case BR_PAIR: return k_blind_rotate_pair<L, F, M>;
      case BR_SINGLE: return M ? k_blind_rotate_wide2_many<L, F> : k_blind_rotate_wide2<L, F>;
      default: return M ? k_blind_rotate_many<L, F> : k_blind_rotate<L, F>;
    }
  });
}

typedef void (*ep_kernel_t)(const uint32_t *, const int32_t *, const double2 *, uint32_t, const double2 *, int,
                            uint32_t, uint32_t *);
ep_kernel_t ep_kernel(const tfhe_hip_ctx *ctx) {
  return kernel_inst(ctx, false, [](auto inst) -> ep_kernel_t { return k_external_product<decltype(inst)::L, decltype(inst)::FAST>; });
}
struct BrPlan {
  int nparts = 0;
  BrKind kind[2] = {BR_BATCH, BR_BATCH};
  size_t begin[2] = {0, 0}, count[2] = {0, 0};
  void add(BrKind k, size_t b, size_t c) {
    kind[nparts] = k;
    begin[nparts] = b;
    count[nparts] = c;
    ++nparts;
  }
};

BrPlan plan_blind_rotate(const tfhe_hip_ctx *ctx, size_t count) {
  BrPlan pl;
  if (count == 0) return pl;
  if (ctx->dispatch.br_force) {  // TFHE_HIP_BR_KERNEL: that kernel at every batch size
    pl.add((BrKind)(ctx->dispatch.br_force - 1), 0, count);
    return pl;
  }
  // Small batches, N = #CUs (measured at 128 bit, profiles/exp/logs/r3x_pair_kernel.log, r3o_crossover.log):
  // up to N ciphertexts one workgroup each (2.2 ms); N < count <= 2N two ciphertexts per workgroup, half a step apart
  // (3.6 ms; two rounds of singles take 4.5); up to 3N the first 2N as pairs and the rest as singles (5.8; three
  // rounds of singles 6.4, pairs alone 7.3, the batch kernel 7.0 for anything up to 4N).
  const size_t N1 = ctx->dispatch.pair_lo, N2 = ctx->dispatch.pair_max;
  const bool pairs_on = N2 > N1 && ctx->dispatch.wide_max >= N1;
  if (pairs_on && count > N1 && count <= N2) {
    pl.add(BR_PAIR, 0, count);
    return pl;
  }
  // 2N < count <= 3N: the first 2N as pairs, the rest one per workgroup (not at l = 1, where the batch kernel's first
  // step is cheaper than a pair launch plus a single one: SECURITY_UINT4 4.3 vs 4.9 ms; l = 2: 5.1 vs 5.4, l = 3: 5.8 vs 6.9)
  if (pairs_on && ctx->P.l >= 2 && N2 == 2 * N1 && count > N2 && count <= N2 + N1) {
    pl.add(BR_PAIR, 0, N2);
    pl.add(BR_SINGLE, N2, count - N2);
    return pl;
  }
  if (count <= ctx->dispatch.wide_max) {
    pl.add(BR_SINGLE, 0, count);
    return pl;
  }
  // The batch kernel's time is a staircase with a step every 4N (one more four-wave workgroup per CU: 6.9 / 11.5 /
  // 17.1 / 21.8 ms at 1,024 / 2,048 / 3,072 / 4,096).  A tail of up to 2N ciphertexts above a step is cheaper as a
  // latency-kernel launch of its own (2.2 ms up to N, 3.6 up to 2N) than as a whole further step (1,100: 9.1 vs 10.8
  // ms, 2,200: 14.4 vs 17.9, 3,300: 19.7 vs 22.9); done up to 32N, beyond which the step is a few per cent of the launch.
  // (at l = 1 a pair launch costs as much as the step it would save: tails of up to N only)
  size_t tail = 0;
  if (pairs_on && count <= 32 * N1) {
    const size_t r = count % (4 * N1);
    if (r > 0 && r <= (ctx->P.l == 1 ? N1 : N2) && count > r) tail = r;
  }
  pl.add(BR_BATCH, 0, count - tail);
  if (tail) pl.add(tail <= N1 ? BR_SINGLE : BR_PAIR, count - tail, tail);
  return pl;
}

int launch_blind_rotate(tfhe_hip_ctx *ctx, hipStream_t s, const BrCall &c) {
  const size_t count = c.count;
  const int lut_shift = c.lut_shift;
  if (count == 0) return TFHE_HIP_OK;
  if (count > 0x7FFFFFFFull) return fail(ctx, TFHE_HIP_EINVAL, "count too large");
  // many-LUT (lut_shift > 0): 2^lut_shift extractions per ciphertext, function-major [2^lut_shift][count] rows
  if (lut_shift < 0 || lut_shift > 3) return fail(ctx, TFHE_HIP_EINVAL, "n_luts must be 1, 2, 4 or 8");
  if (((size_t)count << lut_shift) > 0x7FFFFFFFull) return fail(ctx, TFHE_HIP_EINVAL, "n_luts * count too large");
  BlindRotateArgs A;
  A.in_a = c.in_a;
  A.in_b = c.gp.cb ? c.in_b : nullptr;
  A.ca = c.gp.ca;
  A.cb = c.gp.cb;
  A.cconst = c.gp.cconst;
  A.gate_codes = c.gate_codes;
  A.idx_a = c.idx_a;  // row indices (circuit levels): the operand bases stay, the indices are sliced per part
  A.idx_b = c.idx_b;
  A.testvec = c.testvec ? c.testvec : ctx->K->d_testvec;
  A.per_ct_stride = (c.testvec && c.per_ct) ? (size_t)2 * kN : 0;
  A.bsk = ctx->K->d_bsk;
  A.tw = ctx->d_tw;
  A.n = ctx->P.n;
  A.bgbit = ctx->P.bgbit;
  A.offset = ctx->K->offset;
  A.out_trlwe = c.out_trlwe;
  A.out_lv1 = c.out_lv1;
  A.out_ext2 = c.out_ext2;
  A.count = count;
  A.lut_shift = lut_shift;
  A.n_luts = 1 << lut_shift;
  A.out_fn_stride = count;  // the whole call's: part() moves the output bases, not the stride
  const bool many = lut_shift > 0;
  A.clk = ctx->profiling ? ctx->d_diag : nullptr;
  A.err_flag = reinterpret_cast<uint32_t *>(ctx->d_diag + 2);
  // sample_extract_index_2 reads a[n - i] of an N-coefficient polynomial (trlwe.rs:122-136): the reference
  // indexes out of bounds (panics) for n > N; refuse instead of reading the b half of the accumulator
  if (c.out_ext2 && ctx->P.n > kN)
    return fail(ctx, TFHE_HIP_EINVAL, "bootstrap without key switch needs n <= N (sample_extract_index_2)");
  if (c.gp.cb && !c.in_b) return fail(ctx, TFHE_HIP_EINVAL, "second gate operand is NULL");
  // ciphertexts [done, done + m) of this call as a launch of their own
  auto part = [&](size_t done, size_t m) {
    BlindRotateArgs S = A;
    if (A.idx_a) S.idx_a = A.idx_a + done;
    else S.in_a = A.in_a + done * (size_t)(ctx->P.n + 1);
    if (A.idx_b) S.idx_b = A.idx_b + done;
    else if (A.in_b) S.in_b = A.in_b + done * (size_t)(ctx->P.n + 1);
    if (A.gate_codes) S.gate_codes = A.gate_codes + done;
    S.testvec = A.testvec + done * A.per_ct_stride;
    if (A.out_trlwe) S.out_trlwe = A.out_trlwe + done * (size_t)(2 * kN);
    if (A.out_lv1) S.out_lv1 = A.out_lv1 + done * (size_t)(kN + 1);
    if (A.out_ext2) S.out_ext2 = A.out_ext2 + done * (size_t)(ctx->P.n + 1);
    S.count = m;
    return S;
  };
  auto launch = [&](br_kernel_t kern, unsigned grid, unsigned threads, size_t lds, const BlindRotateArgs &S) -> int {
    TimedScope timed(ctx->ev_br, s, ctx->profiling);  // (its pair is closed however the launch goes)
    CHK(hip_rc(ctx, timed.err));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, s, S);
    HIPCHK(ctx, hipGetLastError());
    return hip_rc(ctx, timed.close());
  };
  BrPlan pl = plan_blind_rotate(ctx, count);
  for (int q = 0; q < pl.nparts; ++q) {
    const size_t begin = pl.begin[q], m_all = pl.count[q];
    if (pl.kind[q] == BR_PAIR) {
      CHK(launch(br_kernel(ctx, BR_PAIR, many), (unsigned)((m_all + 1) / 2), 64u * kPairWaves, blind_rotate_pair_lds_bytes(ctx->P.n),
                 part(begin, m_all)));
    } else if (pl.kind[q] == BR_SINGLE) {
      CHK(launch(br_kernel(ctx, BR_SINGLE, many), (unsigned)m_all, 64u * kWide2Waves, blind_rotate_wide2_lds_bytes(ctx->P.n, ctx->P.l),
                 part(begin, m_all)));
    } else {
      // ONE launch of the whole part (unless small calls are arriving: kYieldChunk).  The four waves of a workgroup meet
      // at a barrier every CMUX step (blind_rotate.hpp), which keeps the resident workgroups streaming the key in near
      // lock-step on its own: L1 86 % / L2 97 % hits.
      const size_t chunk = (m_all >= 2 * kYieldChunk && comb_interactive(ctx)) ? kYieldChunk : m_all;
      for (size_t done = 0; done < m_all; done += chunk) {
        const size_t m = (m_all - done < chunk) ? m_all - done : chunk;
        CHK(launch(br_kernel(ctx, BR_BATCH, many), (unsigned)((m + kBrWaves - 1) / kBrWaves), 64u * kBrWaves,
                   blind_rotate_lds_bytes(ctx->P.n), part(begin + done, m)));
      }
    }
  }
  ctx->bootstraps += count;
  return TFHE_HIP_OK;
}

// ---- base-4 key switch on the matrix cores (key_switch_mfma.hpp) -----------------------------------
typedef void (*km_kernel_t)(const uint32_t *, const unsigned char *, int, int, uint32_t *, size_t, unsigned long long *, int);
// instantiated tile counts of the widest column block (32 columns each): 1 .. kKmMaxTiles
int ks_mfma_nt(int n) {
  const int need = ks_mfma_tiles(n);
  return (need >= 1 && need <= kKmMaxTiles) ? need : 0;
}
template <int NT>
km_kernel_t km_kernel_from(int nt) {
  if constexpr (NT > kKmMaxTiles) return nullptr;
  else return nt == NT ? (km_kernel_t)k_key_switch_mfma<NT> : km_kernel_from<NT + 1>(nt);
}
km_kernel_t km_kernel(int nt) { return km_kernel_from<1>(nt); }
bool ks_mfma_possible(const tfhe_hip_params &P) {
  return P.basebit == 2 && P.t >= 6 && P.t <= 13 && ks_mfma_nt(P.n) != 0;
}

// ---- which key-switch kernel a batch of `count` runs on ----------------------------------------------
// Integer arithmetic: every kernel returns the same bits (trgsw.rs:332-360).
//   MFMA     k_key_switch_mfma    base 4: one-hot byte-plane contraction on the int8 matrix cores
//   SLICED   k_key_switch_sliced  wider bases: 64-column slices of all `base` candidate rows through an LDS ring
//   B4       k_key_switch_b4      base 4 without the matrix cores: candidate rows through a wave-private LDS ring
//   GENERIC  k_key_switch         any set: buffer loads, 32 ciphertexts per workgroup
//   SPLIT    k_key_switch_split   small batches: one ciphertext's walk cut over 32 workgroups
// MFMA, SPLIT and SLICED with K chunks merge partial sums with integer atomics into a zeroed output: `atomics`.
enum KsKind { KS_MFMA = 0, KS_SLICED = 1, KS_B4 = 2, KS_GENERIC = 3, KS_SPLIT = 4 };
const char *const kKsKindName[5] = {"mfma", "sliced", "b4", "generic", "split"};
struct KsPlan {
  KsKind kind = KS_GENERIC;
  int kparts = 1;  // MFMA: K chunks per row block; SLICED: K chunks (grid.z)
  int sets = 0;    // SLICED: accumulator sets per lane
  bool atomics = false;
};

// column-sliced kernel (second form): bases 16 .. 128, its ring + stage within a CU's LDS
bool ks_sliced_fits(const tfhe_hip_params &P) {
  return P.basebit >= 4 && P.basebit <= 7 && ks_sl2_lds_bytes(P.basebit, 36, ks_sl2_rp(P.basebit)) <= 160 * 1024;
}
constexpr size_t kKsSl2Slab = 131072;  // ciphertexts per launch of the column-sliced kernel (bounds its digit scratch: 0.4 GB at t = 3)
typedef void (*sl2_kernel_t)(const uint32_t *, size_t, const uint32_t *, const unsigned char *, int, int, uint32_t *, size_t);
template <int BB>
sl2_kernel_t sl2_kernel_sets(int sets) {
  constexpr int RP = ks_sl2_rp(BB);
  switch (sets) {
    case 24: return k_key_switch_sliced<BB, 24, RP>;
    case 28: return k_key_switch_sliced<BB, 28, RP>;
    case 36: return k_key_switch_sliced<BB, 36, RP>;
    default: return k_key_switch_sliced<BB, 32, RP>;
  }
}
sl2_kernel_t sl2_kernel(int basebit, int sets) {
  switch (basebit) {
    case 4: return sl2_kernel_sets<4>(sets);
    case 5: return sl2_kernel_sets<5>(sets);
    case 6: return sl2_kernel_sets<6>(sets);
    default: return sl2_kernel_sets<7>(sets);
  }
}
// Accumulator sets per lane, chosen per launch so that the grid fills whole rounds of the machine: a workgroup's time is
// proportional to S, the grid is ceil(count / 16S) x slices workgroups, `slots` of them run at once, so the launch
// costs ceil(grid / slots) x S (SECURITY_UINT4, 65,536 ciphertexts, 13 slices, 512 slots: S = 32 is 3.25 rounds = 4 x 32,
// S = 36 is 2.9 rounds = 3 x 36; base 64 / 128 run ONE eight-wave workgroup per CU, 256 slots: SECURITY_UINT7, 19
// slices: S = 32 is 4.75 rounds = 5 x 32 -- 15.8 ms measured, 16.8 / 17.8 at 36 / 28) -- profiles/exp/logs/r4_ks_sl_ablation.log.
int ks_sl2_pick_sets(int basebit, size_t count, int slices, int slots) {
  int best = basebit == 7 ? 36 : basebit == 6 ? 28 : 32;
  size_t best_cost = ~(size_t)0;
  for (int sets : {24, 28, 32, 36}) {
    const size_t grid = ((count + (size_t)ks_sl2_cts(basebit, sets) - 1) / (size_t)ks_sl2_cts(basebit, sets)) * (size_t)slices;
    const size_t cost = ((grid + (size_t)slots - 1) / (size_t)slots) * (size_t)sets;
    if (cost < best_cost || (cost == best_cost && sets == 32)) {
      best = sets;
      best_cost = cost;
    }
  }
  return best;
}
bool ks_b4_fits(const tfhe_hip_params &P) {
  const int bd = ((ksk_row_words(P.n) >> 2) + 63) & ~63;
  return P.basebit == 2 && ks_b4_lds_bytes(bd >> 6, kKsG) <= 64 * 1024;
}
bool ks_kind_possible(const tfhe_hip_params &P, KsKind k) {
  switch (k) {
    case KS_MFMA: return ks_mfma_possible(P);
    case KS_SLICED: return ks_sliced_fits(P);
    case KS_B4: return ks_b4_fits(P);
    default: return true;
  }
}

KsPlan plan_key_switch(const tfhe_hip_ctx *ctx, size_t count) {
  const tfhe_hip_params &P = ctx->P;
  const int n = P.n;
  KsPlan pl;
  const bool forced = ctx->dispatch.ks_force != 0;
  // base-4 sets from 64 ciphertexts up: the matrix-core kernel, its walk over K cut into chunks while the batch is
  // too small to fill the chip with row blocks (0.10 / 0.11 / 0.15 / 0.18 / 0.25 / 0.40 ms at 64 / 256 / 512 / 1,024 /
  // 2,048 / 4,096 ciphertexts; the split kernel takes 0.12 / 0.33 / 0.55 / 0.97 / 1.8 / 3.6, the matrix-core kernel
  // without chunks 0.42-0.49 throughout: profiles/exp/logs/r3_ks_splitk.log).
  // Wider bases from 384 ciphertexts up: the column-sliced kernel with its walk over the coefficients cut into chunks
  // (SECURITY_UINT4: 0.37 / 0.37 / 0.57 / 1.05 ms at 512 / 1,024 / 2,048 / 4,096 ciphertexts where the split kernel
  // takes 0.46 / 0.85 / 1.62 / 3.42 and wins below: 0.27 vs 0.29 at 256 -- profiles/exp/logs/r3_ks_sl_chunks.log).
  // Smaller batches, and whatever neither LDS kernel covers, up to ks_split_max: the split kernel.
  if (forced) pl.kind = (KsKind)(ctx->dispatch.ks_force - 1);
  else if (ctx->K->d_ksk8 && count >= ctx->dispatch.ks_mfma_min) pl.kind = KS_MFMA;
  else {
    const bool sliced_ok = ks_sliced_fits(P);
    if (count <= ctx->dispatch.ks_split_max && !(sliced_ok && count >= ctx->dispatch.ks_sl_chunk_min)) pl.kind = KS_SPLIT;
    else if (sliced_ok) pl.kind = KS_SLICED;
    else if (ks_b4_fits(P)) pl.kind = KS_B4;
    else pl.kind = KS_GENERIC;
  }
  if (pl.kind == KS_MFMA) {
    // one workgroup per (128 rows, column block, byte plane, K chunk); small batches have few row blocks: the walk over
    // K is cut into up to 16 chunks so that there are about two workgroups per CU to run
    const size_t rb = (count + kKmRows - 1) / kKmRows;
    const int tiles = ks_mfma_total_tiles(n);
    const size_t ncb = (size_t)(tiles < kKmColBlocks ? tiles : kKmColBlocks);
    int ksplit = 1;
    while (ksplit < 16 && rb * ncb * 4 * (size_t)ksplit < 2 * (size_t)ctx->num_cus) ksplit *= 2;
    pl.kparts = ksplit;
    pl.atomics = true;
  } else if (pl.kind == KS_SLICED) {
    // accumulator sets per lane: whichever fills whole rounds of the machine (workgroups resident at once: two per CU
    // while two rings fit a CU's LDS, else one)
    const int slices = (n + 1 + 63) / 64, rp = ks_sl2_rp(P.basebit);
    const size_t in_launch = count < kKsSl2Slab ? count : kKsSl2Slab;
    // workgroups resident per CU: two waves per SIMD by registers (8 wave slots), and the rings must fit the LDS
    const int by_waves = 8 / ks_sl2_waves(P.basebit), by_lds = 2 * ks_sl2_lds_bytes(P.basebit, 36, rp) <= 160 * 1024 ? 2 : 1;
    const int per_cu = by_waves < by_lds ? by_waves : by_lds;
    const int sets = ks_sl2_pick_sets(P.basebit, in_launch, slices, per_cu * ctx->num_cus);
    // small batches have few ciphertext groups: the walk over the N * t groups is cut into up to 64 chunks (grid.z)
    // so that about two workgroups per CU exist; the chunks meet in the zeroed output through integer atomics.
    // A chunk is whole rings (2 * rp groups).
    const size_t groups = (in_launch + (size_t)ks_sl2_cts(P.basebit, sets) - 1) / (size_t)ks_sl2_cts(P.basebit, sets);
    int kchunks = 1;
    while (kchunks < 64 && groups * (size_t)slices * (size_t)kchunks < 2 * (size_t)ctx->num_cus) kchunks *= 2;
    while (kchunks > 1 && (kN * P.t / kchunks) % (2 * rp) != 0) kchunks /= 2;
    pl.sets = sets;
    pl.kparts = kchunks;
    pl.atomics = kchunks > 1;
  } else if (pl.kind == KS_SPLIT) {
    pl.kparts = 32;
    pl.atomics = true;
  }
  return pl;
}

// (re)build the byte planes from the u32 engine key; called where a key becomes current (key_change.hpp's commits)
int build_ksk_planes(tfhe_hip_ctx *ctx) {
  if (!ks_mfma_possible(ctx->P) || (ctx->dispatch.ks_force && ctx->dispatch.ks_force - 1 != KS_MFMA)) return TFHE_HIP_OK;
  const tfhe_hip_params &P = ctx->P;
  const size_t bytes = ks_mfma_key_bytes(P.n, P.t);
  CHK(alloc_exact(ctx, ctx->K->d_ksk8, bytes + kKmKeyTailPad, "hipMalloc((void **)&ctx->K->d_ksk8, bytes + kKmKeyTailPad)"));
  const size_t chunks = bytes / 16;
  hipLaunchKernelGGL(k_ksk_planes, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, ctx->stream, ctx->K->d_ksk,
                     ctx->K->d_ksk8, P.n, P.t, chunks);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return TFHE_HIP_OK;
}
}  // namespace

int launch_key_switch(tfhe_hip_ctx *ctx, hipStream_t s, const uint32_t *lv1, uint32_t *out, size_t count) {
  if (count == 0) return TFHE_HIP_OK;
  CHK(claim_scratch(ctx, s));  // (whether or not ks_out or ks_dig is taken below: what is synchronised does not depend on the plan)
  const tfhe_hip_params &P = ctx->P;
  const int n = P.n;
  const KsPlan pl = plan_key_switch(ctx, count);
  if (pl.kind == KS_MFMA && !ctx->K->d_ksk8) return fail(ctx, TFHE_HIP_EINVAL, "matrix-core key switch: byte planes not built");
  const size_t obytes = count * (size_t)(n + 1) * 4;
  // Kernels that merge partial sums with integer atomics need a zeroed DEVICE destination: a host (pinned, zero-copy)
  // output would take the atomics over PCIe, which not every root complex completes (AtomicOps are optional), and
  // silently returns wrong words where it does not -- such outputs go through a device buffer and leave in one copy.
  uint32_t *dst = out;
  bool host_out = false;
  if (pl.atomics) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, (const void *)out) != hipSuccess) {
      (void)hipGetLastError();
      return fail(ctx, TFHE_HIP_EINVAL, "key switch output is not GPU-addressable memory");
    }
    if (at.type == hipMemoryTypeHost) {
      host_out = true;
      CHK(take(ctx, s, ctx->ks_out, obytes));
      dst = (uint32_t *)ctx->ks_out.p;
    }
  }
  if (pl.kind == KS_SLICED) {
    const size_t in_launch = count < kKsSl2Slab ? count : kKsSl2Slab;
    CHK(take(ctx, s, ctx->ks_dig, (size_t)(kN * P.t / 4) * ks_sl2_ct_stride(in_launch, P.basebit, pl.sets) * 4));
  }
  const int rw4 = ksk_row_words(n) >> 2;
  const int bd = (rw4 + 63) & ~63;  // <= 320 for n <= 1279
  const size_t ksk_bytes = (size_t)kN * P.t * (1u << P.basebit) * ksk_row_words(n) * 4;
  TimedScope timed(ctx->ev_ks, s, ctx->profiling);  // (its pair is closed whichever way the launches go)
  CHK(hip_rc(ctx, timed.err));
  if (pl.atomics) HIPCHK(ctx, hipMemsetAsync(dst, 0, obytes, s));
  switch (pl.kind) {
    case KS_MFMA: {
      const int nt = ks_mfma_nt(n);
      const size_t rb = (count + kKmRows - 1) / kKmRows;
      const int tiles = ks_mfma_total_tiles(n);
      const unsigned ncb = (unsigned)(tiles < kKmColBlocks ? tiles : kKmColBlocks);
      hipLaunchKernelGGL(km_kernel(nt), dim3((unsigned)rb * (unsigned)pl.kparts, ncb, 4), dim3(64 * kKmWaves),
                         ks_mfma_lds_bytes(nt), s, lv1, (const unsigned char *)ctx->K->d_ksk8, n, P.t, dst, count,
                         ctx->profiling ? ctx->d_diag + 4 : nullptr, pl.kparts);
      break;
    }
    case KS_SPLIT:
      // small batch: split each ciphertext's walk over 32 workgroups, merge with integer atomics
      hipLaunchKernelGGL(k_key_switch_split, dim3((unsigned)count, (unsigned)pl.kparts), dim3(bd), 0, s, lv1,
                         (const uint4 *)ctx->K->d_ksk.p, (uint32_t)ksk_bytes, n, P.basebit, P.t, dst);
      break;
    case KS_SLICED: {
      // digits first (k_ks_digits: one byte per (ciphertext, group), [quad of groups][ciphertext]), then the walk;
      // slabs of kKsSl2Slab ciphertexts bound the digit scratch
      const int slices = (n + 1 + 63) / 64, rp = ks_sl2_rp(P.basebit);
      const size_t lds = ks_sl2_lds_bytes(P.basebit, pl.sets, rp);
      const sl2_kernel_t kern = sl2_kernel(P.basebit, pl.sets);
      const unsigned quads = (unsigned)(kN * P.t / 4);
      for (size_t done = 0; done < count; done += kKsSl2Slab) {
        const size_t m = count - done < kKsSl2Slab ? count - done : kKsSl2Slab;
        const size_t ct_stride = ks_sl2_ct_stride(m, P.basebit, pl.sets);
        const uint32_t *src = lv1 + done * (size_t)(kN + 1);
        hipLaunchKernelGGL(k_ks_digits, dim3((unsigned)((ct_stride + 63) / 64), quads / 32), dim3(256), 0, s, src,
                           (uint32_t *)ctx->ks_dig.p, ct_stride, m, P.basebit, P.t);
        const size_t groups = (m + (size_t)ks_sl2_cts(P.basebit, pl.sets) - 1) / (size_t)ks_sl2_cts(P.basebit, pl.sets);
        hipLaunchKernelGGL(kern, dim3((unsigned)groups, (unsigned)slices, (unsigned)pl.kparts), dim3(64u * (unsigned)ks_sl2_waves(P.basebit)), lds, s,
                           (const uint32_t *)ctx->ks_dig.p, ct_stride, src, (const unsigned char *)ctx->K->d_ksk.p, n, P.t,
                           dst + done * (size_t)(n + 1), m);
      }
      break;
    }
    case KS_B4:
      hipLaunchKernelGGL((k_key_switch_b4<kKsG>), dim3((unsigned)((count + kKsG - 1) / kKsG)), dim3(bd),
                         ks_b4_lds_bytes(bd >> 6, kKsG), s, lv1, (const unsigned char *)ctx->K->d_ksk.p, n, P.t, dst, count);
      break;
    default:
      hipLaunchKernelGGL((k_key_switch<kKsG>), dim3((unsigned)((count + kKsG - 1) / kKsG)), dim3(bd), 0, s, lv1,
                         (const uint4 *)ctx->K->d_ksk.p, (uint32_t)ksk_bytes, n, P.basebit, P.t, dst, count);
      break;
  }
  HIPCHK(ctx, hipGetLastError());
  if (host_out) HIPCHK(ctx, hipMemcpyAsync(out, dst, obytes, hipMemcpyDefault, s));
  return hip_rc(ctx, timed.close());
}

int need_key(tfhe_hip_ctx *ctx) {
  if (!ctx->K->key_loaded) return fail(ctx, TFHE_HIP_ENOKEY, "cloud key not loaded");
  return TFHE_HIP_OK;
}

namespace {
int need_reenc_key(tfhe_hip_ctx *ctx) {
  if (!ctx->K->reenc_loaded) return fail(ctx, TFHE_HIP_ENOKEY, "re-encryption key not loaded");
  return TFHE_HIP_OK;
}
}  // namespace

// ---- device-pointer implementations (mutex held by caller) -------------------

// A bootstrap on stream `s`: the blind rotation `call` describes (everything but its output), then, with `keyswitch`,
// the key switch of its count << lut_shift extracted rows into `out`; without, the rows are extracted straight into
// `out` (bootstrap_without_key_switch).  The one place that takes the context's lv1 scratch for a blind rotation.
int run_bootstrap(tfhe_hip_ctx *ctx, hipStream_t s, BrCall call, uint32_t *out, bool keyswitch) {
  if (!keyswitch) {
    call.out_ext2 = out;
    return launch_blind_rotate(ctx, s, call);
  }
  const size_t rows = call.count << call.lut_shift;
  CHK(take(ctx, s, ctx->lv1, lv1_bytes(rows)));
  call.out_lv1 = (uint32_t *)ctx->lv1.p;
  CHK(launch_blind_rotate(ctx, s, call));
  return launch_key_switch(ctx, s, call.out_lv1, out, rows);
}

namespace {
int gate_dev(tfhe_hip_ctx *ctx, int gate, const uint32_t *a, const uint32_t *b, uint32_t *out,
             size_t count, hipStream_t s) {
  GatePrep gp;
  if (!gate_prep(gate, gp)) return fail(ctx, TFHE_HIP_EINVAL, "unknown gate");
  return run_bootstrap(ctx, s, {.in_a = a, .in_b = b, .gp = gp, .count = count}, out, true);
}

// proxy_reenc::reencrypt_tlwe_lv0 (proxy_reenc.rs:468-510): pad to the key switch's source shape, then the key switch
int reencrypt_dev(tfhe_hip_ctx *ctx, const uint32_t *in, uint32_t *out, size_t count, hipStream_t s) {
  if (count == 0) return TFHE_HIP_OK;
  CHK(take(ctx, s, ctx->lv1, lv1_bytes(count)));
  hipLaunchKernelGGL(k_reenc_pad, dim3((unsigned)count), dim3(256), 0, s, in, (uint32_t *)ctx->lv1.p, ctx->P.n);
  HIPCHK(ctx, hipGetLastError());
  return launch_key_switch(ctx, s, (const uint32_t *)ctx->lv1.p, out, count);
}

}  // namespace

// n_luts in {1, 2, 4, 8} -> log2, else -1
int lut_shift_of(int n_luts) {
  switch (n_luts) {
    case 1: return 0;
    case 2: return 1;
    case 4: return 2;
    case 8: return 3;
    default: return -1;
  }
}

namespace {
// the checks of the many-LUT entry points, in one order for the host, device and pool forms: why the call is
// TFHE_HIP_EINVAL, or nullptr (the context forms file the text under the context, the pool forms under the pool)
const char *many_refusal(const uint32_t *a, uint32_t cb, const uint32_t *b, const uint32_t *testvec, int n_luts,
                         const uint32_t *out, size_t count) {
  const int shift = lut_shift_of(n_luts);
  if (shift < 0) return "n_luts must be 1, 2, 4 or 8";
  if (!testvec) return "many-LUT bootstrap needs a test vector";
  if (cb && !b) return "null pointer";
  if (count && (!a || !out)) return "null pointer";
  if ((count << shift) > 0x7FFFFFFFull || count > 0x7FFFFFFFull) return "n_luts * count too large";
  return nullptr;
}

int lincomb_dev(tfhe_hip_ctx *ctx, GatePrep gp, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t count,
                hipStream_t s) {
  if (count == 0) return TFHE_HIP_OK;
  const size_t total = count * (size_t)(ctx->P.n + 1);
  hipLaunchKernelGGL(k_tlwe_lincomb, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, gp.ca, a,
                     gp.cb, gp.cb ? b : nullptr, gp.cconst, out, (uint32_t)(ctx->P.n + 1), total);
  HIPCHK(ctx, hipGetLastError());
  return TFHE_HIP_OK;
}

int mux_dev(tfhe_hip_ctx *ctx, int naive, const uint32_t *a, const uint32_t *b, const uint32_t *c,
            uint32_t *out, size_t count, hipStream_t s) {
  CHK(take(ctx, s, ctx->u1, tlwe_bytes(ctx, count)));
  CHK(take(ctx, s, ctx->u2, tlwe_bytes(ctx, count)));
  uint32_t *u1 = (uint32_t *)ctx->u1.p, *u2 = (uint32_t *)ctx->u2.p;
  GatePrep g_and, g_andny;
  gate_prep(TFHE_HIP_AND, g_and);
  gate_prep(TFHE_HIP_ANDNY, g_andny);  // and(not(a), c) = -a + c - 1/8  (gates.rs:172-175, 196-197)
  if (naive) {  // gates.rs:189-199
    CHK(gate_dev(ctx, TFHE_HIP_AND, a, b, u1, count, s));
    CHK(gate_dev(ctx, TFHE_HIP_ANDNY, a, c, u2, count, s));
    return gate_dev(ctx, TFHE_HIP_OR, u1, u2, out, count, s);
  }
  // gates.rs:157-183: two bootstrap_without_key_switch, add, one full bootstrap
  CHK(run_bootstrap(ctx, s, {.in_a = a, .in_b = b, .gp = g_and, .count = count}, u1, false));
  CHK(run_bootstrap(ctx, s, {.in_a = a, .in_b = c, .gp = g_andny, .count = count}, u2, false));
  return gate_dev(ctx, TFHE_HIP_OR, u1, u2, out, count, s);
}

// host staging helpers
// Pool members (several contexts fed from one host by one thread each) stage pageable operands through a pinned
// arena of their own: the member's thread copies its slice with memcpy, the DMA engine takes it from there, and
// no two members meet in the runtime's single pageable-copy staging path.  A lone context keeps the runtime's
// pipelined pageable copy (one thread cannot memcpy 550 MB faster than that).
bool via_pin(tfhe_hip_ctx *ctx, Staging &s, size_t bytes) {  // (no arena: the caller falls back to the pageable copy)
  return ctx->stage_pinned && s.pool_pinned && bytes >= (1u << 20) && s.pin.grow(bytes, false);
}

}  // namespace

int to_dev(tfhe_hip_ctx *ctx, Staging &s, const void *src, size_t bytes) {
  CHK(ensure(ctx, s.dev, bytes));
  if (via_pin(ctx, s, bytes)) {
    memcpy(s.pin.p, src, bytes);
    src = s.pin.p;
  }
  HIPCHK(ctx, hipMemcpyAsync(s.dev.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  return TFHE_HIP_OK;
}

int to_host(tfhe_hip_ctx *ctx, void *dst, Staging &s, size_t bytes) {
  if (via_pin(ctx, s, bytes)) {
    HIPCHK(ctx, hipMemcpyAsync(s.pin.p, s.dev.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(dst, s.pin.p, bytes);
    return TFHE_HIP_OK;
  }
  HIPCHK(ctx, hipMemcpyAsync(dst, s.dev.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return TFHE_HIP_OK;
}

// Zero-copy for pinned host buffers: memory from tfhe_hip_host_alloc (hipHostMalloc) or registered with
// hipHostRegister is addressable by the GPU, so the host entry points hand such buffers to the kernels as they
// are -- each ciphertext is read once in the blind rotation's prologue and written once by the key switch, and
// those PCIe transactions spread over the whole launch instead of three staging copies around it.
// Returns the device view of `p`, or nullptr when `p` is ordinary pageable memory.
void *pinned_view(const void *p, size_t bytes) {
  if (!p) return nullptr;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, (const void *)p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory is "invalid value" to the runtime: not an error here
    return nullptr;
  }
  if (at.type != hipMemoryTypeHost) return nullptr;
  // the LAST byte must belong to the same pinned allocation / registration as the first: a range registered
  // shorter than the operand (or an interior pointer near the end of one) would fault in the kernel, where the
  // staged path works -- so such operands are staged
  if (bytes > 1) {
    hipPointerAttribute_t last;
    const void *q = (const void *)((const unsigned char *)p + bytes - 1);
    if (hipPointerGetAttributes(&last, q) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    if (last.type != hipMemoryTypeHost) return nullptr;
    void *b0 = nullptr, *b1 = nullptr;
    size_t s0 = 0, s1 = 0;
    if (hipMemGetAddressRange((hipDeviceptr_t *)&b0, &s0, (hipDeviceptr_t)p) == hipSuccess &&
        hipMemGetAddressRange((hipDeviceptr_t *)&b1, &s1, (hipDeviceptr_t)q) == hipSuccess) {
      if (b0 != b1) return nullptr;
    } else {
      (void)hipGetLastError();  // registered (not allocated) memory may have no address range: both ends are host-pinned
    }
  }
  void *d = nullptr;
  if (hipHostGetDevicePointer(&d, (void *)p, 0) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return d;
}

int launched(tfhe_hip_ctx *ctx) {  // status of the kernel launch just made
  HIPCHK(ctx, hipGetLastError());
  return TFHE_HIP_OK;
}

#include "combine.hpp"
#include "key_change.hpp"

namespace {
bool comb_interactive(const tfhe_hip_ctx *ctx) {
  const Combiner *C = ctx->comb;
  if (!C || C->max_count.load(std::memory_order_relaxed) == 0) return false;
  const int64_t t = C->last_arrival_ns.load(std::memory_order_relaxed);
  return t != 0 && combq::now_ns() - t < kYieldWindowNs;
}
}  // namespace

bool params_supported(const tfhe_hip_params *p) {
  return !(p->n < 1 || p->n > 1279 || p->l < 1 || p->l > 3 || p->bgbit < 1 || p->l * p->bgbit > 32 ||
           p->basebit < 1 || p->basebit > 10 || p->t < 1 || p->basebit * p->t > 31 ||
           (double)ksk_bytes(*p) >= 4294967296.0);
}

#if TFHE_ABL_CATALOG
// The catalogue build (experiment.hpp): the names TFHE_HIP_MUTANT may hold, and the selected defect written into every
// unit's device word on the current device.  -1: no such name.
TFHE_MUTANT_PUBLISH(core)
namespace {
#define TFHE_MUTANT_NAME(name) {#name, kMut_##name},
const struct {
  const char *name;
  unsigned id;
} kMutantNames[] = {TFHE_MUTANT_LIST(TFHE_MUTANT_NAME)};
#undef TFHE_MUTANT_NAME
int mutant_lookup(const char *name) {
  if (!name || !*name) return (int)kMutNone;
  for (const auto &e : kMutantNames)
    if (!strcmp(name, e.name)) return (int)e.id;
  return -1;
}
hipError_t mutant_publish(unsigned id) {
  hipError_t e = mutant_publish_core(id);
  if (e == hipSuccess) e = mutant_publish_planes(id);
  if (e == hipSuccess) e = mutant_publish_rings(id);
  return e;
}
}  // namespace
#endif

// =============================================================================
// C ABI
// =============================================================================
extern "C" {

const char *tfhe_hip_name(void) { return TFHE_ABLATED ? "hip-gfx950-EXPERIMENT" : "hip-gfx950"; }

int tfhe_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

const char *tfhe_hip_last_error(const tfhe_hip_ctx *ctx) {
  if (ctx && ctx->parent) ctx = ctx->parent;
  return ctx ? err_text(ctx->id) : g_create_error.c_str();
}

int tfhe_hip_ctx_create(const tfhe_hip_params *p, int device, tfhe_hip_ctx **out) {
  if (!p || !out) {
    g_create_error = "null argument";
    return TFHE_HIP_EINVAL;
  }
  *out = nullptr;
  if (!params_supported(p)) {
    g_create_error = "unsupported parameter set";
    return TFHE_HIP_EINVAL;
  }
  // The supported controls (include/tfhe_hip.h): force ONE kernel at every batch size.  The parity suite uses them to
  // hold every shipped kernel to the CPU checker; they never change result bits.  (Validated before anything is allocated.)
  int br_force = 0, ks_force = 0;
  if (const char *env = getenv("TFHE_HIP_BR_KERNEL")) {
    const std::string v(env);
    if (v == "batch") br_force = BR_BATCH + 1;
    else if (v == "single") br_force = BR_SINGLE + 1;
    else if (v == "pair") br_force = BR_PAIR + 1;
    else if (v != "auto" && !v.empty()) {
      g_create_error = "TFHE_HIP_BR_KERNEL must be auto, batch, single or pair";
      return TFHE_HIP_EINVAL;
    }
    if (br_force == BR_PAIR + 1 && blind_rotate_pair_lds_bytes(p->n) > 160 * 1024) {
      g_create_error = "TFHE_HIP_BR_KERNEL=pair: not available for this parameter set";
      return TFHE_HIP_EINVAL;
    }
  }
  if (const char *env = getenv("TFHE_HIP_KS_KERNEL")) {
    const std::string v(env);
    int k = -1;
    for (int i = 0; i < 5; ++i)
      if (v == kKsKindName[i]) k = i;
    if (k < 0 && v != "auto" && !v.empty()) {
      g_create_error = "TFHE_HIP_KS_KERNEL must be auto, mfma, sliced, b4, generic or split";
      return TFHE_HIP_EINVAL;
    }
    if (k >= 0 && !ks_kind_possible(*p, (KsKind)k)) {
      g_create_error = std::string("TFHE_HIP_KS_KERNEL=") + v + ": not available for this parameter set";
      return TFHE_HIP_EINVAL;
    }
    ks_force = k + 1;
  }
  long combine_env = -1;  // -1: the default (the device's CU count)
  if (const char *env = getenv("TFHE_HIP_COMBINE")) {
    char *end = nullptr;
    const long v = strtol(env, &end, 10);
    if (*env && end && *end == 0 && v >= 0 && v <= (long)Combiner::kBatchCap) combine_env = v;
    else if (*env) {
      g_create_error = "TFHE_HIP_COMBINE must be 0 (off) or the largest call to merge, at most 4096 ciphertexts";
      return TFHE_HIP_EINVAL;
    }
  }
#if TFHE_ABL_CATALOG
  const int mutant = mutant_lookup(getenv("TFHE_HIP_MUTANT"));
  if (mutant < 0) {
    g_create_error = "TFHE_HIP_MUTANT names no defect of the catalogue (csrc/experiment.hpp)";
    return TFHE_HIP_EINVAL;
  }
#endif
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_create_error = std::string("no HIP device: ") + hipGetErrorString(e);
    return TFHE_HIP_EHIP;
  }
  if (device < 0 || device >= ndev) {
    g_create_error = "device ordinal out of range";
    return TFHE_HIP_EINVAL;
  }
  tfhe_hip_ctx *ctx = new tfhe_hip_ctx();
  ctx->P = *p;
  ctx->device = device;
  auto bail = [&](const char *what, hipError_t err) {
    g_create_error = std::string(what) + ": " + hipGetErrorString(err);
    delete ctx;  // (with what it had made so far)
    return TFHE_HIP_EHIP;
  };
  DeviceGuard dg(device);
  if (dg.err != hipSuccess) return bail("hipSetDevice", dg.err);
#if TFHE_ABL_CATALOG
  if ((e = mutant_publish((unsigned)mutant)) != hipSuccess) return bail("hipMemcpyToSymbol(g_tfhe_mutant)", e);
#endif
  if ((e = hipStreamCreateWithFlags(&ctx->stream.s, hipStreamNonBlocking)) != hipSuccess)
    return bail("hipStreamCreate", e);
  if ((e = ctx->d_diag.grow(1024, true)) != hipSuccess) return bail("hipMalloc diagnostics", e);
  if ((e = hipMemset(ctx->d_diag, 0, 1024)) != hipSuccess) return bail("hipMemset diagnostics", e);
  if (hipDeviceGetAttribute(&ctx->rtc_khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || ctx->rtc_khz <= 0)
    ctx->rtc_khz = 100000;
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return bail("hipGetDeviceProperties", e);
  ctx->num_cus = prop.multiProcessorCount;
  const size_t combine_max = combine_env >= 0 ? (size_t)combine_env : 2 * (size_t)ctx->num_cus;
  // pre-rounding magnitude bound: 2l polynomials x N terms x (Bg/2) digit x 2^31 key coefficient
  ctx->dispatch.fast_round = std::log2(2.0 * p->l) + 10.0 + (p->bgbit - 1) + 31.0 < 51.0;
  // crossovers of the automatic dispatch, measured on the 256-CU part and kept as multiples of the CU count:
  // key switch vs the group kernels ~7.8k ciphertexts (base 4, LDS ring), ~4.1k (column-sliced); blind rotation vs the
  // batch kernel (7.0 ms for anything up to 1,024 ciphertexts at 128 bit): the eight-wave form takes 2.2 / 4.5 / 6.6 /
  // 8.5 ms for 1 / 2 / 3 / 4 rounds of one workgroup per CU (profiles/exp/logs/r3o_crossover.log) -- three rounds only
  // at l = 3: at l = 1, 2 the batch kernel's first step (4.3 / 5.4 ms) is cheaper than three rounds of singles (6.2 ms)
  ctx->dispatch.ks_split_max = (p->basebit == 2 ? 28 : 16) * (size_t)ctx->num_cus;
  ctx->dispatch.wide_max = (p->l >= 3 ? 3 : 2) * (size_t)ctx->num_cus;
  ctx->dispatch.pair_lo = (size_t)ctx->num_cus;
  ctx->dispatch.pair_max = 2 * (size_t)ctx->num_cus;
  if (blind_rotate_pair_lds_bytes(p->n) > 160 * 1024) ctx->dispatch.pair_max = 0;  // (n > 1,900: no parameter set)
  ctx->dispatch.br_force = br_force;
  ctx->dispatch.ks_force = ks_force;
  // Dynamic LDS above the 64 KiB default.  The attribute belongs to the (kernel, device), not to the context, and
  // contexts of different n share an instantiation (SECURITY_80/110/128_BIT all run k_blind_rotate<3, true>): it is
  // set to the size for the LARGEST supported n, so the order in which contexts are created cannot lower it below
  // what an earlier context launches with.  (A launch still requests only what its own n needs.)
  {
    constexpr int kMaxN = 1279;  // tfhe_hip_ctx_create's bound
    auto set_lds = [&](const void *kern, size_t bytes) {
      const size_t cap = 160 * 1024;
      return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes < cap ? bytes : cap));
    };
    for (int many = 0; many < 2; ++many)  // the many-LUT instantiations have the same LDS layouts
      for (BrKind kind : {BR_BATCH, BR_SINGLE, BR_PAIR}) {
        if (kind == BR_PAIR && !ctx->dispatch.pair_max) continue;
        const size_t bytes = kind == BR_PAIR     ? blind_rotate_pair_lds_bytes(kMaxN)
                             : kind == BR_SINGLE ? blind_rotate_wide2_lds_bytes(kMaxN, p->l)
                                                 : blind_rotate_lds_bytes(kMaxN);
        if ((e = set_lds((const void *)br_kernel(ctx, kind, many), bytes)) != hipSuccess)
          return bail((std::string("hipFuncSetAttribute(blind rotation: ") + kBrKindName[kind] + (many ? ", many-LUT)" : ")")).c_str(), e);
      }
    if (ks_sliced_fits(*p))
      for (int sets : {24, 28, 32, 36})
        if ((e = set_lds((const void *)sl2_kernel(p->basebit, sets), ks_sl2_lds_bytes(p->basebit, sets, ks_sl2_rp(p->basebit)))) != hipSuccess)
          return bail("hipFuncSetAttribute(k_key_switch_sliced)", e);
    if (ks_mfma_possible(*p)) {  // one instantiation per tile count: its LDS size does not depend on n beyond that
      const int nt = ks_mfma_nt(p->n);
      if ((e = set_lds((const void *)km_kernel(nt), ks_mfma_lds_bytes(nt))) != hipSuccess)
        return bail("hipFuncSetAttribute(k_key_switch_mfma)", e);
    }
  }
  std::vector<double2> tw;
  make_twiddles(tw);
  if ((e = ctx->d_tw.grow(tw.size() * sizeof(double2), true)) != hipSuccess)
    return bail("hipMalloc twiddles", e);
  if ((e = hipMemcpy(ctx->d_tw, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice)) != hipSuccess)
    return bail("hipMemcpy twiddles", e);
  // The combining front end (combine.hpp): host-pointer calls of up to `max_count` ciphertexts from concurrent threads
  // share launches.  Default bound: 2 x #CUs (what the pair kernel runs in one go).  Measured with calls of 512 / 1,024 /
  // 4,096 gates (profiles/exp/logs/r7_combining_bound.log): merging them costs a LONE caller nothing at 512 (4.08 vs 4.16 ms),
  // 2.6 % at 1,024 and 13 % at 4,096 (one thread packs 23 MB), and gives 8 concurrent callers +23 % at 512, +16 % at
  // 1,024 and nothing at 4,096.  TFHE_HIP_COMBINE=0 switches the front end off, any other number is the bound
  // (tfhe_hip_set_combining changes it at run time).
  ctx->comb = new Combiner();
  ctx->comb->max_count = combine_max;
  *out = ctx;
  return TFHE_HIP_OK;
}

namespace {
void free_key(KeyState &k) { k = KeyState(); }
}  // namespace

void tfhe_hip_ctx_destroy(tfhe_hip_ctx *ctx) {
  if (!ctx) return;
  if (ctx->parent) {  // a key view: drain the work that may still read its key, free the key, leave the parent alone
    tfhe_hip_ctx *base = ctx->parent;
    bool last_of_dying = false;
    {
      std::lock_guard<FairMutex> lk(base->mu);
      DeviceGuard dg(base->device);
      // (not drain_key_readers: that returns at the first failed synchronisation, and the key is freed here regardless)
      (void)sync_scratch_owner(base, true);
      if (base->stream) (void)hipStreamSynchronize(base->stream);
      comb_quiesce(base);  // (merged launches run on the lanes' streams)
      free_key(ctx->own);
      last_of_dying = --base->views == 0 && base->dying;
      delete ctx;  // (a view's id keys no text -- its errors are its parent's -- but it is registered as live until here)
    }
    if (last_of_dying) tfhe_hip_ctx_destroy(base);  // the parent was destroyed first: it has waited for its views
    return;
  }
  {
    // Destroyed before its views (the header asks for the opposite order): the views still run on this context's
    // stream, scratch and mutex, so keep it alive until the last of them goes.
    std::lock_guard<FairMutex> lk(ctx->mu);
    if (ctx->views > 0) {
      ctx->dying = true;
      return;
    }
  }
  DeviceGuard dg(ctx->device);
  comb_destroy(ctx);  // the front end's lanes (private sibling contexts) go first
  (void)sync_scratch_owner(ctx, true);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  delete ctx;  // nothing is queued any more: the buffers, arenas and events go, then the stream
}

// ---- key views: several resident cloud keys on ONE context ------------------------------------------------
int tfhe_hip_key_create(tfhe_hip_ctx *ctx, tfhe_hip_ctx **out) {
  if (!out) return TFHE_HIP_EINVAL;
  *out = nullptr;
  if (!ctx) return TFHE_HIP_EINVAL;
  tfhe_hip_ctx *base = ctx->parent ? ctx->parent : ctx;  // a view of a view is a view of the same context
  std::lock_guard<FairMutex> lk(base->mu);
  tfhe_hip_ctx *v = new tfhe_hip_ctx();
  v->P = base->P;
  v->device = base->device;
  v->parent = base;
  ++base->views;
  *out = v;
  return TFHE_HIP_OK;
}

tfhe_hip_ctx *tfhe_hip_key_parent(tfhe_hip_ctx *key) { return key ? (key->parent ? key->parent : key) : nullptr; }

int tfhe_hip_key_is_loaded(tfhe_hip_ctx *ctx) { return flag_is_loaded(ctx, &KeyState::key_loaded); }

int tfhe_hip_load_cloud_key(tfhe_hip_ctx *ctx, const double *bsk, const uint32_t *ksk,
                            uint32_t decomp_offset, const uint32_t *testvec) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (!bsk || !ksk || !testvec) return fail(ctx, TFHE_HIP_EINVAL, "null key pointer");
  CHK(begin_key_change(ctx, KEY_BUF_ALL));
  const tfhe_hip_params &P = ctx->P;
  const size_t polys = bsk_polys(P), rows = ksk_rows(P);
  // bootstrapping key: upload the reference layout, permute + scale on the device
  CHK(upload_through_temp(ctx, "bsk", {{bsk, bsk_bytes(P)}}, 0, [&](void *d_ref) {
    hipLaunchKernelGGL(k_bsk_convert, dim3((unsigned)polys), dim3(512), 0, ctx->stream, (const double *)d_ref, ctx->K->d_bsk, polys, key_scale(ctx->dispatch.fast_round));
    return hipGetLastError();
  }));
  // key-switching key: upload the reference layout, pad rows to 16 B and zero the k == 0 rows
  CHK(upload_through_temp(ctx, "ksk", {{ksk, rows * (size_t)(P.n + 1) * 4}}, 0, [&](void *d_ref) {
    return ksk_convert_launch(ctx, (const uint32_t *)d_ref, rows);
  }));
  HIPCHK(ctx, hipMemcpyAsync(ctx->K->d_testvec, testvec, key_testvec_bytes(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return commit_cloud_key(ctx, decomp_offset);
}

namespace {
// ctx->mu held, ctx's device current
int gen_cloud_key_locked(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha_ksk,
                         double alpha_bsk, const ChaChaKey &rk) {
  if (!key_lv0 || !key_lv1) return fail(ctx, TFHE_HIP_EINVAL, "null key pointer");
  if (!(alpha_ksk >= 0.0) || !(alpha_bsk >= 0.0)) return fail(ctx, TFHE_HIP_EINVAL, "negative noise parameter");
  CHK(begin_key_change(ctx, KEY_BUF_ALL));
  const tfhe_hip_params &P = ctx->P;
  StagedSecrets s(ctx);  // (wiped on every exit path)
  CHK(stage_secrets(ctx, key_lv0, key_lv1, rk, s));
  const auto gen_bsk = kernel_inst(ctx, false, [](auto inst) { return k_gen_bsk<decltype(inst)::L>; });
  hipLaunchKernelGGL(gen_bsk, dim3((unsigned)(P.n * 2 * P.l)), dim3(64), kStageLdsBytes, ctx->stream, s.d_k0, s.d_spec,
                     ctx->d_tw, ctx->K->d_bsk, P.bgbit, alpha_bsk, s.d_rk, key_scale(ctx->dispatch.fast_round));
  HIPCHK(ctx, hipGetLastError());
  CHK(ksk_rows_launch(ctx, s, nullptr, alpha_ksk, nullptr, ctx->K->d_ksk));
  uint32_t off = 0;
  CHK(default_offset_and_testvec(ctx, &off));
  return commit_cloud_key(ctx, off);
}

// 64-bit seed -> 256-bit generator key (SplitMix64): reproducible, and only as strong as the seed
ChaChaKey key_from_seed(uint64_t seed) {
  ChaChaKey k;
  uint64_t x = seed;
  for (int i = 0; i < 4; ++i) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    k.k[2 * i] = (uint32_t)z;
    k.k[2 * i + 1] = (uint32_t)(z >> 32);
  }
  return k;
}
}  // namespace

int tfhe_hip_gen_cloud_key(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha_ksk,
                           double alpha_bsk, uint64_t seed) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  return gen_cloud_key_locked(ctx, key_lv0, key_lv1, alpha_ksk, alpha_bsk, key_from_seed(seed));
}

int tfhe_hip_gen_cloud_key_with_key(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1,
                                    double alpha_ksk, double alpha_bsk, const uint8_t rng_key[32]) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (!rng_key) return fail(ctx, TFHE_HIP_EINVAL, "null generator key");
  GeneratorKey gk;
  CHK(gk.fill(ctx, rng_key));
  return gen_cloud_key_locked(ctx, key_lv0, key_lv1, alpha_ksk, alpha_bsk, gk.k);
}

int tfhe_hip_gen_cloud_key_secure(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1,
                                  double alpha_ksk, double alpha_bsk) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  GeneratorKey gk;
  CHK(gk.fill(ctx, nullptr));  // (a failure is reported on the base context)
  return gen_cloud_key_locked(ctx, key_lv0, key_lv1, alpha_ksk, alpha_bsk, gk.k);
}


int tfhe_hip_export_cloud_key(tfhe_hip_ctx *ctx, double *bsk, uint32_t *ksk, uint32_t *decomp_offset,
                              uint32_t *testvec) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_key(ctx));
  const tfhe_hip_params &P = ctx->P;
  if (bsk) {
    const size_t polys = bsk_polys(P);
    CHK(ensure(ctx, ctx->out.dev, bsk_bytes(P)));
    hipLaunchKernelGGL(k_bsk_export, dim3((unsigned)polys), dim3(512), 0, ctx->stream, ctx->K->d_bsk, (double *)ctx->out.dev.p, polys, 1.0 / key_scale(ctx->dispatch.fast_round));
    HIPCHK(ctx, hipGetLastError());
    CHK(to_host(ctx, bsk, ctx->out, bsk_bytes(P)));
  }
  if (ksk) {
    const size_t rows = ksk_rows(P);
    CHK(ensure(ctx, ctx->out.dev, rows * (size_t)(P.n + 1) * 4));
    HIPCHK(ctx, ksk_export_launch(ctx, (uint32_t *)ctx->out.dev.p, rows));
    CHK(to_host(ctx, ksk, ctx->out, rows * (size_t)(P.n + 1) * 4));
  }
  if (decomp_offset) *decomp_offset = ctx->K->offset;
  if (testvec) {
    HIPCHK(ctx, hipMemcpyAsync(testvec, ctx->K->d_testvec, key_testvec_bytes(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return TFHE_HIP_OK;
}

int tfhe_hip_cloud_key_buffers(tfhe_hip_ctx *ctx, void **bsk, size_t *bsk_bytes, void **ksk, size_t *ksk_bytes,
                               void **testvec, size_t *testvec_bytes, uint32_t *decomp_offset) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(ensure_key_buffers(ctx, KEY_BUF_ALL));
  if (bsk) *bsk = ctx->K->d_bsk;
  if (bsk_bytes) *bsk_bytes = ::bsk_bytes(ctx->P);  // (the parameters carry the header's names, which are the size functions')
  if (ksk) *ksk = ctx->K->d_ksk;
  if (ksk_bytes) *ksk_bytes = ::ksk_bytes(ctx->P);
  if (testvec) *testvec = ctx->K->d_testvec;
  if (testvec_bytes) *testvec_bytes = key_testvec_bytes();
  if (decomp_offset) *decomp_offset = ctx->K->offset;
  return TFHE_HIP_OK;
}

int tfhe_hip_adopt_cloud_key(tfhe_hip_ctx *ctx, uint32_t decomp_offset) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (!ctx->K->d_bsk || !ctx->K->d_ksk || !ctx->K->d_testvec)
    return fail(ctx, TFHE_HIP_EINVAL, "tfhe_hip_adopt_cloud_key before tfhe_hip_cloud_key_buffers");
  // whatever filled the buffers (a peer copy, an RCCL broadcast on another stream) must have finished
  comb_quiesce(ctx);
  HIPCHK(ctx, hipDeviceSynchronize());
  return commit_cloud_key(ctx, decomp_offset);
}

// ---- device-pointer entry points ---------------------------------------------

int tfhe_hip_batch_gate_dev(tfhe_hip_ctx *ctx, int gate, const uint32_t *a, const uint32_t *b,
                            uint32_t *out, size_t count, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count && (!a || !out)) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  return gate_dev(ctx, gate, a, b, out, count, pick(ctx, stream));
}

int tfhe_hip_batch_gates_mixed_dev(tfhe_hip_ctx *ctx, const uint8_t *gates, const uint32_t *a, const uint32_t *b,
                                   uint32_t *out, size_t count, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count && (!gates || !a || !b || !out)) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  return run_bootstrap(ctx, pick(ctx, stream), {.in_a = a, .in_b = b, .gp = kCodesPrep, .count = count, .gate_codes = gates}, out, true);
}

int tfhe_hip_batch_gates_mixed_nks_dev(tfhe_hip_ctx *ctx, const uint8_t *gates, const uint32_t *a, const uint32_t *b,
                                       uint32_t *out, size_t count, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count && (!gates || !a || !b || !out)) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  // (the first level of Gates::mux, gates.rs:165-177)
  return run_bootstrap(ctx, pick(ctx, stream), {.in_a = a, .in_b = b, .gp = kCodesPrep, .count = count, .gate_codes = gates}, out, false);
}

int tfhe_hip_batch_bootstrap_dev(tfhe_hip_ctx *ctx, const uint32_t *in, const uint32_t *testvec,
                                 int per_ct, int keyswitch, uint32_t *out, size_t count,
                                 void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count && (!in || !out)) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  return run_bootstrap(ctx, pick(ctx, stream), {.in_a = in, .testvec = testvec, .per_ct = per_ct, .count = count}, out, keyswitch != 0);
}

int tfhe_hip_batch_tlwe_lincomb_dev(tfhe_hip_ctx *ctx, uint32_t ca, const uint32_t *a, uint32_t cb,
                                    const uint32_t *b, uint32_t cconst, uint32_t *out, size_t count,
                                    void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (count && (!a || !out || (cb && !b))) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  return lincomb_dev(ctx, GatePrep{ca, cb, cconst}, a, b, out, count, pick(ctx, stream));
}

int tfhe_hip_batch_lincomb_bootstrap_dev(tfhe_hip_ctx *ctx, uint32_t ca, const uint32_t *a, uint32_t cb,
                                         const uint32_t *b, uint32_t cconst, const uint32_t *testvec,
                                         int per_ct, int keyswitch, uint32_t *out, size_t count,
                                         void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count && (!a || !out || (cb && !b))) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  return run_bootstrap(ctx, pick(ctx, stream),
                       {.in_a = a, .in_b = b, .gp = {ca, cb, cconst}, .testvec = testvec, .per_ct = per_ct, .count = count}, out,
                       keyswitch != 0);
}

int tfhe_hip_batch_lincomb_bootstrap_many_dev(tfhe_hip_ctx *ctx, uint32_t ca, const uint32_t *a, uint32_t cb,
                                              const uint32_t *b, uint32_t cconst, const uint32_t *testvec, int per_ct,
                                              int n_luts, int keyswitch, uint32_t *out, size_t count, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_key(ctx));
  if (const char *why = many_refusal(a, cb, b, testvec, n_luts, out, count)) return fail(ctx, TFHE_HIP_EINVAL, why);
  // ONE blind rotation per ciphertext with the rotation amounts rounded to multiples of n_luts, then n_luts sample
  // extractions (function-major into lv1 or out) and one key switch over all rows
  return run_bootstrap(ctx, pick(ctx, stream),
                       {.in_a = a, .in_b = b, .gp = {ca, cb, cconst}, .testvec = testvec, .per_ct = per_ct, .count = count,
                        .lut_shift = lut_shift_of(n_luts)},
                       out, keyswitch != 0);
}

int tfhe_hip_batch_blind_rotate_dev(tfhe_hip_ctx *ctx, const uint32_t *in, const uint32_t *testvec,
                                    uint32_t *out_trlwe, size_t count, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count && (!in || !out_trlwe)) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  return launch_blind_rotate(ctx, pick(ctx, stream), {.in_a = in, .testvec = testvec, .count = count, .out_trlwe = out_trlwe});
}

int tfhe_hip_batch_mux_dev(tfhe_hip_ctx *ctx, int naive, const uint32_t *a, const uint32_t *b,
                           const uint32_t *c, uint32_t *out, size_t count, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count && (!a || !b || !c || !out)) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  return mux_dev(ctx, naive, a, b, c, out, count, pick(ctx, stream));
}

// ---- host-pointer entry points -----------------------------------------------

// Small calls (comb_takes) go through the combining front end: the caller checks its own arguments, exactly as the
// direct path below does and in the same order, then queues (combine.hpp).
namespace {
#define COMB_FAIL(base, code, msg)      \
  do {                                  \
    err_slot((base)->id) = (msg);       \
    return (code);                      \
  } while (0)
int comb_gate_call(tfhe_hip_ctx *ctx, int gate, const uint8_t *codes, int keyswitch, const uint32_t *a, const uint32_t *b,
                   const uint32_t *testvec, int per_ct, uint32_t *out, size_t count, const GatePrep *lin = nullptr) {
  tfhe_hip_ctx *base = ctx->parent ? ctx->parent : ctx;
  if (!ctx->own.key_loaded) COMB_FAIL(base, TFHE_HIP_ENOKEY, "cloud key not loaded");
  if (codes) {
    if (!a || !b || !out) COMB_FAIL(base, TFHE_HIP_EINVAL, "null pointer");
    for (size_t i = 0; i < count; ++i)
      if (codes[i] > TFHE_HIP_COPY) COMB_FAIL(base, TFHE_HIP_EINVAL, "unknown gate");
  } else {
    GatePrep gp;
    if (!gate_prep(gate, gp)) COMB_FAIL(base, TFHE_HIP_EINVAL, "unknown gate");
    if (!a || !out || (gp.cb && !b)) COMB_FAIL(base, TFHE_HIP_EINVAL, "null pointer");
  }
  if (!keyswitch && base->P.n > kN)
    COMB_FAIL(base, TFHE_HIP_EINVAL, "bootstrap without key switch needs n <= N (sample_extract_index_2)");
  CombReq r;
  r.key = &ctx->own;
  r.cls = CB_GATES;
  r.gate = gate;
  r.codes = codes;
  r.keyswitch = keyswitch;
  r.a = a;
  r.b = b;
  r.testvec = testvec;
  r.per_ct = per_ct;
  r.out = out;
  r.count = count;
  if (lin) {
    r.lin = true;
    r.lin_ca = lin->ca;
    r.lin_cb = lin->cb;
    r.lin_cconst = lin->cconst;
  }
  return comb_submit(base, r);
}
int comb_mux_call(tfhe_hip_ctx *ctx, int naive, const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *out,
                  size_t count) {
  tfhe_hip_ctx *base = ctx->parent ? ctx->parent : ctx;
  if (!ctx->own.key_loaded) COMB_FAIL(base, TFHE_HIP_ENOKEY, "cloud key not loaded");
  if (!a || !b || !c || !out) COMB_FAIL(base, TFHE_HIP_EINVAL, "null pointer");
  if (!naive && base->P.n > kN)
    COMB_FAIL(base, TFHE_HIP_EINVAL, "bootstrap without key switch needs n <= N (sample_extract_index_2)");
  CombReq r;
  r.key = &ctx->own;
  r.cls = naive ? CB_MUX_NAIVE : CB_MUX;
  r.a = a;
  r.b = b;
  r.c = c;
  r.out = out;
  r.count = count;
  return comb_submit(base, r);
}
int comb_rotate_call(tfhe_hip_ctx *ctx, const uint32_t *in, const uint32_t *testvec, uint32_t *out_trlwe, size_t count) {
  tfhe_hip_ctx *base = ctx->parent ? ctx->parent : ctx;
  if (!ctx->own.key_loaded) COMB_FAIL(base, TFHE_HIP_ENOKEY, "cloud key not loaded");
  CombReq r;
  r.key = &ctx->own;
  r.cls = CB_ROTATE;
  r.a = in;
  r.testvec = testvec;
  r.out = out_trlwe;
  r.count = count;
  return comb_submit(base, r);
}
#undef COMB_FAIL

}  // namespace

int tfhe_hip_batch_gate(tfhe_hip_ctx *ctx, int gate, const uint32_t *a, const uint32_t *b,
                        uint32_t *out, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  if (comb_takes(ctx, count)) return comb_gate_call(ctx, gate, nullptr, 1, a, b, nullptr, 0, out, count);
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count == 0) return TFHE_HIP_OK;
  GatePrep gp;
  if (!gate_prep(gate, gp)) return fail(ctx, TFHE_HIP_EINVAL, "unknown gate");
  if (!a || !out || (gp.cb && !b)) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  const size_t bytes = tlwe_bytes(ctx, count);
  return host_call(ctx, true, {{a, bytes, &ctx->a}, {gp.cb ? b : nullptr, bytes, &ctx->b}}, out, bytes, [&](const void *const *d, void *o) {
    return gate_dev(ctx, gate, u32(d[0]), u32(d[1]), (uint32_t *)o, count, ctx->stream);
  });
}

int tfhe_hip_batch_gates_mixed(tfhe_hip_ctx *ctx, const uint8_t *gates, const uint32_t *a, const uint32_t *b,
                               uint32_t *out, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  if (comb_takes(ctx, count) && gates) return comb_gate_call(ctx, 0, gates, 1, a, b, nullptr, 0, out, count);
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count == 0) return TFHE_HIP_OK;
  if (!gates || !a || !b || !out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  for (size_t i = 0; i < count; ++i)
    if (gates[i] > TFHE_HIP_COPY) return fail(ctx, TFHE_HIP_EINVAL, "unknown gate");
  const size_t bytes = tlwe_bytes(ctx, count);
  CHK(to_dev(ctx, ctx->idx, gates, count));  // one byte per ciphertext: always staged
  return host_call(ctx, true, {{a, bytes, &ctx->a}, {b, bytes, &ctx->b}}, out, bytes, [&](const void *const *d, void *o) {
    return run_bootstrap(ctx, ctx->stream, {.in_a = u32(d[0]), .in_b = u32(d[1]), .gp = kCodesPrep, .count = count, .gate_codes = (const uint8_t *)ctx->idx.dev.p},
                         (uint32_t *)o, true);
  });
}

int tfhe_hip_batch_gates_mixed_nks(tfhe_hip_ctx *ctx, const uint8_t *gates, const uint32_t *a, const uint32_t *b,
                                   uint32_t *out, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  if (comb_takes(ctx, count) && gates) return comb_gate_call(ctx, 0, gates, 0, a, b, nullptr, 0, out, count);
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count == 0) return TFHE_HIP_OK;
  if (!gates || !a || !b || !out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  for (size_t i = 0; i < count; ++i)
    if (gates[i] > TFHE_HIP_COPY) return fail(ctx, TFHE_HIP_EINVAL, "unknown gate");
  const size_t bytes = tlwe_bytes(ctx, count);
  const HostIn in[] = {{a, bytes, &ctx->a}, {b, bytes, &ctx->b}, {gates, count, &ctx->idx}};
  return host_call(ctx, false, in, out, bytes, [&](const void *const *d, void *o) {
    return run_bootstrap(ctx, ctx->stream, {.in_a = u32(d[0]), .in_b = u32(d[1]), .gp = kCodesPrep, .count = count, .gate_codes = (const uint8_t *)d[2]},
                         (uint32_t *)o, false);
  });
}

int tfhe_hip_batch_bootstrap(tfhe_hip_ctx *ctx, const uint32_t *in, const uint32_t *testvec,
                             int per_ct, int keyswitch, uint32_t *out, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  if (comb_takes(ctx, count))
    return comb_gate_call(ctx, TFHE_HIP_COPY, nullptr, keyswitch != 0, in, nullptr, testvec, per_ct, out, count);
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count == 0) return TFHE_HIP_OK;
  if (!in || !out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  const size_t bytes = tlwe_bytes(ctx, count);
  // the test vector is zero-copied on its own when it is pinned, whatever the ciphertexts are
  const size_t tv_bytes = testvec_bytes(per_ct, count);
  const uint32_t *d_tv = u32(pinned_view(testvec, tv_bytes));
  if (testvec && !d_tv) {
    CHK(to_dev(ctx, ctx->tv, testvec, tv_bytes));
    d_tv = u32(ctx->tv.dev.p);
  }
  return host_call(ctx, true, {{in, bytes, &ctx->a}}, out, bytes, [&](const void *const *d, void *o) {
    return run_bootstrap(ctx, ctx->stream, {.in_a = u32(d[0]), .testvec = d_tv, .per_ct = per_ct, .count = count}, (uint32_t *)o, keyswitch != 0);
  });
}

int tfhe_hip_batch_tlwe_lincomb(tfhe_hip_ctx *ctx, uint32_t ca, const uint32_t *a, uint32_t cb,
                                const uint32_t *b, uint32_t cconst, uint32_t *out, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (count == 0) return TFHE_HIP_OK;
  if (!a || !out || (cb && !b)) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  const size_t bytes = tlwe_bytes(ctx, count);
  return host_call(ctx, false, {{a, bytes, &ctx->a}, {cb ? b : nullptr, bytes, &ctx->b}}, out, bytes, [&](const void *const *d, void *o) {
    return lincomb_dev(ctx, GatePrep{ca, cb, cconst}, u32(d[0]), u32(d[1]), (uint32_t *)o, count, ctx->stream);
  });
}

int tfhe_hip_batch_lincomb_bootstrap(tfhe_hip_ctx *ctx, uint32_t ca, const uint32_t *a, uint32_t cb,
                                     const uint32_t *b, uint32_t cconst, const uint32_t *testvec,
                                     int per_ct, int keyswitch, uint32_t *out, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  if (comb_takes(ctx, count) && a && out && (!cb || b)) {
    // small call: it joins the merged launches as a COPY bootstrap whose rows are formed on the device first
    // (k_tlwe_lincomb over the packed rows, one launch per run of requests with the same coefficients)
    const GatePrep lin{ca, cb, cconst};
    return comb_gate_call(ctx, TFHE_HIP_COPY, nullptr, keyswitch != 0, a, cb ? b : nullptr, testvec, per_ct, out, count, &lin);
  }
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count == 0) return TFHE_HIP_OK;
  if (!a || !out || (cb && !b)) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  const size_t bytes = tlwe_bytes(ctx, count);
  const HostIn in[] = {{a, bytes, &ctx->a}, {cb ? b : nullptr, bytes, &ctx->b},
                       {testvec, testvec_bytes(per_ct, count), &ctx->tv}};
  return host_call(ctx, false, in, out, bytes, [&](const void *const *d, void *o) {
    return run_bootstrap(ctx, ctx->stream,
                         {.in_a = u32(d[0]), .in_b = u32(d[1]), .gp = {ca, cb, cconst}, .testvec = u32(d[2]), .per_ct = per_ct, .count = count},
                         (uint32_t *)o, keyswitch != 0);
  });
}

int tfhe_hip_batch_lincomb_bootstrap_many(tfhe_hip_ctx *ctx, uint32_t ca, const uint32_t *a, uint32_t cb,
                                          const uint32_t *b, uint32_t cconst, const uint32_t *testvec, int per_ct,
                                          int n_luts, int keyswitch, uint32_t *out, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;  // (never combined: the merged launches have no many-LUT form)
  ENTER(ctx);
  CHK(need_key(ctx));
  if (const char *why = many_refusal(a, cb, b, testvec, n_luts, out, count)) return fail(ctx, TFHE_HIP_EINVAL, why);
  if (count == 0) return TFHE_HIP_OK;
  const size_t bytes = tlwe_bytes(ctx, count);
  const HostIn in[] = {{a, bytes, &ctx->a}, {cb ? b : nullptr, bytes, &ctx->b},
                       {testvec, testvec_bytes(per_ct, count), &ctx->tv}};
  return host_call(ctx, false, in, out, bytes * (size_t)n_luts, [&](const void *const *d, void *o) {
    return run_bootstrap(ctx, ctx->stream,
                         {.in_a = u32(d[0]), .in_b = u32(d[1]), .gp = {ca, cb, cconst}, .testvec = u32(d[2]), .per_ct = per_ct, .count = count,
                          .lut_shift = lut_shift_of(n_luts)},
                         (uint32_t *)o, keyswitch != 0);
  });
}

int tfhe_hip_batch_blind_rotate(tfhe_hip_ctx *ctx, const uint32_t *in, const uint32_t *testvec,
                                uint32_t *out_trlwe, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  if (comb_takes(ctx, count) && in && out_trlwe)  // small call: merged with the other threads' (combine.hpp)
    return comb_rotate_call(ctx, in, testvec, out_trlwe, count);
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count == 0) return TFHE_HIP_OK;
  if (!in || !out_trlwe) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  const HostIn ops[] = {{in, tlwe_bytes(ctx, count), &ctx->a}, {testvec, trlwe_bytes(1), &ctx->tv}};
  return host_call(ctx, false, ops, out_trlwe, trlwe_bytes(count), [&](const void *const *d, void *o) {
    return launch_blind_rotate(ctx, ctx->stream, {.in_a = u32(d[0]), .testvec = u32(d[1]), .count = count, .out_trlwe = (uint32_t *)o});
  });
}

int tfhe_hip_batch_mux(tfhe_hip_ctx *ctx, int naive, const uint32_t *a, const uint32_t *b,
                       const uint32_t *c, uint32_t *out, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  if (comb_takes(ctx, count)) return comb_mux_call(ctx, naive, a, b, c, out, count);
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count == 0) return TFHE_HIP_OK;
  if (!a || !b || !c || !out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  const size_t bytes = tlwe_bytes(ctx, count);
  return host_call(ctx, true, {{a, bytes, &ctx->a}, {b, bytes, &ctx->b}, {c, bytes, &ctx->c}}, out, bytes, [&](const void *const *d, void *o) {
    return mux_dev(ctx, naive, u32(d[0]), u32(d[1]), u32(d[2]), (uint32_t *)o, count, ctx->stream);
  });
}

// ---- single stages --------------------------------------------------------------

int tfhe_hip_batch_external_product(tfhe_hip_ctx *ctx, const uint32_t *trlwe_in,
                                    const int32_t *bsk_index, uint32_t *trlwe_out, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count == 0) return TFHE_HIP_OK;
  if (!trlwe_in || !bsk_index || !trlwe_out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  for (size_t i = 0; i < count; ++i)
    if (bsk_index[i] < 0 || bsk_index[i] >= ctx->P.n) return fail(ctx, TFHE_HIP_EINVAL, "bsk_index out of range");
  const size_t bytes = trlwe_bytes(count);
  const uint32_t bsk_bytes = (uint32_t)((size_t)ctx->P.n * 2 * ctx->P.l * 2 * kN2 * 16);
  return host_call(ctx, false, {{trlwe_in, bytes, &ctx->a}, {bsk_index, count * 4, &ctx->idx}}, trlwe_out, bytes, [&](const void *const *d, void *o) {
    hipLaunchKernelGGL(ep_kernel(ctx), dim3((unsigned)count), dim3(64), kStageLdsBytes, ctx->stream, u32(d[0]), (const int32_t *)d[1],
                       ctx->K->d_bsk, bsk_bytes, ctx->d_tw, ctx->P.bgbit, ctx->K->offset, (uint32_t *)o);
    return launched(ctx);
  });
}

int tfhe_hip_batch_sample_extract(tfhe_hip_ctx *ctx, const uint32_t *trlwe, int k, uint32_t *out, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (k < 0 || k >= kN) return fail(ctx, TFHE_HIP_EINVAL, "extraction index out of range");
  if (count == 0) return TFHE_HIP_OK;
  if (!trlwe || !out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  return host_call(ctx, false, {{trlwe, trlwe_bytes(count), &ctx->a}}, out, count * (size_t)(kN + 1) * 4, [&](const void *const *d, void *o) {
    hipLaunchKernelGGL(k_sample_extract, dim3((unsigned)count), dim3(256), 0, ctx->stream, u32(d[0]), k, (uint32_t *)o, count);
    return launched(ctx);
  });
}

int tfhe_hip_batch_identity_key_switch(tfhe_hip_ctx *ctx, const uint32_t *tlwe_lv1, uint32_t *out, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_key(ctx));
  if (count == 0) return TFHE_HIP_OK;
  if (!tlwe_lv1 || !out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  CHK(ensure(ctx, ctx->a.dev, lv1_bytes(count)));  // whole 256-row groups readable (k_key_switch_mfma)
  const size_t obytes = tlwe_bytes(ctx, count);
  return host_call(ctx, false, {{tlwe_lv1, count * (size_t)(kN + 1) * 4, &ctx->a}}, out, obytes, [&](const void *const *d, void *o) {
    return launch_key_switch(ctx, ctx->stream, u32(d[0]), (uint32_t *)o, count);
  });
}

// ---- proxy re-encryption (src/proxy_reenc.rs; feature `proxy-reenc` of the reference) -------------------------------
// key [n][t][base][n+1]: ProxyReencryptionKey::key_encryptions (proxy_reenc.rs:224-233, index base*t*i + base*j + k).
// It is stored as a key-switching key whose coefficients n .. N-1 have all-zero rows (never selected: k_reenc_pad).
int tfhe_hip_load_reenc_key(tfhe_hip_ctx *ctx, const uint32_t *key) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (!key) return fail(ctx, TFHE_HIP_EINVAL, "null key pointer");
  const tfhe_hip_params &P = ctx->P;
  // the source rides in the key switch's N-coefficient rows (k_reenc_pad): SECURITY_UINT5 .. 8 (n = 1071 / 1160) do not fit
  if (P.n > kN) return fail(ctx, TFHE_HIP_EINVAL, "proxy re-encryption needs n <= N = 1024 (this parameter set's n is larger)");
  CHK(begin_key_change(ctx, KEY_BUF_KSK));  // (both flags go: the buffer is shared with a cloud key's key-switching key)
  const int base = 1 << P.basebit;
  const size_t rows = (size_t)P.n * P.t * base;
  if (const hipError_t e = hipMemsetAsync(ctx->K->d_ksk, 0, ksk_bytes(P), ctx->stream))
    return fail(ctx, TFHE_HIP_EHIP, std::string("re-encryption key upload: ") + hipGetErrorString(e));
  CHK(upload_through_temp(ctx, "re-encryption key", {{key, rows * (size_t)(P.n + 1) * 4}}, 0, [&](void *d_ref) {
    return ksk_convert_launch(ctx, (const uint32_t *)d_ref, rows);
  }));
  return commit_reenc_key(ctx);
}

int tfhe_hip_reenc_key_is_loaded(tfhe_hip_ctx *ctx) { return flag_is_loaded(ctx, &KeyState::reenc_loaded); }

int tfhe_hip_batch_reencrypt_dev(tfhe_hip_ctx *ctx, const uint32_t *in, uint32_t *out, size_t count, void *stream) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_reenc_key(ctx));
  if (count && (!in || !out)) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  return reencrypt_dev(ctx, in, out, count, pick(ctx, stream));
}

int tfhe_hip_batch_reencrypt(tfhe_hip_ctx *ctx, const uint32_t *in, uint32_t *out, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(need_reenc_key(ctx));
  if (count == 0) return TFHE_HIP_OK;
  if (!in || !out) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  const size_t bytes = tlwe_bytes(ctx, count);
  return host_call(ctx, false, {{in, bytes, &ctx->a}}, out, bytes, [&](const void *const *d, void *o) {
    return reencrypt_dev(ctx, u32(d[0]), (uint32_t *)o, count, ctx->stream);
  });
}

int tfhe_hip_batch_ifft(tfhe_hip_ctx *ctx, double *res, const uint32_t *src, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (count == 0) return TFHE_HIP_OK;
  if (!res || !src) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  return host_call(ctx, false, {{src, count * (size_t)kN * 4, &ctx->a}}, res, count * (size_t)kN * 8, [&](const void *const *d, void *o) {
    hipLaunchKernelGGL(k_ifft, dim3((unsigned)count), dim3(64), kStageLdsBytes, ctx->stream, u32(d[0]), ctx->d_tw, (double *)o);
    return launched(ctx);
  });
}

int tfhe_hip_batch_fft(tfhe_hip_ctx *ctx, uint32_t *res, const double *src, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (count == 0) return TFHE_HIP_OK;
  if (!res || !src) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  return host_call(ctx, false, {{src, count * (size_t)kN * 8, &ctx->a}}, res, count * (size_t)kN * 4, [&](const void *const *d, void *o) {
    hipLaunchKernelGGL(k_fft, dim3((unsigned)count), dim3(64), kStageLdsBytes, ctx->stream, (const double *)d[0], ctx->d_tw, (uint32_t *)o);
    return launched(ctx);
  });
}

int tfhe_hip_batch_poly_mul(tfhe_hip_ctx *ctx, uint32_t *res, const uint32_t *a, const uint32_t *b, size_t count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (count == 0) return TFHE_HIP_OK;
  if (!res || !a || !b) return fail(ctx, TFHE_HIP_EINVAL, "null pointer");
  const size_t bytes = count * (size_t)kN * 4;
  return host_call(ctx, false, {{a, bytes, &ctx->a}, {b, bytes, &ctx->b}}, res, bytes, [&](const void *const *d, void *o) {
    hipLaunchKernelGGL(k_poly_mul, dim3((unsigned)count), dim3(64), kStageLdsBytes, ctx->stream, u32(d[0]), u32(d[1]), ctx->d_tw, (uint32_t *)o);
    return launched(ctx);
  });
}

// ---- measurement ---------------------------------------------------------------

int tfhe_hip_set_profiling(tfhe_hip_ctx *ctx, int enabled) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  if (enabled && !ctx->profiling) {
    HIPCHK(ctx, hipMemsetAsync(ctx->d_diag, 0, 16, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_diag + 4, 0, 16, ctx->stream));
  }
  ctx->profiling = enabled != 0;
  comb_with_idle_lanes(ctx, [&](Combiner &C) {  // the front end's lanes record their launches too
    C.profiling = enabled != 0;
    for (tfhe_hip_ctx *x : C.lane_ctx)
      if (x) x->profiling = enabled != 0;
  });
  return TFHE_HIP_OK;
}

int tfhe_hip_get_kernel_times(tfhe_hip_ctx *ctx, tfhe_hip_kernel_times *out) {
  if (!ctx || !out) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  memset(out, 0, sizeof(*out));
  auto drain = [&](tfhe_hip_ctx *x) -> int {
    CHK(hip_rc(ctx, x->ev_br.drain(out->blind_rotate_ms, &out->blind_rotate_launches)));
    return hip_rc(ctx, x->ev_ks.drain(out->key_switch_ms, &out->key_switch_launches));
  };
  CHK(drain(ctx));
  out->bootstraps = ctx->bootstraps;
  ctx->bootstraps = 0;
  int lane_rc = TFHE_HIP_OK;  // merged launches of small calls ran on the front end's lanes
  comb_with_idle_lanes(ctx, [&](Combiner &C) {
    for (tfhe_hip_ctx *x : C.lane_ctx) {
      if (!x) continue;
      if (lane_rc == TFHE_HIP_OK) lane_rc = drain(x);
      out->bootstraps += x->bootstraps;
      x->bootstraps = 0;
    }
  });
  return lane_rc;
}

// the two sums at d_diag[at], [at + 1] since the last sample
static int clock_sample(tfhe_hip_ctx *ctx, int at, tfhe_hip_clock_sample *out) {
  if (!ctx || !out) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(hip_rc(ctx, sync_scratch_owner(ctx)));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  unsigned long long h[2] = {0, 0};
  const char *const copy = at ? "hipMemcpy(h, ctx->d_diag + 4, 16, hipMemcpyDeviceToHost)" : "hipMemcpy(h, ctx->d_diag, 16, hipMemcpyDeviceToHost)";
  const char *const zero = at ? "hipMemset(ctx->d_diag + 4, 0, 16)" : "hipMemset(ctx->d_diag, 0, 16)";
  CHK(hip_rc(ctx, {hipMemcpy(h, ctx->d_diag + at, 16, hipMemcpyDeviceToHost), copy}));
  CHK(hip_rc(ctx, {hipMemset(ctx->d_diag + at, 0, 16), zero}));
  out->shader_cycles = h[0];
  out->rtc_ticks = h[1];
  out->rtc_mhz = ctx->rtc_khz / 1000.0;
  out->shader_mhz = h[1] ? (double)h[0] / (double)h[1] * out->rtc_mhz : 0.0;
  return TFHE_HIP_OK;
}

int tfhe_hip_get_clock_sample(tfhe_hip_ctx *ctx, tfhe_hip_clock_sample *out) { return clock_sample(ctx, 0, out); }
int tfhe_hip_get_key_switch_clock_sample(tfhe_hip_ctx *ctx, tfhe_hip_clock_sample *out) { return clock_sample(ctx, 4, out); }

int tfhe_hip_describe_dispatch(tfhe_hip_ctx *ctx, size_t count, char *buf, size_t buflen) {
  if (!ctx || !buf || buflen == 0) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  std::string d = "blind_rotate=";
  const BrPlan bp = plan_blind_rotate(ctx, count);
  for (int q = 0; q < bp.nparts; ++q) {
    if (q) d += "+";
    d += std::string(kBrKindName[bp.kind[q]]) + "[" + std::to_string(bp.begin[q]) + "," + std::to_string(bp.begin[q] + bp.count[q]) + ")";
  }
  if (bp.nparts == 0) d += "none";
  d += " key_switch=";
  if (count == 0) d += "none";
  else {
    const KsPlan kp = plan_key_switch(ctx, count);
    d += kKsKindName[kp.kind];
    if (kp.kind == KS_MFMA || kp.kind == KS_SLICED || kp.kind == KS_SPLIT) d += "(k=" + std::to_string(kp.kparts);
    if (kp.kind == KS_SLICED) d += ",sets=" + std::to_string(kp.sets);
    if (kp.kind == KS_MFMA || kp.kind == KS_SLICED || kp.kind == KS_SPLIT) d += ")";
  }
  if (d.size() + 1 > buflen) return fail(ctx, TFHE_HIP_EINVAL, "tfhe_hip_describe_dispatch: buffer too small");
  memcpy(buf, d.c_str(), d.size() + 1);
  return TFHE_HIP_OK;
}

const char *tfhe_hip_rounding_mode(const tfhe_hip_ctx *ctx) {
  if (!ctx) return "none";
  const tfhe_hip_ctx *base = ctx->parent ? ctx->parent : ctx;
  return base->dispatch.fast_round ? "fast" : "general";
}

int tfhe_hip_set_combining(tfhe_hip_ctx *ctx, size_t max_count) {
  if (!ctx) return TFHE_HIP_EINVAL;
  tfhe_hip_ctx *base = ctx->parent ? ctx->parent : ctx;
  if (max_count > Combiner::kBatchCap) {
    err_slot(base->id) = "tfhe_hip_set_combining: at most 4096 ciphertexts per merged call";
    return TFHE_HIP_EINVAL;
  }
  if (base->comb) base->comb->max_count.store(max_count, std::memory_order_relaxed);
  return TFHE_HIP_OK;
}

int tfhe_hip_get_combine_stats(tfhe_hip_ctx *ctx, tfhe_hip_combine_stats *out) {
  if (!ctx || !out) return TFHE_HIP_EINVAL;
  tfhe_hip_ctx *base = ctx->parent ? ctx->parent : ctx;
  memset(out, 0, sizeof(*out));
  Combiner *C = base->comb;
  if (!C) return TFHE_HIP_OK;
  std::lock_guard<std::mutex> lk(C->st_mu);
  out->max_count = C->max_count.load(std::memory_order_relaxed);
  out->launches = C->st_launches;
  out->requests = C->st_requests;
  out->ciphertexts = C->st_units;
  out->max_requests_per_launch = C->st_max_requests;
  out->lingers = C->st_lingers;
  out->linger_us = C->st_linger_us;
  out->pack_us = C->st_pack_us;
  out->gpu_us = C->st_gpu_us;
  out->unpack_us = C->st_unpack_us;
  C->st_launches = C->st_requests = C->st_units = C->st_max_requests = C->st_lingers = 0;
  C->st_linger_us = C->st_pack_us = C->st_gpu_us = C->st_unpack_us = 0;
  return TFHE_HIP_OK;
}

int tfhe_hip_host_alloc(size_t bytes, void **out) {
  if (!out) return TFHE_HIP_EINVAL;
  *out = nullptr;
  if (bytes == 0) return TFHE_HIP_OK;
  const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    g_create_error = std::string("hipHostMalloc: ") + hipGetErrorString(e);
    *out = nullptr;
    return e == hipErrorOutOfMemory ? TFHE_HIP_ENOMEM : TFHE_HIP_EHIP;
  }
  return TFHE_HIP_OK;
}

void tfhe_hip_host_free(void *p) {
  pinned_free(p);
}

int tfhe_hip_synchronize(tfhe_hip_ctx *ctx) {
  if (!ctx) return TFHE_HIP_EINVAL;
  ENTER(ctx);
  CHK(hip_rc(ctx, sync_scratch_owner(ctx, true)));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->scratch.owned = false;
  uint32_t flag = 0;
  HIPCHK(ctx, hipMemcpy(&flag, ctx->d_diag + 2, 4, hipMemcpyDeviceToHost));
  if (flag) {
    HIPCHK(ctx, hipMemset(ctx->d_diag + 2, 0, 8));
    return fail(ctx, TFHE_HIP_EINVAL, "a *_mixed_dev launch saw a gate code outside tfhe_hip_gate (treated as COPY)");
  }
  return TFHE_HIP_OK;
}

}  // extern "C"
#include "pool.hpp"
#include "circuit.hpp"
