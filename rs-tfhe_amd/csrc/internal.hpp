// internal.hpp -- the whole interface between the library's translation units (host code only).
//
// libtfhe_hip.so is linked from several units.  tfhe_hip.hip is the core: the context, the error text, dispatch and
// plans, the blind-rotation and key-switch launches, the cloud-key routes, the batch entry points, the combiner, the
// pool and the circuit scheduler -- and every kernel of blind_rotate.hpp, blind_rotate_wide.hpp, key_switch.hpp,
// key_switch_mfma.hpp and keygen.hpp, the ones bench.py times.  The feature units (planes.hip, rings.hip) hold the
// calls built on top of it, each with the kernels of its own headers.  A feature unit includes this header and the
// feature headers it is made of, nothing else of the library; what it may use of the core is what is declared here:
//   * the types a handle is made of (tfhe_hip_ctx, KeyState and the owners of resources.hpp / secrets.hpp), none of
//     them in an anonymous namespace: they are shared between units;
//   * ENTER / HIPCHK / CHK and the size helpers;
//   * the templates whose callers instantiate them (kernel_inst, host_call, upload_through_temp, encrypt_host_call);
//   * the functions that are defined once, in the unit named beside them.
// Everything declared here has hidden visibility: the shared library exports include/tfhe_hip.h and nothing of this.
// State exists once, in tfhe_hip.hip: the per-thread error tables, the live-handle set, the handle id counter, the
// creation error, the RCCL table and the combiner are reached through the functions below or not at all.
//
// Every kernel instantiation is emitted by exactly one unit.  Where two units need the same kernel they go through
// one host function of the unit that owns it (lwe_rows_launch, stage_secrets, derive_public_seed, ksk_convert_launch,
// ksk_export_launch, key_spectrum_launch here; polymul_dev of planes.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <tuple>
#include <atomic>
#include <condition_variable>
#include <initializer_list>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/tfhe_hip.h"
#include "experiment.hpp"

// The core's kernel headers hold, beside the kernels, the device functions, types and constants the feature kernels
// are built from (ChaChaKey, LweRowJob, natural_mask, row_noise, add_ring_product, the FFT passes, the matrix-core
// fragment types).  Some of their kernels are plain functions, not templates, and a second definition of those would
// not link.  tfhe_hip.hip, which owns the kernels, includes the files itself (TFHE_HIP_CORE_UNIT); in every other unit
// what they declare gets internal linkage: no host stub is emitted (nothing there launches these kernels:
// tests/test_host_logic.py holds the objects to that), and the unit's code object carries an unused copy of the plain
// ones.  (The files themselves are byte-stable: bench.py stamps its results with their hash.)
#ifndef TFHE_HIP_CORE_UNIT
#pragma clang attribute push(__attribute__((internal_linkage)), apply_to = function)
#include "keygen.hpp"  // (blind_rotate.hpp, key_switch.hpp, fft512.hpp)
#include "key_switch_mfma.hpp"
#pragma clang attribute pop
#endif

using namespace tfhe;

#pragma GCC visibility push(hidden)

#include "resources.hpp"  // DevBuf, PinBuf, Staging, the scratch claim, the timing pairs: each frees itself
#include "secrets.hpp"    // SecretStage and scrub over them

// ---- error text (tfhe_hip.hip) ----------------------------------------------------------------------------------------
// Kept per (calling thread, handle); every context and pool carries an id that is never reused.
uint64_t new_handle_id();
void handle_gone(uint64_t id);
std::string &err_slot(uint64_t id);  // the slot a FAILING call writes its text into

// Calls on one handle are serialised IN ARRIVAL ORDER (a ticket lock).  std::mutex makes no such promise: a thread that
// issues calls back to back re-acquires it before a waiting thread wakes, and under `Send + Sync` use (a Rayon team
// calling Bootstrap::bootstrap on one strategy, src/bootstrap/mod.rs:23) one worker could starve the rest for as long
// as it had work -- seen in tests/cpp/test_mirror.cpp, where 400 failing calls took minutes beside a thread that kept
// bootstrapping.
class FairMutex {
 public:
  void lock() {
    std::unique_lock<std::mutex> lk(m_);
    const uint64_t ticket = next_++;
    cv_.wait(lk, [&] { return serving_ == ticket; });
  }
  void unlock() {
    {
      std::lock_guard<std::mutex> lk(m_);
      ++serving_;
    }
    cv_.notify_all();
  }

 private:
  std::mutex m_;
  std::condition_variable cv_;
  uint64_t next_ = 0, serving_ = 0;
};

// One resident cloud key in the engine layouts (src/key.rs:51-56).  A context owns one (`own`); every key view
// created with tfhe_hip_key_create owns another and runs on its parent's device, stream, scratch and mutex.
struct KeyState {
  DevArray<double2> d_bsk;
  DevArray<uint32_t> d_ksk;
  DevArray<unsigned char> d_ksk8;  // base-4 sets: the key as signed byte planes in MFMA fragment order (k_ksk_planes)
  DevArray<uint32_t> d_testvec;
  // the side keys, as byte planes: beside, not part of, the cloud key (a cloud-key load or change leaves them; freeing
  // the key view frees them)
  DevArray<unsigned char> d_pk8;    // the packing key (packing.hpp)
  bool pk_loaded = false;
  DevArray<unsigned char> d_pke8;   // the public key (pk_encrypt.hpp)
  int pke_size = 0;                 // encryptions of zero in the loaded public key
  bool pke_loaded = false;
  // the TRLWE switching keys (trlwe_switch.hpp), found by k: plain rows [t][2][N], the B operand of MmNegacyclic
  struct TrlweSwitchKey {
    int k = 0, basebit = 0, t = 0;
    DevArray<uint32_t> rows;
    bool loaded = false;
  };
  static constexpr int kMaxTrlweSwitchKeys = 16;
  TrlweSwitchKey tsk[kMaxTrlweSwitchKeys];
  uint32_t offset = 0;
  // The flags are written in key_change.hpp only: begin_key_change clears both, commit_cloud_key sets key_loaded (and
  // clears reenc_loaded), commit_reenc_key sets reenc_loaded; begin_side_key clears pk_loaded, pke_loaded or a
  // switching key's `loaded` and commit_side_key sets it.
  bool key_loaded = false;
  bool reenc_loaded = false;  // d_ksk (+ d_ksk8) hold a proxy re-encryption key (proxy_reenc.rs:224-233) instead of a cloud key's
};

// the context's own stream (a key view has none)
struct OwnStream {
  hipStream_t s = nullptr;
  OwnStream() = default;
  OwnStream(const OwnStream &) = delete;
  OwnStream &operator=(const OwnStream &) = delete;
  ~OwnStream() {
    if (s) (void)hipStreamDestroy(s);
  }
  operator hipStream_t() const { return s; }
};

struct Combiner;  // combine.hpp: the combining front end of the small host-pointer calls

// Every buffer, arena and event below frees itself when the context is deleted (resources.hpp), in reverse order of
// declaration: `stream` stands ahead of them all and so outlives them.  tfhe_hip_ctx_destroy drains the streams first.
struct tfhe_hip_ctx {
  tfhe_hip_params P{};
  int device = 0;
  OwnStream stream;
  KeyState own;
  KeyState *K = &own;            // the key of the call in progress (bound by ENTER under the mutex)
  tfhe_hip_ctx *parent = nullptr;  // non-null: this handle is a key view of `parent` (only P, own, parent are used)
  int views = 0;                 // live key views of this context
  bool dying = false;            // destroyed while views were alive: the last view to go frees the context
  DevArray<double2> d_tw;
  // scratch, sized through take() alone
  ScratchBuf lv1, u1, u2, ks_out, ks_dig;  // (ks_dig: key-switch digit bytes)
  ScratchBuf biv_s1, biv_tv;               // tree bootstrap (table.hpp): stage-1 results [m][chunk][n+1], their tables [chunk][2][N]
  ScratchBuf pke_sel;                      // public-key encryption (pk_encrypt.hpp): selector words and addends of one pass
  ScratchBuf ts_dig;                       // TRLWE key switch (trlwe_switch.hpp): digit planes [chunk][t][N] i8, then b' [chunk][N]
  ScratchBuf cm_dig;                       // packed CMUX (cmux.hpp): digit planes [chunk][2t][N] i8
  Scratch scratch;                         // the stream whose queued work may still use them (claim_scratch)
  DevBuf sym_sec;                      // the staged secrets of one call (secrets.hpp: SecretStage), wiped behind it
  // host-API staging: a / b / c / out also stage through their arenas on pool members (to_dev / to_host);
  // the arenas of tv / idx serve the combiner lanes only
  Staging a{{}, {}, true}, b{{}, {}, true}, c{{}, {}, true}, out{{}, {}, true}, tv, idx;
  Combiner *comb = nullptr;      // base contexts: concurrent small host-pointer calls are merged into shared launches (combine.hpp)
  bool is_lane = false;          // this context is a combiner lane of another one (never handed to a caller)
  bool stage_pinned = false;     // set by a pool with several members: stage pageable operands through the arenas
  FairMutex mu;  // one call at a time per context, first come first served
  uint64_t id = new_handle_id();  // key of this context's per-thread error text (err_slot)
  bool profiling = false;
  int num_cus = 0;
  // ---- dispatch (plan_blind_rotate / plan_key_switch of tfhe_hip.hip; tfhe_hip_describe_dispatch prints a plan) ----
  // One member, so that a combiner lane takes its base context's choices with one assignment (comb_make_lane): a
  // knob added here reaches the merged small calls too.
  struct Dispatch {
    // The two selectors are the supported controls (TFHE_HIP_BR_KERNEL / TFHE_HIP_KS_KERNEL, include/tfhe_hip.h):
    // AUTO picks per batch size, anything else runs that kernel at every batch size.
    int br_force = 0;  // BrKind + 1, 0 = auto
    int ks_force = 0;  // KsKind + 1, 0 = auto
    // crossovers of the automatic choice, in ciphertexts; set from the CU count at creation
    size_t wide_max = 256;      // blind rotate: one eight-wave workgroup per ciphertext up to this batch size
    size_t pair_lo = 0, pair_max = 0;  // ... two ciphertexts per workgroup (k_blind_rotate_pair) for pair_lo < count <= pair_max
    size_t ks_split_max = 256;  // key switch: coefficient walk split over 32 workgroups up to this batch size
    size_t ks_mfma_min = 64;    // smallest batch the matrix-core kernel takes (below: the split kernel)
    size_t ks_sl_chunk_min = 384;  // wider bases: smallest batch the column-sliced kernel takes (with K chunks; below: the split kernel)
    bool fast_round = false;  // |pre-rounding value| < 2^51 guaranteed (see round_to_torus<FAST>)
  } dispatch;
  EventPairs ev_br, ev_ks;              // one pair per launch while profiling is on
  EventPairs ev_pke_sel, ev_pke_mm;     // pk_encrypt.hpp: the keystream pass, the contraction
  EventPairs ev_ts_dig, ev_ts_mm;       // trlwe_switch.hpp: the digits pass, the contraction
  EventPairs ev_cm_dig, ev_cm_mm, ev_cm_add;  // cmux.hpp: the digits pass, the contraction, the addend
  uint64_t bootstraps = 0;
  // device diagnostics: [0] shader cycles, [1] constant-rate ticks (both summed over blind-rotate
  // workgroups while profiling is on), [2] error flag raised by kernels (bad gate code), [4] / [5] the same two
  // sums for the matrix-core key switch
  DevArray<unsigned long long> d_diag;
  int rtc_khz = 100000;  // rate of s_memrealtime (hipDeviceAttributeWallClockRate)
  ~tfhe_hip_ctx() { handle_gone(id); }  // (registration and erasure cannot drift apart: every `delete` passes here)
};

// The HIP current device is per host thread and shared with every other library in the process
// (torch included): set ours for the duration of a call and put the caller's back.
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) err = hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// Every entry point: a key view runs on its parent -- `ctx` is re-pointed at the parent, whose mutex serialises the
// call, whose device is made current (the caller's is put back on return) and whose key pointer K is bound to the
// view's key for the duration of the call (RAII; a plain context binds its own).
struct KeyBind {
  tfhe_hip_ctx *c;
  KeyBind(tfhe_hip_ctx *base, KeyState *k) : c(base) { c->K = k; }
  ~KeyBind() { c->K = &c->own; }
};
#define ENTER(ctx)                                                                     \
  tfhe_hip_ctx *self_ = (ctx);                                                         \
  if (self_->parent) (ctx) = self_->parent;                                            \
  std::lock_guard<FairMutex> lk_((ctx)->mu);                                           \
  KeyBind kb_((ctx), &self_->own);                                                     \
  DeviceGuard dg_((ctx)->device);                                                      \
  if (dg_.err != hipSuccess) {                                                         \
    err_slot((ctx)->id) = std::string("hipSetDevice: ") + hipGetErrorString(dg_.err);  \
    return TFHE_HIP_EHIP;                                                              \
  }

#define HIPCHK(ctx, call)                                                                   \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      err_slot((ctx)->id) = std::string(#call) + ": " + hipGetErrorString(e_);              \
      return TFHE_HIP_EHIP;                                                                 \
    }                                                                                       \
  } while (0)

#define CHK(expr)                 \
  do {                            \
    int rc_ = (expr);             \
    if (rc_ != TFHE_HIP_OK) return rc_; \
  } while (0)

// ---- errors, buffers, scratch (tfhe_hip.hip; fail, ensure and claim_scratch are declared by secrets.hpp) --------------
int hip_rc(tfhe_hip_ctx *ctx, const HipErr &r);  // a runtime call that resources.hpp made for this context
// A buffer of exactly `bytes` that is allocated once; `call` is how that allocation reads in the text of its failure.
int alloc_exact(tfhe_hip_ctx *ctx, DevBuf &b, size_t bytes, const char *call);
// The scratch buffers are sized here and nowhere else: the claim, then the growth.  `what` names the buffer in the text
// of a failed allocation.
int take(tfhe_hip_ctx *ctx, hipStream_t s, ScratchBuf &b, size_t bytes, bool exact = false, const char *what = "hipMalloc scratch: ");
int launched(tfhe_hip_ctx *ctx);  // status of the kernel launch just made
inline hipStream_t pick(tfhe_hip_ctx *ctx, void *stream) { return stream ? (hipStream_t)stream : ctx->stream; }
inline const uint32_t *u32(const void *p) { return (const uint32_t *)p; }

// ---- sizes ---------------------------------------------------------------------------------------------------------------
// the operands the entry points name: `count` TLWE rows [n+1], TRLWE [2][N], level-1 rows [N+1] in the whole 256-row
// groups the matrix-core key switch reads, and a test vector (one per ciphertext, or one for the call)
inline size_t lv1_rows(size_t count) { return (count + kKmRows - 1) / kKmRows * kKmRows; }
inline size_t tlwe_bytes(const tfhe_hip_ctx *ctx, size_t count) { return count * (size_t)(ctx->P.n + 1) * 4; }
inline size_t trlwe_bytes(size_t count) { return count * (size_t)2 * kN * 4; }
inline size_t lv1_bytes(size_t count) { return lv1_rows(count) * (size_t)(kN + 1) * 4; }
inline size_t testvec_bytes(int per_ct, size_t count) { return trlwe_bytes(per_ct ? count : 1); }
// the key buffers (engine layouts)
inline size_t bsk_polys(const tfhe_hip_params &P) { return (size_t)P.n * 2 * P.l * 2; }
inline size_t bsk_bytes(const tfhe_hip_params &P) { return bsk_polys(P) * kN * sizeof(double); }
inline size_t ksk_rows(const tfhe_hip_params &P) { return (size_t)kN * P.t * ((size_t)1 << P.basebit); }
inline size_t ksk_bytes(const tfhe_hip_params &P) { return ksk_rows(P) * ksk_row_words(P.n) * 4; }
inline size_t key_testvec_bytes() { return testvec_bytes(0, 1); }
bool params_supported(const tfhe_hip_params *p);  // tfhe_hip_ctx_create's bounds

// ---- kernel families -----------------------------------------------------------------------------------------------------
// The instantiation of a kernel family for this context: pick(KernelInst<l, fast_round, many>{}).  Every family of
// kernels templated on the decomposition level and the rounding is named once, in its `pick`.
template <int L_, bool FAST_, bool MANY_>
struct KernelInst {
  static constexpr int L = L_;
  static constexpr bool FAST = FAST_, MANY = MANY_;
};
template <int L, typename Pick>
auto kernel_inst_at(bool fast, bool many, Pick pick) {
  return fast ? (many ? pick(KernelInst<L, true, true>{}) : pick(KernelInst<L, true, false>{}))
              : (many ? pick(KernelInst<L, false, true>{}) : pick(KernelInst<L, false, false>{}));
}
template <typename Pick>
auto kernel_inst(const tfhe_hip_ctx *ctx, bool many, Pick pick) {
  const bool f = ctx->dispatch.fast_round;
  switch (ctx->P.l) {
    case 1: return kernel_inst_at<1>(f, many, pick);
    case 2: return kernel_inst_at<2>(f, many, pick);
    default: return kernel_inst_at<3>(f, many, pick);
  }
}

// ---- bootstrap and key switch (tfhe_hip.hip) -----------------------------------------------------------------------------
// TFHE_HIP_COPY: the plain bootstrap of the first operand, no second one
static_assert(kGateCount == TFHE_HIP_COPY + 1, "kGateTable (blind_rotate.hpp) has one row per tfhe_hip_gate");
constexpr GatePrep kCopyPrep = kGateTable[TFHE_HIP_COPY];

// One blind-rotation launch, described.  Everything defaults to "absent": a call site names what it sets.
struct BrCall {
  const uint32_t *in_a = nullptr, *in_b = nullptr;  // operand rows [count][n+1]; with idx_a / idx_b the base the indices select from
  GatePrep gp = kCopyPrep;                          // the rotated row is ca * a + cb * b, [n] += cconst
  const uint32_t *testvec = nullptr;                // nullptr: the key's own
  int per_ct = 0;                                   // one test vector per ciphertext (only with `testvec`)
  size_t count = 0;
  // exactly one output: the rotated TRLWE [count][2][N], its extraction as the key switch's source [count][N+1], or its
  // extraction as a TLWE of the input's shape [count][n+1] (bootstrap_without_key_switch)
  uint32_t *out_trlwe = nullptr, *out_lv1 = nullptr, *out_ext2 = nullptr;
  const uint8_t *gate_codes = nullptr;                  // per-ciphertext gates (gp: kCodesPrep)
  const uint32_t *idx_a = nullptr, *idx_b = nullptr;    // row indices into in_a / in_b (circuit levels)
  int lut_shift = 0;                                    // many-LUT: 2^lut_shift extractions per ciphertext
};
// A bootstrap on stream `s`: the blind rotation `call` describes (everything but its output), then, with `keyswitch`,
// the key switch of its count << lut_shift extracted rows into `out`; without, the rows are extracted straight into
// `out` (bootstrap_without_key_switch).  The one place that takes the context's lv1 scratch for a blind rotation.
int run_bootstrap(tfhe_hip_ctx *ctx, hipStream_t s, BrCall call, uint32_t *out, bool keyswitch);
int launch_key_switch(tfhe_hip_ctx *ctx, hipStream_t s, const uint32_t *lv1, uint32_t *out, size_t count);
int need_key(tfhe_hip_ctx *ctx);
int lut_shift_of(int n_luts);  // n_luts in {1, 2, 4, 8} -> log2, else -1

// ---- host staging (tfhe_hip.hip) ------------------------------------------------------------------------------------------
int to_dev(tfhe_hip_ctx *ctx, Staging &s, const void *src, size_t bytes);
int to_host(tfhe_hip_ctx *ctx, void *dst, Staging &s, size_t bytes);
// the device view of a pinned host range [p, p + bytes), or nullptr when `p` is ordinary pageable memory
void *pinned_view(const void *p, size_t bytes);

// The direct path, after a call's own checks.  One operand: `bytes` at `host`, staged through `slot`; a null `host`
// is an operand this call does not use, which reaches the launch as nullptr.
struct HostIn {
  const void *host;
  size_t bytes;
  Staging *slot;
};
// With `zero_copy` (gate, gates_mixed, bootstrap, mux) and every operand and the output pinned, the launch runs on
// them in place (see pinned_view) and the stream is synchronised.  Otherwise each operand is staged with to_dev in
// list order, the launch writes ctx->out, and the result returns through to_host.  launch(in, out) gets the device
// view of each operand in list order and of the output.
template <size_t N, class Launch>
int host_call(tfhe_hip_ctx *ctx, bool zero_copy, const HostIn (&in)[N], void *out, size_t out_bytes, Launch &&launch) {
  const void *d[N] = {};
  if (zero_copy) {  // all operands pinned: no staging
    bool pinned = true;
    for (size_t i = 0; i < N && pinned; ++i)
      if (in[i].host) pinned = (d[i] = pinned_view(in[i].host, in[i].bytes)) != nullptr;
    if (void *dout = pinned ? pinned_view(out, out_bytes) : nullptr) {
      CHK(launch(d, dout));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      return TFHE_HIP_OK;
    }
  }
  for (size_t i = 0; i < N; ++i) {
    d[i] = nullptr;
    if (!in[i].host) continue;
    CHK(to_dev(ctx, *in[i].slot, in[i].host, in[i].bytes));
    d[i] = in[i].slot->dev.p;
  }
  CHK(ensure(ctx, ctx->out.dev, out_bytes));
  CHK(launch(d, ctx->out.dev.p));
  return to_host(ctx, out, ctx->out, out_bytes);
}

// A host-form encryption of plain [count], staged through slot a.  The primary output (out, or the bodies alone)
// returns through host_call; with both asked for, the bodies ride in staging buffer b.  bulk(d_plain, d_bodies, d_out)
// queues the call on the context's stream.  The plaintexts do not stay behind in the library's buffers.
template <class Bulk>
int encrypt_host_call(tfhe_hip_ctx *ctx, const uint32_t *plain, size_t count, uint32_t *bodies, size_t body_bytes, uint32_t *out,
                      size_t out_bytes, Bulk &&bulk) {
  if (out && bodies) CHK(ensure(ctx, ctx->b.dev, body_bytes));
  int rc = host_call(ctx, false, {{plain, count * 4, &ctx->a}}, out ? out : bodies, out ? out_bytes : body_bytes,
                     [&](const void *const *d, void *o) {
                       uint32_t *d_out = out ? (uint32_t *)o : nullptr;
                       uint32_t *d_bodies = out ? (bodies ? (uint32_t *)ctx->b.dev.p : nullptr) : (uint32_t *)o;
                       return bulk(u32(d[0]), d_bodies, d_out);
                     });
  if (rc == TFHE_HIP_OK && out && bodies) rc = to_host(ctx, bodies, ctx->b, body_bytes);
  scrub(ctx->stream, {{&ctx->a, count * 4}});
  return rc;
}

// ---- key changes (key_change.hpp, in tfhe_hip.hip; ctx->mu held and ctx's device current) --------------------------------
enum KeyBufs { KEY_BUF_BSK = 1, KEY_BUF_KSK = 2, KEY_BUF_TESTVEC = 4, KEY_BUF_ALL = 7 };
int begin_key_change(tfhe_hip_ctx *ctx, int which);
int commit_cloud_key(tfhe_hip_ctx *ctx, uint32_t offset);
int commit_reenc_key(tfhe_hip_ctx *ctx);
int begin_side_key(tfhe_hip_ctx *ctx, bool &flag, DevBuf &planes, size_t bytes);
inline void commit_side_key(bool &flag) { flag = true; }
int flag_is_loaded(tfhe_hip_ctx *ctx, bool KeyState::*flag);
// what a generated key gets: the decomposition offset (key.rs:78-89) and the test vector (key.rs:91-100), uploaded
int default_offset_and_testvec(tfhe_hip_ctx *ctx, uint32_t *offset);

// A device temporary of the sources' bytes plus `extra_bytes`; the sources copied into it back to back on ctx->stream;
// launch(temporary) -> hipError_t queues the conversion; the stream drained and the temporary freed on every path.
struct HostSrc {
  const void *p;
  size_t bytes;
};
template <class Launch>
int upload_through_temp(tfhe_hip_ctx *ctx, const char *label, std::initializer_list<HostSrc> srcs, size_t extra_bytes,
                        Launch &&launch) {
  size_t total = extra_bytes;
  for (const HostSrc &s : srcs) total += s.bytes;
  DevArray<char> d_tmp;
  CHK(alloc_exact(ctx, d_tmp, total, "hipMalloc((void **)&d_tmp, total)"));
  hipError_t e = hipSuccess;
  size_t at = 0;
  for (const HostSrc &s : srcs) {
    if (e == hipSuccess) e = hipMemcpyAsync(d_tmp + at, s.p, s.bytes, hipMemcpyHostToDevice, ctx->stream);
    at += s.bytes;
  }
  if (e == hipSuccess) e = launch(d_tmp.p);
  const hipError_t es = hipStreamSynchronize(ctx->stream);  // (nothing reads the temporary once this has returned)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(ctx, TFHE_HIP_EHIP, std::string(label) + " upload: " + hipGetErrorString(e));
  return TFHE_HIP_OK;
}

// The conversions between the reference layout and the engine layout of the key-switching key in ctx->K->d_ksk, queued
// on ctx->stream (k_ksk_convert / k_ksk_export): `rows` rows of n + 1 words at d_ref.
hipError_t ksk_convert_launch(tfhe_hip_ctx *ctx, const uint32_t *d_ref, size_t rows);
hipError_t ksk_export_launch(tfhe_hip_ctx *ctx, uint32_t *d_ref, size_t rows);

// ---- generator keys and staged secrets (key_change.hpp) -----------------------------------------------------------------
inline ChaChaKey seed_key(const uint8_t seed[32]) {
  ChaChaKey k;
  memcpy(k.k, seed, 32);  // 8 little-endian words, as tfhe_hip_gen_cloud_key_with_key reads its generator key
  return k;
}

// The 256-bit generator key K of one call: the caller's rng_key, or (NULL) 32 bytes of getrandom(2).  Wiped when the call
// leaves, whichever way.
struct GeneratorKey {
  ChaChaKey k{};
  GeneratorKey() = default;
  GeneratorKey(const GeneratorKey &) = delete;
  GeneratorKey &operator=(const GeneratorKey &) = delete;
  int fill(tfhe_hip_ctx *ctx, const uint8_t *rng_key);
  ~GeneratorKey() { wipe_host(k.k, sizeof(k.k)); }
};

// The secret keys, the spectrum of the ring key and the generator key do not outlive the call on the device,
// whichever way it ends: they travel through one SecretStage (secrets.hpp) on the context's stream, which zeroes the
// buffer and drains the stream on every exit path.  The generator key travels in the buffer too (not in
// kernel-argument memory).  The layout: K, the slot derive_public_seed writes, key_lv0 [n], key_lv1 [N], and the
// spectrum of key_lv1, which k_key_spectrum writes (16-byte aligned: it is read as double2).  The TRLWE switching key
// (trlwe_switch.hpp) stages a ring key where key_lv0 stands: k0_words = N, d_k0 the key switched from, d_k1 the key
// switched to.  TRGSW encryption (cmux.hpp) stages no first key at all: k0_words = 0.
struct StagedSecrets {
  size_t k0_words;  // words of the first key: n, or N for a ring key
  SecretStage stage;
  const uint32_t *d_k0 = nullptr, *d_k1 = nullptr;
  const double2 *d_spec = nullptr;
  ChaChaKey *d_rk = nullptr;  // the derived-seed slot is d_rk + 1
  explicit StagedSecrets(tfhe_hip_ctx *ctx) : StagedSecrets(ctx, (size_t)ctx->P.n) {}
  StagedSecrets(tfhe_hip_ctx *ctx, size_t k0_words)
      : k0_words(k0_words), stage(ctx, ctx->sym_sec, ctx->stream, 2 * sizeof(ChaChaKey) + (k0_words + kN) * 4, true) {}
};
static_assert(2 * sizeof(ChaChaKey) + ((size_t)kLweMaxN + kN) * 4 <= kSecretImageMax, "the largest image a call stages");
// Use: `StagedSecrets s(ctx); CHK(stage_secrets(ctx, ..., s));`
int stage_secrets(tfhe_hip_ctx *ctx, const uint32_t *key_lv0, const uint32_t *key_lv1, const ChaChaKey &rk, StagedSecrets &s);
// the spectrum of the ring key at d_key_lv1 into d_spec [N / 2], on stream s (k_key_spectrum)
int key_spectrum_launch(tfhe_hip_ctx *ctx, const uint32_t *d_key_lv1, double2 *d_spec, hipStream_t s);
// The public mask seed S of stream STREAM of the staged generator key (k_derive_stream_seed), derived into the slot
// behind it and copied back.  Instantiated in key_change.hpp for the library's seed streams.
template <uint32_t STREAM>
int derive_public_seed(tfhe_hip_ctx *ctx, const StagedSecrets &s, ChaChaKey &seed);
// The one launch of k_lwe_rows (keygen.hpp), on stream s: the encrypting variant, or with no generator key (j.k NULL)
// the expansion of given bodies.  j.rows >= 1.
int lwe_rows_launch(tfhe_hip_ctx *ctx, const LweRowJob &j, hipStream_t s);
// The key-switching key's rows (key.rs:102-122) over the staged secrets: plain (masks under K, streams 0 / 1) into the
// engine layout at `out`, or compressed (seed != NULL: masks under S, streams 16 / 17) as bodies only.
int ksk_rows_launch(tfhe_hip_ctx *ctx, const StagedSecrets &s, const ChaChaKey *seed, double alpha, uint32_t *bodies,
                    uint32_t *out);

// ---- between the feature units ---------------------------------------------------------------------------------------------
// planes.hip (matmul.hpp): the plaintext polynomial product on packed ciphertexts, on stream s; cols <= kPolymulMaxCols
constexpr size_t kPolymulMaxCols = 64;
int polymul_dev(tfhe_hip_ctx *ctx, const int8_t *w, const uint32_t *bias, size_t rows, size_t cols, const uint32_t *trlwe,
                size_t groups, uint32_t *out, hipStream_t s);
// planes.hip (table.hpp): why a tree bootstrap is TFHE_HIP_EINVAL, or nullptr (the pool form files it under the pool)
const char *bivariate_refusal(const uint32_t *x, const uint32_t *y, const uint32_t *testvecs, int m, int n_luts,
                              const uint32_t *out, size_t count);

#if TFHE_ABL_CATALOG
// The catalogue build alone (experiment.hpp): every unit's device code reads the selected defect from a word of its
// own, and tfhe_hip_ctx_create writes all three once, on the context's device, through the unit's own function.
hipError_t mutant_publish_core(unsigned id);    // tfhe_hip.hip
hipError_t mutant_publish_planes(unsigned id);  // planes.hip
hipError_t mutant_publish_rings(unsigned id);   // rings.hip
#define TFHE_MUTANT_PUBLISH(unit) \
  hipError_t mutant_publish_##unit(unsigned id) { return hipMemcpyToSymbol(HIP_SYMBOL(g_tfhe_mutant), &id, sizeof(id)); }
#endif

#pragma GCC visibility pop
