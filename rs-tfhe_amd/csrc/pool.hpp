// pool.hpp -- several GPUs behind ONE handle of the C ABI (included by tfhe_hip.hip; needs tfhe_hip_ctx).
//
// The reference's batch entry points are `par_iter().map().collect()` over the ciphertexts of a slice
// (src/parallel/rayon_impl.rs:40-47, called from src/gates.rs:357-383): order-preserving, embarrassingly
// parallel, one shared read-only &CloudKey.  The pool is that map over devices: one context per device, the
// cloud key generated / uploaded ONCE and replicated device-to-device in the engine layouts (no second
// conversion, no host round trip), a contiguous order-preserving split of the batch, one host thread per
// shard (each thread makes its shard's device current; the HIP current device is per thread), results
// written in place into the caller's output slice.  No collective and no exchange on the data path.
#pragma once
#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the library is opened at run time (rccl_api)

#include <chrono>
#include <system_error>
#include <thread>

struct RcclApi;
namespace {
struct PoolTimed {  // one bracket of a transfer (see tfhe_hip_pool's transfer timing)
  OwnEvent a, b;
  int member = 0;       // whose device the events live on
  long home_ix = -1;    // RCCL: the call's home-stream pair
  bool gather = false;  // (ev_home) which direction's group this pair brackets
};
}  // namespace
struct tfhe_hip_pool {
  std::vector<tfhe_hip_ctx *> ctxs;
  tfhe_hip_pool *parent = nullptr;  // non-null: a key view of `parent` (same devices, streams, staging, communicator and mutex)
  int views = 0;                    // live key views (root only)
  bool dying = false;               // destroyed while views were alive: the last view to go frees the pool
  FairMutex own_mu;  // one call at a time per ROOT pool, first come first served: a view's calls serialise with its parent's (they share streams and staging)
  uint64_t id = new_handle_id();  // key of the per-thread error text (err_slot)
  bool replicated_by_rccl = false;  // how the last key reached the members (tfhe_hip_pool_key_transport)
  // ---- root only: what the device-resident (_dev) calls and the key replication share ----
  std::vector<ncclComm_t> comms;    // ONE persistent communicator per pool (created on first use, destroyed with the pool)
  int comm_state = 0;               // 0 = not tried yet, 1 = ready, -1 = unavailable (duplicate devices, no librccl, init failed)
  bool comms_dropped = false;       // a group failed half-way (pool_drop_comms): streams it touched may never drain
  struct Stage {                    // per member: staging for shards that arrive from / leave for another member's GPU
    DevBuf in[5], out;
    OwnEvent done;                  // recorded on the member's stream when its shard's result has left
    // (spelled out only to stay out of the library's dynamic symbols, as the owners in the unnamed namespaces do)
    Stage() = default;
    __attribute__((visibility("hidden"))) Stage(Stage &&) = default;
    __attribute__((visibility("hidden"))) Stage &operator=(Stage &&) = default;
    __attribute__((visibility("hidden"))) ~Stage() = default;
  };
  std::vector<Stage> stage;
  OwnEvent ready;                     // recorded on the home stream when the call's operands are ready (peer-copy path)
  int ready_device = -1;
  const char *last_transport = "none";  // transport of the last _dev call: "rccl" / "peer-copy" / "none" (nothing moved)
  // transfer timing (tfhe_hip_pool_get_transfer_times): per moved shard one event pair on the MEMBER's stream (the
  // receiver of a scatter, the sender of a gather); on the RCCL path also one pair per call and direction on the HOME
  // stream around the group (`home_ix` into ev_home).  A transfer can only start when BOTH ends have reached it, so
  // the pair of the side that arrived last brackets the transfer alone and the other one also brackets its wait for
  // the peer (e.g. the home stream's receive group waits for the slowest member's compute): a shard's transfer time
  // is the SHORTER of its two brackets.
  using Timed = PoolTimed;
  bool timing = false;
  std::vector<Timed> ev_scatter, ev_gather, ev_home;
  uint64_t scatter_bytes = 0, gather_bytes = 0, dev_calls = 0;
  // set-up costs, host wall clock (not reset by reading): creating the persistent communicator (ncclCommInitAll, once
  // per pool) and the last replication of a cloud key to the members (ncclBroadcast or peer copies + the members'
  // byte-plane builds), so that neither hides inside a "key generation" figure
  double comm_create_ms = 0.0, key_replication_ms = 0.0;

  ~tfhe_hip_pool() { handle_gone(id); }
  tfhe_hip_pool *root() { return parent ? parent : this; }
  const tfhe_hip_pool *root() const { return parent ? parent : this; }
};

namespace {

// [lo, hi) of shard r of `world` over `count` items: contiguous, order-preserving, sizes differ by at most 1
inline void pool_shard(size_t count, int r, int world, size_t &lo, size_t &hi) {
  const size_t base = count / (size_t)world, rem = count % (size_t)world;
  lo = (size_t)r * base + ((size_t)r < rem ? (size_t)r : rem);
  hi = lo + base + ((size_t)r < rem ? 1 : 0);
}

int pool_fail(tfhe_hip_pool *p, int code, const std::string &msg) {
  err_slot(p->id) = msg;
  return code;
}

// What a member's failed call becomes on the pool: "device N: <the member's text>".  A member's text is per thread
// (err_slot): this is for the thread that made the call.
std::string pool_member_text(tfhe_hip_ctx *c) { return "device " + std::to_string(c->device) + ": " + tfhe_hip_last_error(c); }
// `rc` of a call just made on member `c` by this thread, recorded on the pool when it is a failure
int pool_member_rc(tfhe_hip_pool *p, tfhe_hip_ctx *c, int rc) {
  return rc == TFHE_HIP_OK ? rc : pool_fail(p, rc, pool_member_text(c));
}

// dst takes src's key (engine layouts), device to device.  Either may be a key view; both idle on entry.
int clone_key(tfhe_hip_ctx *dst, tfhe_hip_ctx *src) {
  const KeyState *from = &src->own;  // the key src OWNS (K is only bound during a call)
  const int src_device = src->device;
  tfhe_hip_ctx *ctx = dst;
  ENTER(ctx);
  CHK(begin_key_change(ctx, KEY_BUF_ALL));
  HIPCHK(ctx, hipMemcpyPeer(ctx->K->d_bsk, ctx->device, from->d_bsk, src_device, bsk_bytes(ctx->P)));
  HIPCHK(ctx, hipMemcpyPeer(ctx->K->d_ksk, ctx->device, from->d_ksk, src_device, ksk_bytes(ctx->P)));
  HIPCHK(ctx, hipMemcpyPeer(ctx->K->d_testvec, ctx->device, from->d_testvec, src_device, key_testvec_bytes()));
  HIPCHK(ctx, hipDeviceSynchronize());
  return commit_cloud_key(ctx, from->offset);
}

// ---- RCCL over xGMI: one persistent communicator per pool -------------------------------------------------------
// north_star: "RCCL over xGMI used only for the trivial scatter/gather".  The exchanges this path has are the
// replication of the cloud key (172 MB, once per key: one grouped ncclBroadcast per key buffer, in place in the
// engine layouts) and, for a batch that is resident on ONE member's GPU (the *_dev pool calls below), the scatter of
// its shards and the gather of their results (grouped ncclSend / ncclRecv, one pair per peer, so all xGMI links run
// concurrently).  librccl is opened at run time (no link-time dependency: a process that already carries torch's
// RCCL reuses it by SONAME).  The communicator is created on first use and lives as long as the pool.  Anything that
// fails -- library absent, duplicate devices (ncclCommInitAll refuses them), a transport error -- falls back to
// hipMemcpyPeer[Async].
struct RcclApi {
  void *lib = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;  // optional
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  bool ok = false;
};
inline RcclApi &rccl_api() {
  static RcclApi a = [] {
    RcclApi r;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      r.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (r.lib) break;
    }
    if (!r.lib) return r;
    r.CommInitAll = (decltype(r.CommInitAll))dlsym(r.lib, "ncclCommInitAll");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
    r.CommAbort = (decltype(r.CommAbort))dlsym(r.lib, "ncclCommAbort");
    r.GroupStart = (decltype(r.GroupStart))dlsym(r.lib, "ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))dlsym(r.lib, "ncclGroupEnd");
    r.Broadcast = (decltype(r.Broadcast))dlsym(r.lib, "ncclBroadcast");
    r.Send = (decltype(r.Send))dlsym(r.lib, "ncclSend");
    r.Recv = (decltype(r.Recv))dlsym(r.lib, "ncclRecv");
    r.ok = r.CommInitAll && r.CommDestroy && r.GroupStart && r.GroupEnd && r.Broadcast && r.Send && r.Recv;
    return r;
  }();
  return a;
}

inline int pool_rccl_mode() {  // 0 = never, 1 = pools of >= 2 distinct devices, 2 = also a pool of one (plumbing test)
  const char *env = getenv("TFHE_HIP_POOL_RCCL");
  return env ? atoi(env) : 1;
}

// The pool's communicator (root pool's mutex held): created once, reused by every key replication and every
// device-resident batch call, destroyed by tfhe_hip_pool_destroy.  nullptr: take the peer-copy path.
std::vector<ncclComm_t> *pool_comms(tfhe_hip_pool *p) {
  tfhe_hip_pool *root = p->root();
  if (root->comm_state == 1) return &root->comms;
  if (root->comm_state < 0) return nullptr;
  root->comm_state = -1;
  const int n = (int)root->ctxs.size();
  const int mode = pool_rccl_mode();
  if (mode == 0 || n < (mode >= 2 ? 1 : 2)) return nullptr;
  RcclApi &R = rccl_api();
  if (!R.ok) return nullptr;
  std::vector<int> devs;
  for (auto *c : root->ctxs) devs.push_back(c->device);
  for (int i = 0; i < n; ++i)  // one rank per GPU: a pool that repeats a device takes the peer-copy path
    for (int j = i + 1; j < n; ++j)
      if (devs[(size_t)i] == devs[(size_t)j]) return nullptr;
  int prev = -1;
  (void)hipGetDevice(&prev);
  std::vector<ncclComm_t> comms((size_t)n, nullptr);
  const auto t0 = std::chrono::steady_clock::now();
  const bool good = R.CommInitAll(comms.data(), n, devs.data()) == ncclSuccess;
  root->comm_create_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (prev >= 0) (void)hipSetDevice(prev);
  if (!good) {
    (void)hipGetLastError();
    return nullptr;
  }
  root->comms = std::move(comms);
  root->comm_state = 1;
  return &root->comms;
}

// A call failed INSIDE an open RCCL group (or its GroupEnd did): sends / receives of the group may have been launched
// without their partners, so the communicator's state is undefined and the streams it was used on may never drain.
// The pool stops using it: the communicators are aborted (ncclCommAbort where the library has it, which also releases
// kernels that wait for a partner) and every later call takes the peer-copy path.
void pool_drop_comms(tfhe_hip_pool *p) {
  tfhe_hip_pool *root = p->root();
  if (root->comm_state != 1) return;
  RcclApi &R = rccl_api();
  // (no ncclCommAbort in this librccl: the communicators are LEAKED -- ncclCommDestroy waits for outstanding work, and a
  // send whose receive was never launched would hang the caller here, with the pool's mutex held)
  for (ncclComm_t c : root->comms)
    if (c && R.CommAbort) (void)R.CommAbort(c);
  root->comms.clear();
  root->comm_state = -1;
  root->comms_dropped = true;
  (void)hipGetLastError();
}

// member i >= 1: drained, its key buffers allocated, no valid key until finish_replica
int prepare_replica(tfhe_hip_ctx *member) {
  tfhe_hip_ctx *ctx = member;
  ENTER(ctx);
  return begin_key_change(ctx, KEY_BUF_ALL);
}
int finish_replica(tfhe_hip_ctx *member, uint32_t offset) {
  tfhe_hip_ctx *ctx = member;
  ENTER(ctx);
  HIPCHK(ctx, hipDeviceSynchronize());
  return commit_cloud_key(ctx, offset);
}

// true: every member holds member 0's key.  false: nothing usable happened (members >= 1 may hold garbage and are
// marked unloaded): the caller takes the peer-copy path.  The root pool's mutex is held by the caller, which keeps
// every other pool call (the parent's and its views': they share that mutex) off the members' streams meanwhile.
bool replicate_key_rccl(tfhe_hip_pool *p) {
  const int n = (int)p->ctxs.size();
  std::vector<ncclComm_t> *comms = pool_comms(p);
  if (!comms) return false;
  RcclApi &R = rccl_api();
  for (int i = 1; i < n; ++i)
    if (prepare_replica(p->ctxs[(size_t)i]) != TFHE_HIP_OK) return false;
  int prev = -1;
  (void)hipGetDevice(&prev);
  const tfhe_hip_params &P = p->ctxs[0]->P;
  const size_t bytes[3] = {bsk_bytes(P), ksk_bytes(P), key_testvec_bytes()};
  // the members' own mutexes: a member borrowed with tfhe_hip_pool_ctx() and used from another thread waits
  std::vector<std::unique_lock<FairMutex>> held;
  for (int i = 0; i < n; ++i) {
    tfhe_hip_ctx *c = p->ctxs[(size_t)i];
    held.emplace_back((c->parent ? c->parent : c)->mu);
  }
  bool good = true;
  for (int b = 0; b < 3 && good; ++b) {
    good = R.GroupStart() == ncclSuccess;
    for (int i = 0; i < n && good; ++i) {
      tfhe_hip_ctx *c = p->ctxs[(size_t)i];
      tfhe_hip_ctx *base = c->parent ? c->parent : c;
      KeyState &k = c->own;
      void *buf = b == 0 ? (void *)k.d_bsk : b == 1 ? (void *)k.d_ksk : (void *)k.d_testvec;
      good = hipSetDevice(c->device) == hipSuccess &&
             R.Broadcast(buf, buf, bytes[b], ncclUint8, 0, (*comms)[(size_t)i], base->stream) == ncclSuccess;
    }
    good = (R.GroupEnd() == ncclSuccess) && good;
  }
  for (int i = 0; i < n; ++i) {
    tfhe_hip_ctx *c = p->ctxs[(size_t)i];
    tfhe_hip_ctx *base = c->parent ? c->parent : c;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(base->stream) != hipSuccess) good = false;
  }
  held.clear();
  if (prev >= 0) (void)hipSetDevice(prev);
  if (!good) {
    pool_drop_comms(p);  // a broadcast group that failed half-way: the communicator is not used again
    (void)hipGetLastError();
    return false;
  }
  for (int i = 1; i < n; ++i)
    if (finish_replica(p->ctxs[(size_t)i], p->ctxs[0]->own.offset) != TFHE_HIP_OK) return false;
  p->replicated_by_rccl = true;
  return true;
}

int replicate_key(tfhe_hip_pool *p) {
  p->replicated_by_rccl = false;
  tfhe_hip_pool *root = p->root();
  const bool had_comm = root->comm_state == 1;
  auto t0 = std::chrono::steady_clock::now();
  struct Stamp {  // (the communicator's creation, when this call caused it, is reported on its own)
    tfhe_hip_pool *root;
    std::chrono::steady_clock::time_point t0;
    bool had_comm;
    ~Stamp() {
      double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (!had_comm && root->comm_state == 1) ms -= root->comm_create_ms;
      root->key_replication_ms = ms > 0 ? ms : 0.0;
    }
  } stamp{root, t0, had_comm};
  if (replicate_key_rccl(p)) return TFHE_HIP_OK;
  for (size_t i = 1; i < p->ctxs.size(); ++i) {
    CHK(pool_member_rc(p, p->ctxs[i], clone_key(p->ctxs[i], p->ctxs[0])));
  }
  return TFHE_HIP_OK;
}

// Members a batch of `count` is spread over: one device runs up to 256 ciphertexts in the time of one (the
// latency kernels give every ciphertext its own workgroup), so smaller batches are not cut thinner than that.
inline int pool_world_for(const tfhe_hip_pool *p, size_t count) {
  const size_t want = (count + 255) / 256;
  const size_t have = p->ctxs.size();
  return (int)(want < 1 ? 1 : (want < have ? want : have));
}

// run(ctx, lo, hi) on every non-empty shard, shard 0 on the calling thread; first failure wins.  A shard's error text
// is read on the thread that ran it (the text is per thread, err_slot).  world_req > 0: that many members (at most the
// pool's) instead of pool_world_for's count, for calls whose items are not single ciphertexts.
template <class F>
int pool_map(tfhe_hip_pool *p, size_t count, F &&run, int world_req = 0) {
  const int world = world_req > 0 ? std::min(world_req, (int)p->ctxs.size()) : pool_world_for(p, count);
  std::vector<int> rc((size_t)world, TFHE_HIP_OK);
  std::vector<std::string> text((size_t)world);
  auto shard = [&](int r, size_t lo, size_t hi) {
    tfhe_hip_ctx *c = p->ctxs[(size_t)r];
    rc[(size_t)r] = run(c, lo, hi);
    if (rc[(size_t)r] != TFHE_HIP_OK) text[(size_t)r] = pool_member_text(c);
  };
  std::vector<std::thread> th;
  for (int r = 1; r < world; ++r) {
    size_t lo, hi;
    pool_shard(count, r, world, lo, hi);
    if (hi <= lo) continue;
    try {
      th.emplace_back([&, r, lo, hi] { shard(r, lo, hi); });
    } catch (const std::system_error &) {  // no thread to be had: this shard runs on the calling thread
      shard(r, lo, hi);
    }
  }
  {
    size_t lo, hi;
    pool_shard(count, 0, world, lo, hi);
    if (hi > lo) shard(0, lo, hi);
  }
  for (auto &t : th) t.join();
  for (int r = 0; r < world; ++r)
    if (rc[(size_t)r] != TFHE_HIP_OK) return pool_fail(p, rc[(size_t)r], text[(size_t)r]);
  return TFHE_HIP_OK;
}

// ---- a batch that is RESIDENT on one member's GPU (the *_dev pool calls) ---------------------------------------
// "scatter inputs / gather outputs as grouped ncclSend / ncclRecv when the batch is resident on one
// GPU".  The caller's operands and result are device pointers on member `home`'s GPU and the call is only
// ENQUEUED (like the single-context *_dev calls): on `stream` (home) and on the other members' own streams, tied
// together by events / by the RCCL kernels themselves.  Shard r of the order-preserving split runs on member
// (home + r) mod size, so shard 0 -- and a batch too small to be cut -- never leaves home.  Per call:
//   home stream   [ sends of shards 1.. ]  [ shard 0 computed in place ]  [ receives of results 1.. ]
//   peer stream   [ receive shard ]        [ compute from / into staging ] [ send result ]
// One grouped ncclSend/ncclRecv per (peer, operand): every xGMI link carries its own peer's shard concurrently
// (65,536 NAND over 8 GPUs: 2 x 23 MB in, 23 MB out per peer = 0.45 ms at 153 GB/s, against 42 ms of compute).
// Without a communicator (a repeated device, no librccl, TFHE_HIP_POOL_RCCL=0): hipMemcpyPeerAsync on the peer's
// stream behind an event of the home stream, and an event per peer ahead of whatever follows on the home stream.
struct PoolIn {
  const void *ptr = nullptr;  // on home's GPU (host-pointer forms: the caller's); nullptr = operand absent
  size_t row_bytes = 0;       // per ciphertext when sharded, the whole operand otherwise
  bool sharded = true;        // false: every member needs all of it (a shared test vector)
  bool required = false;      // absent is "null pointer" (unless the batch is empty)
};

// op(ctx, ins[5], out, m, stream): enqueue the batched operation for m ciphertexts on member `ctx` (world_req: as for
// pool_map)
template <class Op>
int pool_dev_map(tfhe_hip_pool *p, int home, size_t count, void *stream_v, const PoolIn (&ins)[5], void *out,
                 size_t out_row_bytes, Op &&op, int world_req = 0) {
  tfhe_hip_pool *root = p->root();
  const int size = (int)p->ctxs.size();
  if (home < 0 || home >= size) return pool_fail(p, TFHE_HIP_EINVAL, "no such pool member (home)");
  root->last_transport = "none";
  if (count == 0) return TFHE_HIP_OK;
  tfhe_hip_ctx *hctx = p->ctxs[(size_t)home];
  tfhe_hip_ctx *hbase = hctx->parent ? hctx->parent : hctx;
  hipStream_t hs = stream_v ? (hipStream_t)stream_v : hbase->stream;
  // `hs` goes to the member's *_dev entry point as it is (there NULL means "the context's own stream", so the default
  // stream is named by hipStreamLegacy); the event, wait and RCCL calls below take the runtime's own name for the
  // default stream, NULL (hipStreamWaitEvent on the hipStreamLegacy handle faults in this HIP runtime)
  hipStream_t hrt = hs == hipStreamLegacy ? (hipStream_t) nullptr : hs;
  const int world = world_req > 0 ? std::min(world_req, size) : pool_world_for(p, count);
  std::vector<ncclComm_t> *comms = world > 1 || pool_rccl_mode() >= 2 ? pool_comms(p) : nullptr;
  // TFHE_HIP_POOL_RCCL=2 on a pool of ONE member (plumbing test on a one-GPU box): home's own shard takes the remote
  // path through a self send / receive, so the same symbols, group structure and stream handling run as among peers
  const bool loopback = comms && size == 1 && pool_rccl_mode() >= 2;
  const bool any_remote = world > 1 || loopback;
  RcclApi &R = rccl_api();
  if (root->stage.size() < (size_t)size) root->stage.resize((size_t)size);
  int prev = -1;
  (void)hipGetDevice(&prev);
  struct Restore {
    int d;
    ~Restore() {
      if (d >= 0) (void)hipSetDevice(d);
    }
  } restore{prev};
  auto hipfail = [&](const char *what, hipError_t e, int member) {
    return pool_fail(p, TFHE_HIP_EHIP, "device " + std::to_string(p->ctxs[(size_t)member]->device) + ": " + what + ": " + hipGetErrorString(e));
  };
  auto ensure_on = [&](int member, DevBuf &b, size_t bytes) -> int {
    if (bytes <= b.cap) return TFHE_HIP_OK;
    const hipError_t e = hipSetDevice(p->ctxs[(size_t)member]->device);
    if (e != hipSuccess) return hipfail("hipSetDevice", e, member);
    if (b.grow(bytes) != hipSuccess) {
      (void)hipGetLastError();
      return pool_fail(p, TFHE_HIP_ENOMEM, "device " + std::to_string(p->ctxs[(size_t)member]->device) + ": hipMalloc pool staging");
    }
    return TFHE_HIP_OK;
  };
  // transfer timing: begin records the first event of a new pair on `s` and returns the pair's index (-1: off), end
  // records the second event of pair `idx`
  using TimedVec = std::vector<tfhe_hip_pool::Timed>;
  auto timed_begin = [&](TimedVec &v, int member, hipStream_t s, long home_ix = -1) -> long {
    if (!root->timing || v.size() >= 4096) return -1;  // (a caller that never collects: stop at 4,096 pending pairs)
    (void)hipSetDevice(p->ctxs[(size_t)member]->device);
    tfhe_hip_pool::Timed t;
    if (t.a.create() != hipSuccess || t.b.create() != hipSuccess) return -1;
    (void)hipEventRecord(t.a, s);
    t.member = member;
    t.home_ix = home_ix;
    v.push_back(std::move(t));
    return (long)v.size() - 1;
  };
  auto timed_end = [&](TimedVec &v, long idx, hipStream_t s) {
    if (idx < 0) return;
    (void)hipSetDevice(p->ctxs[(size_t)v[(size_t)idx].member]->device);
    (void)hipEventRecord(v[(size_t)idx].b, s);
  };
  // shard table: shard r -> member, [lo, hi), remote?
  struct Sh {
    int member;
    size_t lo, hi;
    bool remote;
  };
  std::vector<Sh> shards;
  for (int r = 0; r < world; ++r) {
    size_t lo, hi;
    pool_shard(count, r, world, lo, hi);
    if (hi <= lo) continue;
    const int member = (home + r) % size;
    shards.push_back({member, lo, hi, member != home || loopback});
  }
  // 1. staging on the receiving members
  for (const Sh &sh : shards) {
    if (!sh.remote) continue;
    tfhe_hip_pool::Stage &st = root->stage[(size_t)sh.member];
    for (int k = 0; k < 5; ++k)
      if (ins[k].ptr) CHK(ensure_on(sh.member, st.in[k], ins[k].sharded ? (sh.hi - sh.lo) * ins[k].row_bytes : ins[k].row_bytes));
    CHK(ensure_on(sh.member, st.out, (sh.hi - sh.lo) * out_row_bytes));
    if (!st.done) {
      (void)hipSetDevice(p->ctxs[(size_t)sh.member]->device);
      const hipError_t e = st.done.create(hipEventDisableTiming);
      if (e != hipSuccess) return hipfail("hipEventCreate", e, sh.member);
    }
  }
  auto member_stream = [&](int member) -> hipStream_t {
    tfhe_hip_ctx *c = p->ctxs[(size_t)member];
    return (c->parent ? c->parent : c)->stream;
  };
  // 2. scatter
  if (any_remote) {
    root->last_transport = comms ? "rccl" : "peer-copy";
    if (comms) {
      // everything that can fail for a reason of ours is checked BEFORE the group opens (every device can be made
      // current, every staging buffer exists): inside it only the RCCL calls themselves can fail, and if one does the
      // communicator is dropped (pool_drop_comms) -- a send that was launched without its receive may never complete,
      // so after such an error the home stream may be poisoned and the caller should not wait on it
      for (const Sh &sh : shards) {
        if (!sh.remote) continue;
        const hipError_t e = hipSetDevice(p->ctxs[(size_t)sh.member]->device);
        if (e != hipSuccess) return hipfail("hipSetDevice", e, sh.member);
        for (int k = 0; k < 5; ++k)
          if (ins[k].ptr && !root->stage[(size_t)sh.member].in[k].p) return pool_fail(p, TFHE_HIP_EHIP, "pool staging buffer missing");
      }
      {
        const hipError_t e = hipSetDevice(hctx->device);
        if (e != hipSuccess) return hipfail("hipSetDevice", e, home);
      }
      // (events go in before the group opens: inside it nothing is enqueued yet)
      const long hix = timed_begin(root->ev_home, home, hrt);
      std::vector<long> tix(shards.size(), -1);
      for (size_t q = 0; q < shards.size(); ++q)
        if (shards[q].remote) tix[q] = timed_begin(root->ev_scatter, shards[q].member, member_stream(shards[q].member), hix);
      if (R.GroupStart() != ncclSuccess) return pool_fail(p, TFHE_HIP_EHIP, "ncclGroupStart (scatter)");
      bool good = true;  // (a group that was opened is always closed, whatever fails inside it)
      for (const Sh &sh : shards) {
        if (!sh.remote) continue;
        tfhe_hip_pool::Stage &st = root->stage[(size_t)sh.member];
        for (int k = 0; k < 5 && good; ++k) {
          if (!ins[k].ptr) continue;
          const size_t bytes = ins[k].sharded ? (sh.hi - sh.lo) * ins[k].row_bytes : ins[k].row_bytes;
          const unsigned char *src = (const unsigned char *)ins[k].ptr + (ins[k].sharded ? sh.lo * ins[k].row_bytes : 0);
          good = hipSetDevice(hctx->device) == hipSuccess &&
                 R.Send(src, bytes, ncclUint8, sh.member, (*comms)[(size_t)home], hrt) == ncclSuccess &&
                 hipSetDevice(p->ctxs[(size_t)sh.member]->device) == hipSuccess &&
                 R.Recv(st.in[k].p, bytes, ncclUint8, home, (*comms)[(size_t)sh.member], member_stream(sh.member)) == ncclSuccess;
          root->scatter_bytes += bytes;
        }
      }
      good = (R.GroupEnd() == ncclSuccess) && good;
      for (size_t q = 0; q < shards.size(); ++q)
        if (shards[q].remote) timed_end(root->ev_scatter, tix[q], member_stream(shards[q].member));
      timed_end(root->ev_home, hix, hrt);
      if (!good) {
        pool_drop_comms(p);
        return pool_fail(p, TFHE_HIP_EHIP, "RCCL scatter (ncclSend / ncclRecv) failed inside the group: communicator dropped, later calls use peer copies; the home stream may not drain");
      }
    } else {
      hipError_t e = hipSetDevice(hctx->device);
      if (e != hipSuccess) return hipfail("hipSetDevice", e, home);
      if (!root->ready || root->ready_device != hctx->device) {
        if ((e = root->ready.create(hipEventDisableTiming)) != hipSuccess) return hipfail("hipEventCreate", e, home);
        root->ready_device = hctx->device;
      }
      if ((e = hipEventRecord(root->ready, hrt)) != hipSuccess) return hipfail("hipEventRecord", e, home);
      for (const Sh &sh : shards) {
        if (!sh.remote) continue;
        tfhe_hip_pool::Stage &st = root->stage[(size_t)sh.member];
        const int ddev = p->ctxs[(size_t)sh.member]->device;
        hipStream_t ms = member_stream(sh.member);
        if ((e = hipSetDevice(ddev)) != hipSuccess) return hipfail("hipSetDevice", e, sh.member);
        if ((e = hipStreamWaitEvent(ms, root->ready, 0)) != hipSuccess) return hipfail("hipStreamWaitEvent", e, sh.member);
        const long tix = timed_begin(root->ev_scatter, sh.member, ms);
        for (int k = 0; k < 5; ++k) {
          if (!ins[k].ptr) continue;
          const size_t bytes = ins[k].sharded ? (sh.hi - sh.lo) * ins[k].row_bytes : ins[k].row_bytes;
          const unsigned char *src = (const unsigned char *)ins[k].ptr + (ins[k].sharded ? sh.lo * ins[k].row_bytes : 0);
          if ((e = hipMemcpyPeerAsync(st.in[k].p, ddev, src, hctx->device, bytes, ms)) != hipSuccess)
            return hipfail("hipMemcpyPeerAsync (scatter)", e, sh.member);
          root->scatter_bytes += bytes;
        }
        timed_end(root->ev_scatter, tix, ms);
      }
    }
  }
  // 3. compute: remote shards first (their members are idle until then), home's own shard last
  for (int pass = 0; pass < 2; ++pass)
    for (const Sh &sh : shards) {
      if ((pass == 0) != sh.remote) continue;
      const void *ptrs[5];
      void *o;
      if (sh.remote) {
        tfhe_hip_pool::Stage &st = root->stage[(size_t)sh.member];
        for (int k = 0; k < 5; ++k) ptrs[k] = ins[k].ptr ? st.in[k].p : nullptr;
        o = st.out.p;
      } else {
        for (int k = 0; k < 5; ++k)
          ptrs[k] = ins[k].ptr ? (const unsigned char *)ins[k].ptr + (ins[k].sharded ? sh.lo * ins[k].row_bytes : 0) : nullptr;
        o = (unsigned char *)out + sh.lo * out_row_bytes;
      }
      tfhe_hip_ctx *c = p->ctxs[(size_t)sh.member];
      CHK(pool_member_rc(p, c, op(c, ptrs, o, sh.hi - sh.lo, sh.remote ? (void *)member_stream(sh.member) : (void *)hs)));
    }
  // 4. gather
  if (any_remote) {
    if (comms) {
      // per shard a pair on the SENDING member's stream (its first event follows the member's compute, so the pair
      // brackets the transfer and whatever it waits for on the home side); one pair on the home stream around the
      // group's receives (which also waits for the slowest member's result)
      const long hix = timed_begin(root->ev_home, home, hrt);
      if (hix >= 0) root->ev_home[(size_t)hix].gather = true;
      std::vector<long> gix(shards.size(), -1);
      for (size_t q = 0; q < shards.size(); ++q)
        if (shards[q].remote) gix[q] = timed_begin(root->ev_gather, shards[q].member, member_stream(shards[q].member), hix);
      if (R.GroupStart() != ncclSuccess) return pool_fail(p, TFHE_HIP_EHIP, "ncclGroupStart (gather)");
      bool good = true;
      for (const Sh &sh : shards) {
        if (!sh.remote || !good) continue;
        tfhe_hip_pool::Stage &st = root->stage[(size_t)sh.member];
        const size_t bytes = (sh.hi - sh.lo) * out_row_bytes;
        good = hipSetDevice(p->ctxs[(size_t)sh.member]->device) == hipSuccess &&
               R.Send(st.out.p, bytes, ncclUint8, home, (*comms)[(size_t)sh.member], member_stream(sh.member)) == ncclSuccess &&
               hipSetDevice(hctx->device) == hipSuccess &&
               R.Recv((unsigned char *)out + sh.lo * out_row_bytes, bytes, ncclUint8, sh.member, (*comms)[(size_t)home], hrt) == ncclSuccess;
        root->gather_bytes += bytes;
      }
      good = (R.GroupEnd() == ncclSuccess) && good;
      for (size_t q = 0; q < shards.size(); ++q)
        if (shards[q].remote) timed_end(root->ev_gather, gix[q], member_stream(shards[q].member));
      timed_end(root->ev_home, hix, hrt);
      if (!good) {
        pool_drop_comms(p);
        return pool_fail(p, TFHE_HIP_EHIP, "RCCL gather (ncclSend / ncclRecv) failed inside the group: communicator dropped, later calls use peer copies; the home stream may not drain");
      }
    } else {
      for (const Sh &sh : shards) {
        if (!sh.remote) continue;
        tfhe_hip_pool::Stage &st = root->stage[(size_t)sh.member];
        const int sdev = p->ctxs[(size_t)sh.member]->device;
        hipStream_t ms = member_stream(sh.member);
        const size_t bytes = (sh.hi - sh.lo) * out_row_bytes;
        hipError_t e = hipSetDevice(sdev);
        if (e != hipSuccess) return hipfail("hipSetDevice", e, sh.member);
        const long gix = timed_begin(root->ev_gather, sh.member, ms);
        if ((e = hipMemcpyPeerAsync((unsigned char *)out + sh.lo * out_row_bytes, hctx->device, st.out.p, sdev, bytes, ms)) != hipSuccess)
          return hipfail("hipMemcpyPeerAsync (gather)", e, sh.member);
        timed_end(root->ev_gather, gix, ms);
        if ((e = hipEventRecord(st.done, ms)) != hipSuccess) return hipfail("hipEventRecord", e, sh.member);
        root->gather_bytes += bytes;
      }
      hipError_t e = hipSetDevice(hctx->device);
      if (e != hipSuccess) return hipfail("hipSetDevice", e, home);
      for (const Sh &sh : shards)
        if (sh.remote && (e = hipStreamWaitEvent(hrt, root->stage[(size_t)sh.member].done, 0)) != hipSuccess)
          return hipfail("hipStreamWaitEvent", e, home);
    }
  }
  ++root->dev_calls;
  return TFHE_HIP_OK;
}

}  // namespace

int tfhe_hip_pool_create(const tfhe_hip_params *params, const int *devices, int ndev, tfhe_hip_pool **out) {
  if (!out) return TFHE_HIP_EINVAL;
  *out = nullptr;
  if (!params || !devices || ndev <= 0 || ndev > 64) {
    g_create_error = "pool: need 1..64 devices";
    return TFHE_HIP_EINVAL;
  }
  tfhe_hip_pool *p = new tfhe_hip_pool();
  for (int i = 0; i < ndev; ++i) {
    tfhe_hip_ctx *c = nullptr;
    const int rc = tfhe_hip_ctx_create(params, devices[i], &c);
    if (rc != TFHE_HIP_OK) {  // g_create_error holds the text
      for (auto *x : p->ctxs) tfhe_hip_ctx_destroy(x);
      delete p;
      return rc;
    }
    p->ctxs.push_back(c);
  }
  // direct xGMI for the peer-copy transport (key clone, shards of the device-resident calls when no communicator is to be
  // had): peer access between every pair of distinct devices, where the topology allows it (errors are not fatal: the
  // runtime stages such copies through the host)
  {
    int prev = -1;
    (void)hipGetDevice(&prev);
    for (int i = 0; i < ndev; ++i)
      for (int j = 0; j < ndev; ++j) {
        if (devices[i] == devices[j]) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, devices[i], devices[j]) != hipSuccess || !can) continue;
        if (hipSetDevice(devices[i]) == hipSuccess) (void)hipDeviceEnablePeerAccess(devices[j], 0);
      }
    (void)hipGetLastError();  // (hipErrorPeerAccessAlreadyEnabled and the like)
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  // several members fed by one host: each stages its pageable shard through a pinned arena of its own (to_dev)
  const char *env = getenv("TFHE_HIP_POOL_PINNED_STAGING");
  const bool stage = env ? atoi(env) != 0 : ndev > 1;
  for (auto *c : p->ctxs) c->stage_pinned = stage;
  *out = p;
  return TFHE_HIP_OK;
}

void tfhe_hip_pool_destroy(tfhe_hip_pool *p) {
  if (!p) return;
  if (p->parent) {  // a key view: its keys go, everything else is the parent's
    tfhe_hip_pool *root = p->parent;
    bool last_of_dying = false;
    {
      std::lock_guard<FairMutex> lk(root->own_mu);
      for (auto *c : p->ctxs) tfhe_hip_ctx_destroy(c);  // (drains the member's queued work first)
      last_of_dying = --root->views == 0 && root->dying;
    }
    delete p;
    if (last_of_dying) tfhe_hip_pool_destroy(root);  // the parent was destroyed first: it has waited for its views
    return;
  }
  {
    // destroyed before its views (the header asks for the opposite order): they share this pool's mutex, staging and
    // communicator, so it stays alive until the last of them goes
    std::lock_guard<FairMutex> lk(p->own_mu);
    if (p->views > 0) {
      p->dying = true;
      return;
    }
  }
  int prev = -1;
  (void)hipGetDevice(&prev);
  // queued device-resident calls may still use the staging buffers and the communicator: drain the members first
  // (not after a group failed half-way: a stream that carries a send without its receive never drains)
  for (auto *c : p->ctxs) {
    if (!p->comms_dropped && hipSetDevice(c->device) == hipSuccess) (void)hipStreamSynchronize(c->stream);
  }
  if (p->comm_state == 1)
    for (ncclComm_t c : p->comms)
      if (c) (void)rccl_api().CommDestroy(c);
  for (size_t i = 0; i < p->stage.size() && i < p->ctxs.size(); ++i) {
    (void)hipSetDevice(p->ctxs[i]->device);
    p->stage[i] = tfhe_hip_pool::Stage();  // (its buffers and its event go here, on their device; the rest with `delete p`)
  }
  if (prev >= 0) (void)hipSetDevice(prev);
  for (auto *c : p->ctxs) tfhe_hip_ctx_destroy(c);
  delete p;
}

// A key view of a pool: one key view per member context (same devices, same streams and scratch, its own cloud key);
// it shares the parent's mutex, staging buffers and communicator.
int tfhe_hip_pool_key_create(tfhe_hip_pool *pool, tfhe_hip_pool **out) {
  if (!out) return TFHE_HIP_EINVAL;
  *out = nullptr;
  if (!pool) return TFHE_HIP_EINVAL;
  tfhe_hip_pool *root = pool->root();
  std::lock_guard<FairMutex> lk(root->own_mu);
  tfhe_hip_pool *v = new tfhe_hip_pool();
  v->parent = root;
  for (auto *c : root->ctxs) {
    tfhe_hip_ctx *kv = nullptr;
    const int rc = tfhe_hip_key_create(c, &kv);
    if (rc != TFHE_HIP_OK) {
      for (auto *x : v->ctxs) tfhe_hip_ctx_destroy(x);
      delete v;
      return rc;
    }
    v->ctxs.push_back(kv);
  }
  ++root->views;
  *out = v;
  return TFHE_HIP_OK;
}

int tfhe_hip_pool_size(const tfhe_hip_pool *p) { return p ? (int)p->ctxs.size() : 0; }

tfhe_hip_ctx *tfhe_hip_pool_ctx(tfhe_hip_pool *p, int i) {
  return (p && i >= 0 && (size_t)i < p->ctxs.size()) ? p->ctxs[(size_t)i] : nullptr;
}

const char *tfhe_hip_pool_last_error(const tfhe_hip_pool *p) { return p ? err_text(p->id) : g_create_error.c_str(); }

// "rccl" when the pool's last cloud key reached its members by ncclBroadcast, "peer-copy" when by hipMemcpyPeer
// (or when there was nothing to replicate).
const char *tfhe_hip_pool_key_transport(const tfhe_hip_pool *p) { return (p && p->replicated_by_rccl) ? "rccl" : "peer-copy"; }

// how the last device-resident (_dev) call moved its shards: "rccl", "peer-copy", or "none" (nothing left home)
const char *tfhe_hip_pool_data_transport(const tfhe_hip_pool *p) { return p ? p->root()->last_transport : "none"; }

int tfhe_hip_pool_members_for(const tfhe_hip_pool *p, size_t count) { return p ? pool_world_for(p, count) : 0; }

void tfhe_hip_pool_shard(size_t count, int shard, int nshards, size_t *lo, size_t *hi) {
  size_t a = 0, b = 0;
  if (nshards > 0 && shard >= 0 && shard < nshards) pool_shard(count, shard, nshards, a, b);
  if (lo) *lo = a;
  if (hi) *hi = b;
}

#define POOL_ENTER(p)               \
  if (!(p)) return TFHE_HIP_EINVAL; \
  std::lock_guard<FairMutex> plk_((p)->root()->own_mu)

// Small host-pointer calls from concurrent threads (`Send + Sync`, src/bootstrap/mod.rs:23): they do not queue on the
// pool's mutex; each goes to the member whose combining front end (combine.hpp) has the least work queued and in
// flight, where it shares launches with the other threads' calls.  (Key loads and device-resident calls keep the
// pool's mutex; as for a context, changing a key while calls under it are in flight is the caller's to avoid.)
namespace {
// (up to 256 ciphertexts: beyond that a pool call is cut over several members, pool_world_for -- two devices run 512 in the
// time one runs 256)
inline bool pool_small(const tfhe_hip_pool *p, size_t count) { return p && !p->ctxs.empty() && count <= 256 && comb_takes(p->ctxs[0], count); }
inline tfhe_hip_ctx *pool_least_loaded(tfhe_hip_pool *p) {
  // members that share a device count once (the first of them): two front ends on one GPU would launch on two streams that
  // need not overlap, and every call would wait for the other member's launch (measured on a pool of {0, 0}: 1.5 k gates/s
  // from 8 threads against 3.1 k through one member, profiles/exp/logs/r6c_front_end.log)
  tfhe_hip_ctx *best = p->ctxs[0];
  size_t best_load = ~(size_t)0;
  for (size_t i = 0; i < p->ctxs.size(); ++i) {
    tfhe_hip_ctx *c = p->ctxs[i];
    bool repeat = false;
    for (size_t j = 0; j < i && !repeat; ++j) repeat = p->ctxs[j]->device == c->device;
    if (repeat) continue;
    const tfhe_hip_ctx *base = c->parent ? c->parent : c;
    const size_t load = base->comb ? base->comb->pending.load(std::memory_order_relaxed) : 0;
    if (load < best_load) {
      best = c;
      best_load = load;
    }
  }
  return best;
}
// ---- the batch operations, each described ONCE for its host-pointer and its device-resident pool form ----------------
// An operation is its operand table (PoolIn: pointer, row size, cut with the batch or sent whole, required or not), its
// result's row size, and `run(ctx, operands, out, m, stream)`: the single-context entry point on a shard of m
// ciphertexts.  The null-pointer check, a shard's pointers, the small-call shortcut and what pool_dev_map is handed all
// come from the table (pool_host_call / pool_dev_call).
struct PoolOp {
  PoolIn in[5];                  // in the order `run` takes them
  size_t out_row_bytes;          // of the result, per ciphertext
  bool small;                    // host form: a call the combining front end takes goes whole to the least loaded member
  const char *refuse = nullptr;  // device form: turned away with this text before the pointers are looked at
};
size_t pool_tlwe_bytes(const tfhe_hip_pool *p) { return tlwe_bytes(p->ctxs[0], 1); }

bool pool_missing(const PoolOp &op, const void *out) {
  bool missing = !out;
  for (const PoolIn &in : op.in) missing = missing || (in.required && !in.ptr);
  return missing;
}
// the operands of the shard that starts at ciphertext `lo`
void pool_shard_ptrs(const PoolOp &op, size_t lo, const void *(&q)[5]) {
  for (int k = 0; k < 5; ++k) {
    const PoolIn &in = op.in[k];
    q[k] = in.ptr ? (const unsigned char *)in.ptr + (in.sharded ? lo * in.row_bytes : 0) : nullptr;
  }
}

// host pointers: one host thread per shard (pool_map), results written in place into the caller's slice
template <class Run>
int pool_host_call(tfhe_hip_pool *p, const PoolOp &op, void *out, size_t count, Run &&run) {
  const void *q[5];
  if (op.small && pool_small(p, count)) {
    if (pool_missing(op, out)) return pool_fail(p, TFHE_HIP_EINVAL, "null pointer");
    pool_shard_ptrs(op, 0, q);
    tfhe_hip_ctx *c = pool_least_loaded(p);
    return pool_member_rc(p, c, run(c, q, out, count, nullptr));
  }
  POOL_ENTER(p);
  if (count && pool_missing(op, out)) return pool_fail(p, TFHE_HIP_EINVAL, "null pointer");
  return pool_map(p, count, [&](tfhe_hip_ctx *c, size_t lo, size_t hi) {
    const void *sq[5];
    pool_shard_ptrs(op, lo, sq);
    return run(c, sq, (unsigned char *)out + lo * op.out_row_bytes, hi - lo, nullptr);
  });
}

// device pointers on member `home`'s GPU: only enqueued (pool_dev_map)
template <class Run>
int pool_dev_call(tfhe_hip_pool *p, int home, void *stream, const PoolOp &op, void *out, size_t count, Run &&run) {
  POOL_ENTER(p);
  if (op.refuse) return pool_fail(p, TFHE_HIP_EINVAL, op.refuse);
  if (count && pool_missing(op, out)) return pool_fail(p, TFHE_HIP_EINVAL, "null pointer");
  return pool_dev_map(p, home, count, stream, op.in, out, op.out_row_bytes, run);
}
template <bool DEV, class Run>
int pool_call(tfhe_hip_pool *p, int home, void *stream, const PoolOp &op, void *out, size_t count, Run &&run) {
  if constexpr (DEV) return pool_dev_call(p, home, stream, op, out, count, run);
  else return pool_host_call(p, op, out, count, run);
}

template <bool DEV>
int pool_gate(tfhe_hip_pool *p, int home, int gate, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t count,
              void *stream) {
  if (!p) return TFHE_HIP_EINVAL;
  GatePrep gp;
  const bool known = gate_prep(gate, gp);  // (an unknown gate: the device form refuses it here, the host form's member does)
  const bool has_b = !known || gp.cb;
  const size_t w = pool_tlwe_bytes(p);
  const PoolOp op{{{a, w, true, true}, {has_b ? b : nullptr, w, true, DEV && has_b}}, w, true, DEV && !known ? "unknown gate" : nullptr};
  return pool_call<DEV>(p, home, stream, op, out, count, [&](tfhe_hip_ctx *c, const void *const *q, void *o, size_t m, void *s) {
    if constexpr (DEV) return tfhe_hip_batch_gate_dev(c, gate, u32(q[0]), u32(q[1]), (uint32_t *)o, m, s);
    else return tfhe_hip_batch_gate(c, gate, u32(q[0]), u32(q[1]), (uint32_t *)o, m);
  });
}

template <bool DEV>
int pool_gates_mixed(tfhe_hip_pool *p, int home, bool keyswitch, const uint8_t *gates, const uint32_t *a, const uint32_t *b,
                     uint32_t *out, size_t count, void *stream) {
  if (!p) return TFHE_HIP_EINVAL;
  const size_t w = pool_tlwe_bytes(p);
  const PoolOp op{{{a, w, true, true}, {b, w, true, true}, {gates, 1, true, true}}, w, true};
  return pool_call<DEV>(p, home, stream, op, out, count, [&](tfhe_hip_ctx *c, const void *const *q, void *o, size_t m, void *s) {
    if constexpr (DEV)
      return (keyswitch ? tfhe_hip_batch_gates_mixed_dev : tfhe_hip_batch_gates_mixed_nks_dev)(c, (const uint8_t *)q[2], u32(q[0]), u32(q[1]), (uint32_t *)o, m, s);
    else
      return (keyswitch ? tfhe_hip_batch_gates_mixed : tfhe_hip_batch_gates_mixed_nks)(c, (const uint8_t *)q[2], u32(q[0]), u32(q[1]), (uint32_t *)o, m);
  });
}

template <bool DEV>
int pool_bootstrap(tfhe_hip_pool *p, int home, const uint32_t *in, const uint32_t *testvec, int per_ct, int keyswitch,
                   uint32_t *out, size_t count, void *stream) {
  if (!p) return TFHE_HIP_EINVAL;
  const size_t w = pool_tlwe_bytes(p);
  const PoolOp op{{{in, w, true, true}, {testvec, trlwe_bytes(1), testvec && per_ct}}, w, true};
  return pool_call<DEV>(p, home, stream, op, out, count, [&](tfhe_hip_ctx *c, const void *const *q, void *o, size_t m, void *s) {
    if constexpr (DEV) return tfhe_hip_batch_bootstrap_dev(c, u32(q[0]), u32(q[1]), per_ct, keyswitch, (uint32_t *)o, m, s);
    else return tfhe_hip_batch_bootstrap(c, u32(q[0]), u32(q[1]), per_ct, keyswitch, (uint32_t *)o, m);
  });
}

template <bool DEV>
int pool_tlwe_lincomb(tfhe_hip_pool *p, int home, uint32_t ca, const uint32_t *a, uint32_t cb, const uint32_t *b,
                      uint32_t cconst, uint32_t *out, size_t count, void *stream) {
  if (!p) return TFHE_HIP_EINVAL;
  const size_t w = pool_tlwe_bytes(p);
  const PoolOp op{{{a, w, true, true}, {cb ? b : nullptr, w, true, cb != 0}}, w, false};
  return pool_call<DEV>(p, home, stream, op, out, count, [&](tfhe_hip_ctx *c, const void *const *q, void *o, size_t m, void *s) {
    if constexpr (DEV) return tfhe_hip_batch_tlwe_lincomb_dev(c, ca, u32(q[0]), cb, u32(q[1]), cconst, (uint32_t *)o, m, s);
    else return tfhe_hip_batch_tlwe_lincomb(c, ca, u32(q[0]), cb, u32(q[1]), cconst, (uint32_t *)o, m);
  });
}

template <bool DEV>
int pool_lincomb_bootstrap(tfhe_hip_pool *p, int home, uint32_t ca, const uint32_t *a, uint32_t cb, const uint32_t *b,
                           uint32_t cconst, const uint32_t *testvec, int per_ct, int keyswitch, uint32_t *out, size_t count,
                           void *stream) {
  if (!p) return TFHE_HIP_EINVAL;
  const size_t w = pool_tlwe_bytes(p);
  const PoolOp op{{{a, w, true, true}, {cb ? b : nullptr, w, true, cb != 0}, {testvec, trlwe_bytes(1), testvec && per_ct}}, w, true};
  return pool_call<DEV>(p, home, stream, op, out, count, [&](tfhe_hip_ctx *c, const void *const *q, void *o, size_t m, void *s) {
    if constexpr (DEV)
      return tfhe_hip_batch_lincomb_bootstrap_dev(c, ca, u32(q[0]), cb, u32(q[1]), cconst, u32(q[2]), per_ct, keyswitch, (uint32_t *)o, m, s);
    else
      return tfhe_hip_batch_lincomb_bootstrap(c, ca, u32(q[0]), cb, u32(q[1]), cconst, u32(q[2]), per_ct, keyswitch, (uint32_t *)o, m);
  });
}

// Many-LUT: rows are cut as for lincomb_bootstrap (no combining: many-LUT calls are never merged), but a member's result
// is [k][m] -- function j of its shard belongs at rows j * count + lo of the caller's [k][count] -- so the table and the
// checks are shared and the placing of the results is written out.  Host form: a shard that is not the whole batch lands
// in a vector and is copied out slice by slice.  Device form: the member results travel as rows of k * (n+1) words; a
// batch that is not cut lands in `out` as it is, otherwise it is gathered into a stream-ordered scratch on home and each
// shard's k slices are put in place with one 2D copy.  (The device form looks at `home` before anything else.)
template <bool DEV>
int pool_lincomb_bootstrap_many(tfhe_hip_pool *p, int home, uint32_t ca, const uint32_t *a, uint32_t cb, const uint32_t *b,
                                uint32_t cconst, const uint32_t *testvec, int per_ct, int n_luts, int keyswitch,
                                uint32_t *out, size_t count, void *stream) {
  POOL_ENTER(p);
  if (DEV && (home < 0 || home >= (int)p->ctxs.size())) return pool_fail(p, TFHE_HIP_EINVAL, "no such pool member (home)");
  if (const char *why = many_refusal(a, cb, b, testvec, n_luts, out, count)) return pool_fail(p, TFHE_HIP_EINVAL, why);
  const size_t w = pool_tlwe_bytes(p);
  const PoolOp op{{{a, w, true, true}, {cb ? b : nullptr, w, true, cb != 0}, {testvec, trlwe_bytes(1), per_ct != 0, true}},
                  w * (size_t)n_luts, false};
  auto run = [&](tfhe_hip_ctx *c, const void *const *q, void *o, size_t m, void *s) {
    if constexpr (DEV)
      return tfhe_hip_batch_lincomb_bootstrap_many_dev(c, ca, u32(q[0]), cb, u32(q[1]), cconst, u32(q[2]), per_ct, n_luts, keyswitch, (uint32_t *)o, m, s);
    else
      return tfhe_hip_batch_lincomb_bootstrap_many(c, ca, u32(q[0]), cb, u32(q[1]), cconst, u32(q[2]), per_ct, n_luts, keyswitch, (uint32_t *)o, m);
  };
  if constexpr (!DEV) {
    return pool_map(p, count, [&](tfhe_hip_ctx *c, size_t lo, size_t hi) {
      const size_t m = hi - lo;
      const void *q[5];
      pool_shard_ptrs(op, lo, q);
      if (m == count) return run(c, q, out, m, nullptr);  // one shard: the member writes the caller's layout itself
      std::vector<unsigned char> part((size_t)n_luts * m * w);
      const int rc = run(c, q, part.data(), m, nullptr);
      if (rc != TFHE_HIP_OK) return rc;
      for (int j = 0; j < n_luts; ++j)
        memcpy((unsigned char *)out + ((size_t)j * count + lo) * w, part.data() + (size_t)j * m * w, m * w);
      return TFHE_HIP_OK;
    });
  } else {
    const int world = pool_world_for(p, count);
    if (world <= 1) return pool_dev_map(p, home, count, stream, op.in, out, op.out_row_bytes, run);
    tfhe_hip_ctx *hctx = p->ctxs[(size_t)home];
    tfhe_hip_ctx *hbase = hctx->parent ? hctx->parent : hctx;
    hipStream_t hs = stream ? (hipStream_t)stream : hbase->stream;
    hipStream_t hrt = hs == hipStreamLegacy ? (hipStream_t) nullptr : hs;  // (the runtime's name for the default stream)
    int prev = -1;
    (void)hipGetDevice(&prev);
    struct Restore {
      int d;
      ~Restore() {
        if (d >= 0) (void)hipSetDevice(d);
      }
    } restore{prev};
    if (hipSetDevice(hctx->device) != hipSuccess) return pool_fail(p, TFHE_HIP_EHIP, "hipSetDevice (home)");
    unsigned char *tmp = nullptr;
    const size_t bytes = count * op.out_row_bytes;
    if (hipMallocAsync((void **)&tmp, bytes, hrt) != hipSuccess) {
      (void)hipGetLastError();
      return pool_fail(p, TFHE_HIP_ENOMEM, "hipMallocAsync (many-LUT gather)");
    }
    int rc = pool_dev_map(p, home, count, stream, op.in, tmp, op.out_row_bytes, run);
    (void)hipSetDevice(hctx->device);
    for (int r = 0; r < world && rc == TFHE_HIP_OK; ++r) {
      size_t lo, hi;
      pool_shard(count, r, world, lo, hi);
      if (hi <= lo) continue;
      const size_t m = hi - lo;
      if (hipMemcpy2DAsync((unsigned char *)out + lo * w, count * w, tmp + lo * op.out_row_bytes, m * w, m * w, (size_t)n_luts,
                           hipMemcpyDeviceToDevice, hrt) != hipSuccess) {
        (void)hipGetLastError();
        rc = pool_fail(p, TFHE_HIP_EHIP, "hipMemcpy2DAsync (many-LUT gather)");
      }
    }
    (void)hipFreeAsync(tmp, hrt);
    return rc;
  }
}

template <bool DEV>
int pool_mux(tfhe_hip_pool *p, int home, int naive, const uint32_t *a, const uint32_t *b, const uint32_t *c3, uint32_t *out,
             size_t count, void *stream) {
  if (!p) return TFHE_HIP_EINVAL;
  const size_t w = pool_tlwe_bytes(p);
  const PoolOp op{{{a, w, true, true}, {b, w, true, true}, {c3, w, true, true}}, w, true};
  return pool_call<DEV>(p, home, stream, op, out, count, [&](tfhe_hip_ctx *c, const void *const *q, void *o, size_t m, void *s) {
    if constexpr (DEV) return tfhe_hip_batch_mux_dev(c, naive, u32(q[0]), u32(q[1]), u32(q[2]), (uint32_t *)o, m, s);
    else return tfhe_hip_batch_mux(c, naive, u32(q[0]), u32(q[1]), u32(q[2]), (uint32_t *)o, m);
  });
}

template <bool DEV>
int pool_blind_rotate(tfhe_hip_pool *p, int home, const uint32_t *in, const uint32_t *testvec, uint32_t *out_trlwe,
                      size_t count, void *stream) {
  if (!p) return TFHE_HIP_EINVAL;
  const PoolOp op{{{in, pool_tlwe_bytes(p), true, true}, {testvec, trlwe_bytes(1), false}}, trlwe_bytes(1), true};
  return pool_call<DEV>(p, home, stream, op, out_trlwe, count, [&](tfhe_hip_ctx *c, const void *const *q, void *o, size_t m, void *s) {
    if constexpr (DEV) return tfhe_hip_batch_blind_rotate_dev(c, u32(q[0]), u32(q[1]), (uint32_t *)o, m, s);
    else return tfhe_hip_batch_blind_rotate(c, u32(q[0]), u32(q[1]), (uint32_t *)o, m);
  });
}

// the key calls: made on the first member, whose key is then replicated device to device
template <class F>
int pool_key_call(tfhe_hip_pool *p, F &&on_first) {
  POOL_ENTER(p);
  CHK(pool_member_rc(p, p->ctxs[0], on_first(p->ctxs[0])));
  return replicate_key(p);
}
}  // namespace

int tfhe_hip_pool_load_cloud_key(tfhe_hip_pool *p, const double *bsk, const uint32_t *ksk, uint32_t decomp_offset,
                                 const uint32_t *testvec) {
  return pool_key_call(p, [&](tfhe_hip_ctx *c) { return tfhe_hip_load_cloud_key(c, bsk, ksk, decomp_offset, testvec); });
}

int tfhe_hip_pool_load_compressed_cloud_key(tfhe_hip_pool *p, const uint8_t mask_seed[32], const uint32_t *bsk_bodies,
                                            const uint32_t *ksk_bodies, uint32_t decomp_offset, const uint32_t *testvec) {
  return pool_key_call(p, [&](tfhe_hip_ctx *c) {
    return tfhe_hip_load_compressed_cloud_key(c, mask_seed, bsk_bodies, ksk_bodies, decomp_offset, testvec);
  });
}

int tfhe_hip_pool_gen_cloud_key_secure(tfhe_hip_pool *p, const uint32_t *key_lv0, const uint32_t *key_lv1,
                                       double alpha_ksk, double alpha_bsk) {
  return pool_key_call(p, [&](tfhe_hip_ctx *c) { return tfhe_hip_gen_cloud_key_secure(c, key_lv0, key_lv1, alpha_ksk, alpha_bsk); });
}

int tfhe_hip_pool_gen_cloud_key_with_key(tfhe_hip_pool *p, const uint32_t *key_lv0, const uint32_t *key_lv1,
                                         double alpha_ksk, double alpha_bsk, const uint8_t rng_key[32]) {
  return pool_key_call(p, [&](tfhe_hip_ctx *c) { return tfhe_hip_gen_cloud_key_with_key(c, key_lv0, key_lv1, alpha_ksk, alpha_bsk, rng_key); });
}

int tfhe_hip_pool_gen_cloud_key(tfhe_hip_pool *p, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha_ksk,
                                double alpha_bsk, uint64_t seed) {
  return pool_key_call(p, [&](tfhe_hip_ctx *c) { return tfhe_hip_gen_cloud_key(c, key_lv0, key_lv1, alpha_ksk, alpha_bsk, seed); });
}

int tfhe_hip_pool_export_cloud_key(tfhe_hip_pool *p, int member, double *bsk, uint32_t *ksk, uint32_t *decomp_offset,
                                   uint32_t *testvec) {
  POOL_ENTER(p);
  if (member < 0 || (size_t)member >= p->ctxs.size()) return pool_fail(p, TFHE_HIP_EINVAL, "no such pool member");
  tfhe_hip_ctx *c = p->ctxs[(size_t)member];
  return pool_member_rc(p, c, tfhe_hip_export_cloud_key(c, bsk, ksk, decomp_offset, testvec));
}

// ---- the batch entry points: host pointers, then device pointers on member `home`'s GPU (operations: above) --------
int tfhe_hip_pool_batch_gate(tfhe_hip_pool *p, int gate, const uint32_t *a, const uint32_t *b, uint32_t *out,
                             size_t count) {
  return pool_gate<false>(p, 0, gate, a, b, out, count, nullptr);
}
int tfhe_hip_pool_batch_gates_mixed(tfhe_hip_pool *p, const uint8_t *gates, const uint32_t *a, const uint32_t *b,
                                    uint32_t *out, size_t count) {
  return pool_gates_mixed<false>(p, 0, true, gates, a, b, out, count, nullptr);
}
int tfhe_hip_pool_batch_gates_mixed_nks(tfhe_hip_pool *p, const uint8_t *gates, const uint32_t *a, const uint32_t *b,
                                        uint32_t *out, size_t count) {
  return pool_gates_mixed<false>(p, 0, false, gates, a, b, out, count, nullptr);
}
int tfhe_hip_pool_batch_bootstrap(tfhe_hip_pool *p, const uint32_t *in, const uint32_t *testvec, int per_ct,
                                  int keyswitch, uint32_t *out, size_t count) {
  return pool_bootstrap<false>(p, 0, in, testvec, per_ct, keyswitch, out, count, nullptr);
}
int tfhe_hip_pool_batch_tlwe_lincomb(tfhe_hip_pool *p, uint32_t ca, const uint32_t *a, uint32_t cb, const uint32_t *b,
                                     uint32_t cconst, uint32_t *out, size_t count) {
  return pool_tlwe_lincomb<false>(p, 0, ca, a, cb, b, cconst, out, count, nullptr);
}
int tfhe_hip_pool_batch_lincomb_bootstrap(tfhe_hip_pool *p, uint32_t ca, const uint32_t *a, uint32_t cb,
                                          const uint32_t *b, uint32_t cconst, const uint32_t *testvec, int per_ct,
                                          int keyswitch, uint32_t *out, size_t count) {
  return pool_lincomb_bootstrap<false>(p, 0, ca, a, cb, b, cconst, testvec, per_ct, keyswitch, out, count, nullptr);
}
int tfhe_hip_pool_batch_lincomb_bootstrap_many(tfhe_hip_pool *p, uint32_t ca, const uint32_t *a, uint32_t cb,
                                               const uint32_t *b, uint32_t cconst, const uint32_t *testvec, int per_ct,
                                               int n_luts, int keyswitch, uint32_t *out, size_t count) {
  return pool_lincomb_bootstrap_many<false>(p, 0, ca, a, cb, b, cconst, testvec, per_ct, n_luts, keyswitch, out, count, nullptr);
}
int tfhe_hip_pool_batch_mux(tfhe_hip_pool *p, int naive, const uint32_t *a, const uint32_t *b, const uint32_t *c3,
                            uint32_t *out, size_t count) {
  return pool_mux<false>(p, 0, naive, a, b, c3, out, count, nullptr);
}
int tfhe_hip_pool_batch_blind_rotate(tfhe_hip_pool *p, const uint32_t *in, const uint32_t *testvec, uint32_t *out_trlwe,
                                     size_t count) {
  return pool_blind_rotate<false>(p, 0, in, testvec, out_trlwe, count, nullptr);
}

int tfhe_hip_pool_batch_gate_dev(tfhe_hip_pool *p, int home, int gate, const uint32_t *a, const uint32_t *b,
                                 uint32_t *out, size_t count, void *stream) {
  return pool_gate<true>(p, home, gate, a, b, out, count, stream);
}
int tfhe_hip_pool_batch_gates_mixed_dev(tfhe_hip_pool *p, int home, const uint8_t *gates, const uint32_t *a,
                                        const uint32_t *b, uint32_t *out, size_t count, void *stream) {
  return pool_gates_mixed<true>(p, home, true, gates, a, b, out, count, stream);
}
int tfhe_hip_pool_batch_gates_mixed_nks_dev(tfhe_hip_pool *p, int home, const uint8_t *gates, const uint32_t *a,
                                            const uint32_t *b, uint32_t *out, size_t count, void *stream) {
  return pool_gates_mixed<true>(p, home, false, gates, a, b, out, count, stream);
}
int tfhe_hip_pool_batch_bootstrap_dev(tfhe_hip_pool *p, int home, const uint32_t *in, const uint32_t *testvec, int per_ct,
                                      int keyswitch, uint32_t *out, size_t count, void *stream) {
  return pool_bootstrap<true>(p, home, in, testvec, per_ct, keyswitch, out, count, stream);
}
int tfhe_hip_pool_batch_tlwe_lincomb_dev(tfhe_hip_pool *p, int home, uint32_t ca, const uint32_t *a, uint32_t cb,
                                         const uint32_t *b, uint32_t cconst, uint32_t *out, size_t count, void *stream) {
  return pool_tlwe_lincomb<true>(p, home, ca, a, cb, b, cconst, out, count, stream);
}
int tfhe_hip_pool_batch_lincomb_bootstrap_dev(tfhe_hip_pool *p, int home, uint32_t ca, const uint32_t *a, uint32_t cb,
                                              const uint32_t *b, uint32_t cconst, const uint32_t *testvec, int per_ct,
                                              int keyswitch, uint32_t *out, size_t count, void *stream) {
  return pool_lincomb_bootstrap<true>(p, home, ca, a, cb, b, cconst, testvec, per_ct, keyswitch, out, count, stream);
}
int tfhe_hip_pool_batch_lincomb_bootstrap_many_dev(tfhe_hip_pool *p, int home, uint32_t ca, const uint32_t *a, uint32_t cb,
                                                   const uint32_t *b, uint32_t cconst, const uint32_t *testvec,
                                                   int per_ct, int n_luts, int keyswitch, uint32_t *out, size_t count,
                                                   void *stream) {
  return pool_lincomb_bootstrap_many<true>(p, home, ca, a, cb, b, cconst, testvec, per_ct, n_luts, keyswitch, out, count, stream);
}
int tfhe_hip_pool_batch_mux_dev(tfhe_hip_pool *p, int home, int naive, const uint32_t *a, const uint32_t *b,
                                const uint32_t *c3, uint32_t *out, size_t count, void *stream) {
  return pool_mux<true>(p, home, naive, a, b, c3, out, count, stream);
}
int tfhe_hip_pool_batch_blind_rotate_dev(tfhe_hip_pool *p, int home, const uint32_t *in, const uint32_t *testvec,
                                         uint32_t *out_trlwe, size_t count, void *stream) {
  return pool_blind_rotate<true>(p, home, in, testvec, out_trlwe, count, stream);
}

// Block until every member has finished what the pool's *_dev calls enqueued (home streams passed by the caller are
// the caller's to synchronise; the members' own streams are drained here).
int tfhe_hip_pool_synchronize(tfhe_hip_pool *p) {
  POOL_ENTER(p);
  for (auto *c : p->ctxs) CHK(pool_member_rc(p, c, tfhe_hip_synchronize(c)));
  return TFHE_HIP_OK;
}

int tfhe_hip_pool_set_profiling(tfhe_hip_pool *p, int enabled) {
  POOL_ENTER(p);
  p->root()->timing = enabled != 0;
  for (auto *c : p->ctxs) CHK(pool_member_rc(p, c, tfhe_hip_set_profiling(c, enabled)));
  return TFHE_HIP_OK;
}

int tfhe_hip_pool_get_transfer_times(tfhe_hip_pool *p, tfhe_hip_pool_transfer_times *out) {
  if (!out) return TFHE_HIP_EINVAL;
  POOL_ENTER(p);
  tfhe_hip_pool *root = p->root();
  memset(out, 0, sizeof(*out));
  int prev = -1;
  (void)hipGetDevice(&prev);
  auto elapsed = [&](tfhe_hip_pool::Timed &t) -> double {  // < 0: not measurable
    (void)hipSetDevice(root->ctxs[(size_t)t.member]->device);
    float ms = 0.f;
    if (hipEventSynchronize(t.b) == hipSuccess && hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) return (double)ms;
    (void)hipGetLastError();
    return -1.0;
  };
  std::vector<double> home_ms(root->ev_home.size(), -1.0);
  for (size_t i = 0; i < root->ev_home.size(); ++i) home_ms[i] = elapsed(root->ev_home[i]);
  // between(x, y): ms from event x to event y on ONE device (negative when y fired first), -1e30 if not measurable
  auto between = [&](hipEvent_t x, hipEvent_t y) -> double {
    float ms = 0.f;
    if (hipEventSynchronize(x) == hipSuccess && hipEventSynchronize(y) == hipSuccess && hipEventElapsedTime(&ms, x, y) == hipSuccess)
      return (double)ms;
    (void)hipGetLastError();
    return -1e30;
  };
  auto drain = [&](std::vector<tfhe_hip_pool::Timed> &v, double &sum, double &mx) {
    for (auto &t : v) {
      double ms = elapsed(t);
      if (t.home_ix >= 0 && (size_t)t.home_ix < home_ms.size()) {
        tfhe_hip_pool::Timed &h = root->ev_home[(size_t)t.home_ix];
        const bool same_device = root->ctxs[(size_t)h.member]->device == root->ctxs[(size_t)t.member]->device;
        const double ab = same_device ? between(t.a, h.a) : -1e30, bb = same_device ? between(t.b, h.b) : -1e30;
        if (ab > -1e29 && bb > -1e29) {
          // both brackets on ONE device (a pool that repeats a device, the self send / receive of the plumbing test): the
          // events are comparable, so the transfer is measured exactly -- from the moment the LATER end arrived to the
          // moment the later end finished (a self copy runs inside only one of the two RCCL kernels)
          const double span = between(ab >= 0 ? h.a : t.a, bb >= 0 ? h.b : t.b);
          if (span > -1e29) ms = span;
        } else if (home_ms[(size_t)t.home_ix] >= 0 && (ms < 0 || home_ms[(size_t)t.home_ix] < ms)) {
          // different devices: event times are not comparable; the shorter bracket (see tfhe_hip_pool::Timed)
          ms = home_ms[(size_t)t.home_ix];
        }
      }
      if (ms >= 0) {
        sum += ms;
        if (ms > mx) mx = ms;
      }
    }
    v.clear();
  };
  drain(root->ev_scatter, out->scatter_ms_sum, out->scatter_ms_max);
  drain(root->ev_gather, out->gather_ms_sum, out->gather_ms_max);
  // the home-stream brackets on their own: one per call and direction, around the whole RCCL group (all peers' transfers,
  // and for a gather the wait for the slowest member's compute) -- an upper bound of any one transfer in it
  for (size_t i = 0; i < root->ev_home.size(); ++i)
    if (home_ms[i] >= 0) (root->ev_home[i].gather ? out->gather_group_ms_sum : out->scatter_group_ms_sum) += home_ms[i];
  root->ev_home.clear();
  if (prev >= 0) (void)hipSetDevice(prev);
  out->scatter_bytes = root->scatter_bytes;
  out->gather_bytes = root->gather_bytes;
  out->calls = root->dev_calls;
  out->comm_create_ms = root->comm_create_ms;
  out->key_replication_ms = root->key_replication_ms;
  root->scatter_bytes = root->gather_bytes = root->dev_calls = 0;
  return TFHE_HIP_OK;
}
// ---- packing key switch (packing.hpp): whole groups of N per member, in input order ----------------------------------------------------------
int tfhe_hip_pool_load_packing_key(tfhe_hip_pool *p, const uint8_t mask_seed[32], const uint32_t *bodies) {
  POOL_ENTER(p);
  // every member expands the bodies itself (no cloud key, nothing to replicate)
  for (auto *c : p->ctxs) CHK(pool_member_rc(p, c, tfhe_hip_load_packing_key(c, mask_seed, bodies)));
  return TFHE_HIP_OK;
}

// (packing_keygen.hpp) Generated on the first member; every other member loads the same (S, bodies).
int tfhe_hip_pool_gen_packing_key(tfhe_hip_pool *p, const uint32_t *key_lv0, const uint32_t *key_lv1, double alpha,
                                  const uint8_t rng_key[32], uint8_t mask_seed[32], uint32_t *bodies) {
  if (!p) return TFHE_HIP_EINVAL;
  std::lock_guard<FairMutex> plk(p->root()->own_mu);
  if (!mask_seed) return pool_fail(p, TFHE_HIP_EINVAL, "null pointer");
  tfhe_hip_ctx *first = p->ctxs[0];
  std::vector<uint32_t> own;  // the bodies the other members load when the caller keeps none
  if (!bodies && p->ctxs.size() > 1) {
    own.resize((size_t)first->P.n * first->P.t * kN);
    bodies = own.data();
  }
  CHK(pool_member_rc(p, first, tfhe_hip_gen_packing_key(first, key_lv0, key_lv1, alpha, rng_key, mask_seed, bodies)));
  for (size_t m = 1; m < p->ctxs.size(); ++m)
    CHK(pool_member_rc(p, p->ctxs[m], tfhe_hip_load_packing_key(p->ctxs[m], mask_seed, bodies)));
  return TFHE_HIP_OK;
}

int tfhe_hip_pool_batch_pack_tlwe(tfhe_hip_pool *p, const uint32_t *in, size_t count, uint32_t *out) {
  POOL_ENTER(p);
  if (count == 0) {  // a member's checks (ENOKEY first), nothing to run
    return pool_member_rc(p, p->ctxs[0], tfhe_hip_batch_pack_tlwe(p->ctxs[0], in, 0, out));
  }
  if (!in || !out) return pool_fail(p, TFHE_HIP_EINVAL, "null pointer");
  const size_t w = (size_t)p->ctxs[0]->P.n + 1, groups = (count + kN - 1) / kN;
  const int world = (int)(groups < p->ctxs.size() ? groups : p->ctxs.size());
  return pool_map(p, groups, [&](tfhe_hip_ctx *c, size_t lo, size_t hi) {
    const size_t m_hi = hi * kN < count ? hi * kN : count;
    return tfhe_hip_batch_pack_tlwe(c, in + lo * kN * w, m_hi - lo * kN, out + lo * (size_t)2 * kN);
  }, world);
}

int tfhe_hip_pool_batch_pack_tlwe_dev(tfhe_hip_pool *p, int home, const uint32_t *in, size_t count, uint32_t *out,
                                      void *stream) {
  POOL_ENTER(p);
  if (home < 0 || home >= (int)p->ctxs.size()) return pool_fail(p, TFHE_HIP_EINVAL, "no such pool member (home)");
  if (count == 0) {
    // (a failure is reported with the FIRST member's device and text, whichever member is home)
    CHK(pool_member_rc(p, p->ctxs[0], tfhe_hip_batch_pack_tlwe_dev(p->ctxs[(size_t)home], in, 0, out, stream)));
    p->root()->last_transport = "none";
    return TFHE_HIP_OK;
  }
  if (!in || !out) return pool_fail(p, TFHE_HIP_EINVAL, "null pointer");
  // the whole groups go through the grouped scatter / gather; a last partial group (shorter than a group's rows, so it
  // cannot travel as one) is packed on home, on the same stream, after home's own shard
  const size_t w = (size_t)p->ctxs[0]->P.n + 1, full = count / kN, tail = count - full * kN;
  const PoolIn ins[5] = {{in, kN * w * 4, true}, {}, {}, {}, {}};
  const int world = (int)(full < p->ctxs.size() ? full : p->ctxs.size());
  CHK(pool_dev_map(p, home, full, stream, ins, out, (size_t)2 * kN * 4, [&](tfhe_hip_ctx *c, const void *const *q, void *o, size_t m, void *s) {
    return tfhe_hip_batch_pack_tlwe_dev(c, (const uint32_t *)q[0], m * kN, (uint32_t *)o, s);
  }, world));
  if (tail) {
    tfhe_hip_ctx *c = p->ctxs[(size_t)home];
    return pool_member_rc(p, c, tfhe_hip_batch_pack_tlwe_dev(c, in + full * kN * w, tail, out + full * (size_t)2 * kN, stream));
  }
  return TFHE_HIP_OK;
}

// ---- unpacking key switch (unpack.hpp): slots == NULL cuts on group boundaries, a selection splits the outputs ----------
int tfhe_hip_pool_batch_unpack_trlwe(tfhe_hip_pool *p, const uint32_t *trlwe, size_t groups, const uint32_t *slots,
                                     size_t count, uint32_t *out) {
  POOL_ENTER(p);
  tfhe_hip_ctx *c0 = p->ctxs[0];
  // the checks that need the whole call are a member's (ENOKEY first): an empty or refused batch ends here
  if (count == 0 || !trlwe || !out || (!slots && count > groups * (size_t)kN) || (slots && groups == 0))
    return pool_member_rc(p, c0, tfhe_hip_batch_unpack_trlwe(c0, trlwe, groups, slots, count, out));
  const size_t w = (size_t)c0->P.n + 1;
  if (slots)  // every member reads the groups its slots name: all of them travel (a member checks its own entries)
    return pool_map(p, count, [&](tfhe_hip_ctx *c, size_t lo, size_t hi) {
      return tfhe_hip_batch_unpack_trlwe(c, trlwe, groups, slots + lo, hi - lo, out + lo * w);
    });
  const size_t used = (count + kN - 1) / kN;
  const int world = (int)(used < p->ctxs.size() ? used : p->ctxs.size());
  return pool_map(p, used, [&](tfhe_hip_ctx *c, size_t lo, size_t hi) {
    const size_t m_hi = hi * kN < count ? hi * kN : count;
    return tfhe_hip_batch_unpack_trlwe(c, trlwe + lo * (size_t)2 * kN, hi - lo, nullptr, m_hi - lo * kN, out + lo * kN * w);
  }, world);
}

int tfhe_hip_pool_batch_unpack_trlwe_dev(tfhe_hip_pool *p, int home, const uint32_t *trlwe, size_t groups,
                                         const uint32_t *slots, size_t count, uint32_t *out, void *stream) {
  POOL_ENTER(p);
  if (home < 0 || home >= (int)p->ctxs.size()) return pool_fail(p, TFHE_HIP_EINVAL, "no such pool member (home)");
  tfhe_hip_ctx *hc = p->ctxs[(size_t)home];
  if (count == 0 || !trlwe || !out || (!slots && count > groups * (size_t)kN) || (slots && groups == 0)) {
    // home's checks, nothing to run (a failure is reported with the FIRST member's device and text, whichever member is home)
    CHK(pool_member_rc(p, p->ctxs[0], tfhe_hip_batch_unpack_trlwe_dev(hc, trlwe, groups, slots, count, out, stream)));
    p->root()->last_transport = "none";
    return TFHE_HIP_OK;
  }
  const size_t w = (size_t)hc->P.n + 1;
  if (slots) {
    const PoolIn ins[5] = {{trlwe, groups * (size_t)2 * kN * 4, false}, {slots, 4, true}, {}, {}, {}};
    return pool_dev_map(p, home, count, stream, ins, out, w * 4, [&](tfhe_hip_ctx *c, const void *const *q, void *o, size_t m, void *s) {
      return tfhe_hip_batch_unpack_trlwe_dev(c, (const uint32_t *)q[0], groups, (const uint32_t *)q[1], m, (uint32_t *)o, s);
    });
  }
  // whole groups through the grouped scatter / gather; the outputs of a last partial group (fewer than a group's rows,
  // so they cannot travel as one) are made on home, on the same stream, after home's own shard
  const size_t full = count / kN, tail = count - full * kN;
  const PoolIn ins[5] = {{trlwe, (size_t)2 * kN * 4, true}, {}, {}, {}, {}};
  const int world = (int)(full < p->ctxs.size() ? full : p->ctxs.size());
  CHK(pool_dev_map(p, home, full, stream, ins, out, kN * w * 4, [&](tfhe_hip_ctx *c, const void *const *q, void *o, size_t m, void *s) {
    return tfhe_hip_batch_unpack_trlwe_dev(c, (const uint32_t *)q[0], m, nullptr, m * kN, (uint32_t *)o, s);
  }, world));
  if (tail)
    return pool_member_rc(p, hc, tfhe_hip_batch_unpack_trlwe_dev(hc, trlwe + full * (size_t)2 * kN, 1, nullptr, tail, out + full * kN * w, stream));
  return TFHE_HIP_OK;
}

// ---- tree bootstrap (table.hpp) ------------------------------------------------------------------------------------------------
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
#undef POOL_ENTER
