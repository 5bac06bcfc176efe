// resources.hpp -- one owner for each kind of thing the host side allocates (host code only): a device buffer, a pinned
// arena, an event, the timing pairs of a kernel family, and the claim under which the context's scratch is sized.
// Each frees itself; nothing outside this file calls the runtime's free or destroy.  tests/cpp/test_resources.cpp runs
// this file as it is, over stand-ins for the runtime: the including file supplies the HIP names and the std:: headers.
// Nothing here knows the context.  The types are shared between the library's translation units (internal.hpp): none
// is in an anonymous namespace.
#pragma once

// A failed runtime call: `what` is the text the library has always reported for that call (nullptr: an allocation,
// whose text and code are the caller's).
struct HipErr {
  hipError_t e = hipSuccess;
  const char *what = nullptr;
  explicit operator bool() const { return e != hipSuccess; }
};

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) release(), p = std::exchange(o.p, nullptr), cap = std::exchange(o.cap, 0);
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr, cap = 0;
  }
  // At least `bytes`: nothing is asked of the runtime while they fit; otherwise the old memory goes and a quarter more
  // than asked is allocated (`exact`: just `bytes`).  A failed allocation leaves the buffer empty.
  hipError_t grow(size_t bytes, bool exact = false) {
    if (bytes <= cap) return hipSuccess;
    release();
    const size_t want = exact ? bytes : bytes + bytes / 4;
    const hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) p = nullptr;
    else cap = want;
    return e;
  }
};
// a DevBuf that reads as the T* the kernels take
template <class T>
struct DevArray : DevBuf {
  operator T *() const { return (T *)p; }
};

inline void pinned_free(void *p) {  // memory of hipHostMalloc
  if (p) (void)hipHostFree(p);
}

struct PinBuf {  // pinned host arena (hipHostMalloc)
  void *p = nullptr;
  size_t cap = 0;
  bool heap = false;  // front-end lanes only: pinned memory was not to be had, this is ordinary memory (copies still work)
  PinBuf() = default;
  PinBuf(PinBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)), heap(std::exchange(o.heap, false)) {}
  PinBuf &operator=(PinBuf &&o) noexcept {
    if (this != &o) release(), p = std::exchange(o.p, nullptr), cap = std::exchange(o.cap, 0), heap = std::exchange(o.heap, false);
    return *this;
  }
  ~PinBuf() { release(); }
  void release() {
    if (heap) free(p);
    else pinned_free(p);
    p = nullptr, cap = 0, heap = false;
  }
  // DevBuf's rule with a quarter of slack.  Pinned memory first (not again once an arena has had to be ordinary
  // memory); where that fails and `allow_heap` is set, page-aligned ordinary memory.  false: no arena.
  bool grow(size_t bytes, bool allow_heap) {
    if (bytes <= cap) return true;
    const bool try_pinned = !heap;
    release();
    const size_t want = bytes + bytes / 4;
    if (try_pinned) {
      if (hipHostMalloc(&p, want, hipHostMallocDefault) == hipSuccess) {
        cap = want;
        return true;
      }
      (void)hipGetLastError();
      p = nullptr;
    }
    if (!allow_heap) return false;
    p = aligned_alloc(4096, (want + 4095) & ~(size_t)4095);
    if (!p) return false;
    cap = want;
    heap = true;
    return true;
  }
};

struct Staging {  // a host-API staging buffer on the device and the pinned arena behind it
  DevBuf dev;
  PinBuf pin;
  bool pool_pinned = false;  // pool members route large pageable copies of this slot through `pin`
};

// ---- scratch -----------------------------------------------------------------------------------------------------------
// Buffers that belong to a context, not to a call.  Work queued on one stream may still be using them when the next
// call arrives on another stream, so they are sized through Scratch::take alone, which drains the previous owner first
// (same-stream calls are ordered by the stream itself and pay nothing).  A ScratchBuf can be read by anyone and is no
// DevBuf to anyone else: growing one without the claim does not compile.
class ScratchBuf : private DevBuf {
 public:
  using DevBuf::cap;
  using DevBuf::p;
  friend struct Scratch;
};
struct Scratch {
  hipStream_t owner{};  // stream whose queued work may still use the scratch
  bool owned = false;
  HipErr claim(hipStream_t s) {
    if (owned && owner != s)
      if (const hipError_t e = hipStreamSynchronize(owner)) return {e, "hipStreamSynchronize(ctx->scratch_owner)"};
    owner = s;
    owned = true;
    return {};
  }
  // claim, then grow; where the synchronise fails nothing is sized
  HipErr take(hipStream_t s, ScratchBuf &b, size_t bytes, bool exact = false) {
    if (const HipErr r = claim(s)) return r;
    return {b.grow(bytes, exact), nullptr};
  }
};

// ---- events ------------------------------------------------------------------------------------------------------------
struct OwnEvent {
  hipEvent_t e = nullptr;
  OwnEvent() = default;
  OwnEvent(OwnEvent &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
  OwnEvent &operator=(OwnEvent &&o) noexcept {
    if (this != &o) reset(), e = std::exchange(o.e, nullptr);
    return *this;
  }
  ~OwnEvent() { reset(); }
  void reset() {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  hipError_t create(unsigned flags = hipEventDefault) {
    reset();
    const hipError_t r = hipEventCreateWithFlags(&e, flags);
    if (r != hipSuccess) e = nullptr;
    return r;
  }
  operator hipEvent_t() const { return e; }
};

// The timing pairs of one kernel family, oldest first: every pair in here is live, and has both events created and the
// first recorded.
class EventPairs {
 public:
  // a new pair, its first event recorded on `s`; on any failure what was made is destroyed and nothing is added
  HipErr open(hipStream_t s) {
    OwnEvent a, b;
    if (const hipError_t e = a.create()) return {e, "hipEventCreate(&a)"};
    if (const hipError_t e = b.create()) return {e, "hipEventCreate(&b)"};
    if (const hipError_t e = hipEventRecord(a.e, s)) return {e, "hipEventRecord(a, s)"};
    v_.emplace_back(std::move(a), std::move(b));
    return {};
  }
  // the second event of the newest pair
  HipErr close(hipStream_t s) { return {hipEventRecord(v_.back().second.e, s), "hipEventRecord(v.back().second, s)"}; }
  // Each pair in turn: wait for it, add its time to `ms` (and one to `count`), destroy it.  A failure stops there and
  // leaves that pair and the later ones, all live.
  HipErr drain(double &ms, uint64_t *count = nullptr) {
    while (!v_.empty()) {
      const hipEvent_t a = v_.front().first.e, b = v_.front().second.e;
      if (const hipError_t e = hipEventSynchronize(b)) return {e, "hipEventSynchronize(p.second)"};
      float t = 0.f;
      if (const hipError_t e = hipEventElapsedTime(&t, a, b)) return {e, "hipEventElapsedTime(&t, p.first, p.second)"};
      ms += (double)t;
      if (count) ++*count;
      v_.pop_front();
    }
    return {};
  }
  size_t size() const { return v_.size(); }

 private:
  std::deque<std::pair<OwnEvent, OwnEvent>> v_;
};

// One timed stretch of a stream: while `on`, a pair of `v` opened here and closed when the scope is left, whichever way.
// `err` is the open's failure (the scope then times nothing); close() closes now and tells how that went.
class TimedScope {
 public:
  TimedScope(EventPairs &v, hipStream_t s, bool on) : v_(on ? &v : nullptr), s_(s) {
    if (v_ && (err = v_->open(s))) v_ = nullptr;
  }
  TimedScope(const TimedScope &) = delete;
  TimedScope &operator=(const TimedScope &) = delete;
  ~TimedScope() { (void)close(); }
  HipErr close() {  // once
    EventPairs *v = v_;
    v_ = nullptr;
    return v ? v->close(s_) : HipErr{};
  }
  HipErr err;

 private:
  EventPairs *v_;
  hipStream_t s_;
};
