// The owning types of rs-tfhe_amd/csrc/resources.hpp as the library compiles them, over stand-ins for the HIP runtime:
// device, pinned and heap memory are malloc'd blocks and events are heap objects, each kept in a set of live ones, every
// call is logged, and a switch makes the k-th fallible call fail (the frees and destroys always succeed).  Built and run
// by tests/test_resources_host.py, once more under AddressSanitizer + UBSan.
//
// Every scenario is run with no failure and then once for every k up to the number of fallible calls it makes; after
// each run nothing is live, nothing was freed or destroyed twice and nothing was used after it was freed.  Then the
// rules, one by one: how buffers and arenas grow, what take() synchronises, that a timed scope closes its pair exactly
// once, what a failed drain leaves behind, and that a moved-from owner frees nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <set>
#include <string>
#include <utility>
#include <vector>

typedef int hipStream_t;  // a stream is a number here
struct EventObj {
  int recorded_on = -1;  // the stream of its last record
  int records = 0;
};
typedef EventObj *hipEvent_t;
enum hipError_t { hipSuccess = 0, hipErrorStandIn = 1 };
enum { hipHostMallocDefault = 0, hipEventDefault = 0, hipEventDisableTiming = 2 };

struct Call {
  char op;  // 'M' hipMalloc 'F' hipFree 'P' hipHostMalloc 'Q' hipHostFree 'H' aligned_alloc 'h' free
            // 'C' event create 'D' destroy 'R' record 'W' event synchronise 'T' elapsed time 'S' stream synchronise
  const void *p;
  size_t n;  // bytes, or the stream
};
static std::vector<Call> g_log;
static std::set<void *> g_dev, g_pin, g_heap;
static std::set<hipEvent_t> g_events;
static long g_fallible = 0, g_fail_at = 0;  // the g_fail_at-th fallible call fails (0: none)
static bool g_no_pinned = false;            // every hipHostMalloc fails
static int g_bad = 0;

#define EXPECT(cond)                                     \
  do {                                                   \
    if (!(cond)) {                                       \
      ++g_bad;                                           \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
    }                                                    \
  } while (0)

static bool fails() { return ++g_fallible == g_fail_at; }
static bool live(hipEvent_t e) {
  const bool ok = g_events.count(e) != 0;
  EXPECT(ok);  // used after it was destroyed, or never created
  return ok;
}

static hipError_t hipGetLastError() { return hipSuccess; }
static hipError_t hipMalloc(void **p, size_t bytes) {
  g_log.push_back({'M', nullptr, bytes});
  if (fails()) return hipErrorStandIn;
  g_dev.insert(*p = malloc(bytes ? bytes : 1));
  return hipSuccess;
}
static hipError_t hipFree(void *p) {
  g_log.push_back({'F', p, 0});
  EXPECT(g_dev.erase(p) == 1);  // freed twice, or not device memory
  free(p);
  return hipSuccess;
}
static hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) {
  g_log.push_back({'P', nullptr, bytes});
  if (fails() || g_no_pinned) return hipErrorStandIn;
  g_pin.insert(*p = malloc(bytes ? bytes : 1));
  return hipSuccess;
}
static hipError_t hipHostFree(void *p) {
  g_log.push_back({'Q', p, 0});
  EXPECT(g_pin.erase(p) == 1);  // freed twice, or not pinned memory
  free(p);
  return hipSuccess;
}
static void *standin_aligned_alloc(size_t align, size_t bytes) {
  g_log.push_back({'H', nullptr, bytes});
  EXPECT(align == 4096 && bytes % 4096 == 0);
  if (fails()) return nullptr;
  void *p = aligned_alloc(align, bytes);
  g_heap.insert(p);
  return p;
}
static void standin_free(void *p) {
  if (!p) return;
  g_log.push_back({'h', p, 0});
  EXPECT(g_heap.erase(p) == 1);  // freed twice, or not ordinary memory
  free(p);
}
static hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
  g_log.push_back({'C', nullptr, 0});
  if (fails()) return hipErrorStandIn;
  g_events.insert(*e = new EventObj());
  return hipSuccess;
}
static hipError_t hipEventDestroy(hipEvent_t e) {
  g_log.push_back({'D', e, 0});
  EXPECT(g_events.erase(e) == 1);  // destroyed twice
  delete e;
  return hipSuccess;
}
static hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  g_log.push_back({'R', e, (size_t)s});
  if (!live(e) || fails()) return hipErrorStandIn;
  e->recorded_on = s;
  ++e->records;
  return hipSuccess;
}
static hipError_t hipEventSynchronize(hipEvent_t e) {
  g_log.push_back({'W', e, 0});
  if (!live(e) || fails()) return hipErrorStandIn;
  return hipSuccess;  // (at once for an event that was never recorded, as the runtime does)
}
static hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b) {
  g_log.push_back({'T', a, 0});
  if (!live(a) || !live(b) || fails() || !a->records || !b->records) return hipErrorStandIn;  // (a pair never closed has no time)
  EXPECT(a->records == 1 && b->records == 1 && a->recorded_on == b->recorded_on);
  *ms = 1.0f + (float)a->recorded_on;  // a pair on stream s took 1 + s ms
  return hipSuccess;
}
static hipError_t hipStreamSynchronize(hipStream_t s) {
  g_log.push_back({'S', nullptr, (size_t)s});
  return fails() ? hipErrorStandIn : hipSuccess;
}

#define aligned_alloc(a, n) standin_aligned_alloc(a, n)
#define free(p) standin_free(p)
#include "../../rs-tfhe_amd/csrc/resources.hpp"
#undef aligned_alloc
#undef free

static void reset(long fail_at = 0) {
  g_log.clear();
  g_fallible = 0;
  g_fail_at = fail_at;
  g_no_pinned = false;
}
static long count_ops(char op) {
  long n = 0;
  for (const Call &c : g_log) n += c.op == op;
  return n;
}
static long first_of(char op) {
  for (size_t i = 0; i < g_log.size(); ++i)
    if (g_log[i].op == op) return (long)i;
  return -1;
}
static bool nothing_live() { return g_dev.empty() && g_pin.empty() && g_heap.empty() && g_events.empty(); }

// ---- scenarios: whatever fails, the owners leave nothing behind --------------------------------------------------------
constexpr hipStream_t kA = 3, kB = 5;

static void buffers_scenario() {
  DevBuf a, b;
  (void)a.grow(100);
  (void)a.grow(50);
  (void)a.grow(1000);
  (void)b.grow(64, true);
  DevBuf c(std::move(a));
  b = std::move(c);
  (void)b.grow(5000, true);
  DevArray<uint32_t> d;
  (void)d.grow(16, true);
  Staging s, t{{}, {}, true};
  (void)s.dev.grow(256);
  (void)s.pin.grow(256, false);
  (void)s.pin.grow(4096, false);
  (void)t.pin.grow(100, true);
  g_no_pinned = true;
  (void)t.pin.grow(1000, true);  // falls back to ordinary memory ...
  (void)t.pin.grow(9000, true);  // ... and stays there
  g_no_pinned = false;
  Staging u(std::move(t));
  s = std::move(u);
  std::vector<Staging> v(3);
  (void)v[1].dev.grow(10);
  v.resize(40);  // (reallocates: every slot is moved)
  (void)v[39].pin.grow(10, true);
}

static void scratch_scenario() {
  Scratch sc;
  ScratchBuf lv1, u1;
  (void)sc.take(kA, lv1, 100);
  (void)sc.take(kA, u1, 100, true);
  (void)sc.take(kB, lv1, 400);
  (void)sc.take(kA, u1, 50);
  (void)sc.take(kA, u1, 500, true);
}

// a call that times two stretches and leaves where one of them fails
static int timed_call(EventPairs &first, EventPairs &second, hipStream_t s, bool on) {
  {
    TimedScope timed(first, s, on);
    if (timed.err) return 1;
    if (timed.close()) return 2;
  }
  TimedScope timed(second, s, on);
  if (timed.err) return 3;
  return 0;  // (closed by the scope)
}
static void events_scenario() {
  EventPairs br, ks;
  for (hipStream_t s : {kA, kB, kA}) (void)timed_call(br, ks, s, true);
  (void)timed_call(br, ks, kA, false);
  double ms = 0;
  uint64_t n = 0;
  if (br.drain(ms, &n)) (void)br.drain(ms, &n);  // (a second try, past the failure)
  (void)timed_call(br, ks, kB, true);
  (void)ks.drain(ms);
  OwnEvent e, f;
  (void)e.create(hipEventDisableTiming);
  (void)e.create(hipEventDisableTiming);  // (the first one goes)
  f = std::move(e);
  OwnEvent g(std::move(f));
}

static long every_failure_of(void (*scenario)(), const char *name) {
  reset();
  scenario();
  const long calls = g_fallible;
  EXPECT(calls > 0 && nothing_live());
  for (long k = 1; k <= calls; ++k) {
    const int bad0 = g_bad;
    reset(k);
    scenario();
    EXPECT(nothing_live());
    if (g_bad != bad0) fprintf(stderr, "  (%s, call %ld of %ld failing)\n", name, k, calls);
    g_dev.clear(), g_pin.clear(), g_heap.clear(), g_events.clear();
  }
  return calls;
}

// ---- the rules ---------------------------------------------------------------------------------------------------------
static void growth_rules() {
  reset();
  {
    DevBuf b;
    EXPECT(b.grow(100) == hipSuccess && b.p && b.cap == 125);
    const void *p0 = b.p;
    const size_t calls = g_log.size();
    EXPECT(b.grow(125) == hipSuccess && b.grow(1) == hipSuccess && b.grow(0) == hipSuccess);
    EXPECT(g_log.size() == calls && b.p == p0 && b.cap == 125);  // no call to the runtime while it fits
    EXPECT(b.grow(126) == hipSuccess && b.cap == 126 + 31);
    EXPECT(g_log.size() == calls + 2 && g_log[calls].op == 'F' && g_log[calls].p == p0 && g_log[calls + 1].op == 'M');  // free, then allocate
    EXPECT(b.grow(1001, true) == hipSuccess && b.cap == 1001);
    DevBuf e;
    EXPECT(e.grow(7, true) == hipSuccess && e.cap == 7);
    g_fail_at = g_fallible + 1;
    EXPECT(b.grow(5000) == hipErrorStandIn && b.p == nullptr && b.cap == 0);  // the old memory is gone, none came
    EXPECT(g_dev.size() == 1);
    EXPECT(b.grow(10) == hipSuccess && b.cap == 12);
  }
  EXPECT(nothing_live());
  reset();
  {  // a pinned arena: pinned memory, freed as such; no ordinary memory unless allowed
    PinBuf a;
    EXPECT(a.grow(100, false) && a.p && a.cap == 125 && !a.heap && g_pin.count(a.p));
    const size_t calls = g_log.size();
    EXPECT(a.grow(125, false) && g_log.size() == calls);
    g_no_pinned = true;
    EXPECT(!a.grow(200, false) && a.p == nullptr && a.cap == 0 && !a.heap);
    EXPECT(count_ops('Q') == 1 && count_ops('H') == 0 && nothing_live());
    EXPECT(a.grow(200, true) && a.p && a.cap == 250 && a.heap && g_heap.count(a.p) && g_pin.empty());
    g_no_pinned = false;
    const long pinned_tries = count_ops('P');
    EXPECT(a.grow(300, true) && a.heap && a.cap == 375);  // once ordinary, pinned memory is not tried again
    EXPECT(count_ops('P') == pinned_tries && count_ops('h') == 1 && count_ops('Q') == 1);
    g_fail_at = g_fallible + 1;
    EXPECT(!a.grow(4000, true) && a.p == nullptr && a.cap == 0 && !a.heap && nothing_live());
    PinBuf b;
    EXPECT(b.grow(10, true) && !b.heap);  // pinned memory first where it can be had
  }
  EXPECT(nothing_live() && count_ops('h') == 2 && count_ops('Q') == 2);
}

static void moved_from_frees_nothing() {
  reset();
  {
    DevBuf a;
    EXPECT(a.grow(10) == hipSuccess);
    void *p = a.p;
    DevBuf b(std::move(a));
    EXPECT(a.p == nullptr && a.cap == 0 && b.p == p && b.cap == 12);
    DevBuf c;
    EXPECT(c.grow(20) == hipSuccess);
    c = std::move(b);  // (c's own memory goes here)
    EXPECT(b.p == nullptr && c.p == p && count_ops('F') == 1);
    PinBuf q;
    EXPECT(q.grow(10, true));
    PinBuf r(std::move(q));
    EXPECT(q.p == nullptr && q.cap == 0 && r.p && r.cap == 12);
    OwnEvent e;
    EXPECT(e.create() == hipSuccess);
    OwnEvent f(std::move(e));
    EXPECT(e.e == nullptr && f.e != nullptr);
  }
  EXPECT(count_ops('F') == 2 && count_ops('Q') == 1 && count_ops('D') == 1 && nothing_live());
}

static void take_rules() {
  reset();
  Scratch sc;
  ScratchBuf lv1, u1;
  EXPECT(!sc.take(kA, lv1, 100) && lv1.p && lv1.cap == 125 && sc.owned && sc.owner == kA);
  EXPECT(count_ops('S') == 0);  // nobody owned it
  EXPECT(!sc.take(kA, u1, 64, true) && u1.cap == 64 && count_ops('S') == 0);  // on the owning stream: nothing
  g_log.clear();
  EXPECT(!sc.take(kB, lv1, 1000) && lv1.cap == 1250 && sc.owner == kB);
  EXPECT(count_ops('S') == 1 && g_log[0].op == 'S' && g_log[0].n == (size_t)kA);  // A, once, ahead of the free and the allocation
  EXPECT(first_of('F') > 0 && first_of('M') > first_of('F'));
  g_log.clear();
  EXPECT(!sc.take(kB, lv1, 10) && g_log.empty());  // fits, same stream: no call at all
  EXPECT(!sc.take(kA, lv1, 10) && g_log.size() == 1 && g_log[0].op == 'S' && g_log[0].n == (size_t)kB);  // fits: the claim alone
  g_log.clear();
  const void *p0 = u1.p;
  g_fail_at = g_fallible + 1;
  const HipErr r = sc.take(kB, u1, 5000);  // the synchronise fails: nothing is sized, the owner stays
  EXPECT(r && r.what && std::string(r.what) == "hipStreamSynchronize(ctx->scratch_owner)");
  EXPECT(g_log.size() == 1 && g_log[0].op == 'S' && u1.p == p0 && u1.cap == 64 && sc.owner == kA);
  g_fail_at = g_fallible + 1;
  const HipErr m = sc.take(kA, u1, 5000);  // the allocation fails: no text of its own, an empty buffer
  EXPECT(m && !m.what && u1.p == nullptr && u1.cap == 0);
}

static void event_rules() {
  // the scope records the second event exactly once, however it is left
  for (int how = 0; how < 4; ++how) {
    reset();
    EventPairs v;
    auto call = [&]() -> int {
      TimedScope timed(v, kA, true);
      if (timed.err) return -1;
      if (how == 0) return 7;                       // an error return
      if (how == 1) return timed.close() ? -1 : 0;  // closed by hand, then a return
      if (how == 2) return 0;                       // a plain return
      (void)timed.close();
      (void)timed.close();  // (closing again does nothing)
      return 0;
    };
    EXPECT(call() == (how == 0 ? 7 : 0));
    EXPECT(v.size() == 1 && count_ops('C') == 2 && count_ops('R') == 2);
    EXPECT(g_log[2].op == 'R' && g_log[3].op == 'R' && g_log[2].p != g_log[3].p && g_log[3].n == (size_t)kA);
    double ms = 0;
    EXPECT(!v.drain(ms) && ms == 1.0 + kA && v.size() == 0 && nothing_live());
  }
  {  // profiling off: no event at all
    reset();
    EventPairs v;
    {
      TimedScope timed(v, kA, false);
      EXPECT(!timed.err && !timed.close());
    }
    EXPECT(g_log.empty() && v.size() == 0);
  }
  for (int at = 0; at < 3; ++at) {  // a failed open (first create, second create, the record) adds nothing and keeps nothing
    reset();
    EventPairs v;
    g_fail_at = at + 1;
    {
      TimedScope timed(v, kA, true);
      const char *const texts[3] = {"hipEventCreate(&a)", "hipEventCreate(&b)", "hipEventRecord(a, s)"};
      EXPECT(timed.err && std::string(timed.err.what) == texts[at]);
    }
    EXPECT(v.size() == 0 && nothing_live() && count_ops('R') == (at == 2 ? 1 : 0));
  }
  // drain over n pairs failing at pair k (in the wait, or in the reading): pairs k.. stay, all live; the next drain takes them
  const int n = 5;
  for (int k = 0; k < n; ++k)
    for (int in_elapsed = 0; in_elapsed < 2; ++in_elapsed) {
      reset();
      EventPairs v;
      for (int i = 0; i < n; ++i) {
        TimedScope timed(v, i % 2 ? kA : kB, true);
        EXPECT(!timed.err);
      }
      EXPECT(v.size() == (size_t)n && g_events.size() == 2 * (size_t)n);
      double ms = 0;
      uint64_t cnt = 0;
      g_fail_at = g_fallible + 2 * k + 1 + in_elapsed;
      const HipErr r = v.drain(ms, &cnt);
      EXPECT(r && std::string(r.what) == (in_elapsed ? "hipEventElapsedTime(&t, p.first, p.second)" : "hipEventSynchronize(p.second)"));
      EXPECT(cnt == (uint64_t)k && v.size() == (size_t)(n - k) && g_events.size() == 2 * (size_t)(n - k));
      EXPECT(count_ops('D') == 2 * k);
      EXPECT(!v.drain(ms, &cnt) && cnt == (uint64_t)n && v.size() == 0 && nothing_live());
      EXPECT(ms == 3 * (1.0 + kB) + 2 * (1.0 + kA));
    }
  {  // what is never collected goes with its owner
    reset();
    {
      EventPairs v;
      for (int i = 0; i < 3; ++i) TimedScope timed(v, kA, true);
      EXPECT(g_events.size() == 6);
    }
    EXPECT(nothing_live() && count_ops('D') == 6);
  }
}

int main() {
  const long nb = every_failure_of(buffers_scenario, "buffers");
  const long ns = every_failure_of(scratch_scenario, "scratch");
  const long ne = every_failure_of(events_scenario, "events");
  growth_rules();
  moved_from_frees_nothing();
  take_rules();
  event_rules();
  EXPECT(nothing_live());
  if (g_bad) {
    fprintf(stderr, "%d expectation(s) failed\n", g_bad);
    return 1;
  }
  printf("resources ok: %ld + %ld + %ld failure points, growth, moves, take, timed scopes, drains\n", nb, ns, ne);
  return 0;
}
