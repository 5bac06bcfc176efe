// SecretStage and scrub (rs-tfhe_amd/csrc/secrets.hpp) as the library compiles them, over host memory: the HIP names
// the header uses are stand-ins here (a copy is memcpy, a memset is memset, a synchronise is an entry in a log), each
// with a switch that makes it fail, and so are fail, ensure and claim_scratch.  Built and run by
// tests/test_secrets_host.py, once more under AddressSanitizer + UBSan.
//
// For every way a secret-staging call can go -- all well, the buffer cannot be had, the copy is refused, the copy is
// queued but the synchronise fails, the caller's launch fails -- and for both ways of leaving (finish(), or a plain
// return):  the host image is all zero after land();  after the guard has left scope every byte of the device buffer
// up to its capacity is zero, stale bytes of an earlier call included;  the memset was issued once, on the guard's
// stream, after the last launch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tfhe_hip.h"

typedef int hipStream_t;  // a stream is a number here
enum hipError_t { hipSuccess = 0, hipErrorStandIn = 1 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };

struct Event {
  char op;  // 'k' claim_scratch, 'e' ensure, 'c' copy, 's' synchronise, 'm' memset, 'l' the caller's launch
  hipStream_t stream;
  const void *p;
  size_t bytes;
};
static std::vector<Event> g_log;
static bool g_fail_claim, g_fail_ensure, g_fail_copy, g_fail_sync, g_fail_memset;
static int g_bad = 0;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      ++g_bad;                                                    \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
    }                                                             \
  } while (0)

static const char *hipGetErrorString(hipError_t) { return "stand-in failure"; }
static hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t s) {
  g_log.push_back({'c', s, dst, bytes});
  if (g_fail_copy) return hipErrorStandIn;
  memcpy(dst, src, bytes);
  return hipSuccess;
}
static hipError_t hipMemsetAsync(void *dst, int v, size_t bytes, hipStream_t s) {
  g_log.push_back({'m', s, dst, bytes});
  if (g_fail_memset) return hipErrorStandIn;
  memset(dst, v, bytes);
  return hipSuccess;
}
static hipError_t hipStreamSynchronize(hipStream_t s) {
  g_log.push_back({'s', s, nullptr, 0});
  return g_fail_sync ? hipErrorStandIn : hipSuccess;
}

// what resources.hpp (DevBuf, Staging) names beside those: the buffers here are the test's own memory, which it frees
// itself, so a free does nothing and nothing is ever allocated or timed
typedef void *hipEvent_t;
enum { hipHostMallocDefault = 0, hipEventDefault = 0 };
static hipError_t hipGetLastError() { return hipSuccess; }
static hipError_t hipMalloc(void **, size_t) { return hipErrorStandIn; }
static hipError_t hipFree(void *) { return hipSuccess; }
static hipError_t hipHostMalloc(void **, size_t, unsigned) { return hipErrorStandIn; }
static hipError_t hipHostFree(void *) { return hipSuccess; }
static hipError_t hipEventCreateWithFlags(hipEvent_t *, unsigned) { return hipErrorStandIn; }
static hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
static hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipErrorStandIn; }
static hipError_t hipEventSynchronize(hipEvent_t) { return hipErrorStandIn; }
static hipError_t hipEventElapsedTime(float *, hipEvent_t, hipEvent_t) { return hipErrorStandIn; }

#include "../../rs-tfhe_amd/csrc/resources.hpp"
#include "../../rs-tfhe_amd/csrc/secrets.hpp"

struct tfhe_hip_ctx {
  std::string err;
};

// (the three functions secrets.hpp declares: the library defines them in tfhe_hip.hip)
int fail(tfhe_hip_ctx *ctx, int code, const std::string &msg) {
  ctx->err = msg;
  return code;
}
// the library's growth rule; a new buffer arrives full of 0xA5
int ensure(tfhe_hip_ctx *ctx, DevBuf &b, size_t bytes) {
  g_log.push_back({'e', 0, b.p, bytes});
  if (bytes <= b.cap) return TFHE_HIP_OK;
  if (g_fail_ensure) return fail(ctx, TFHE_HIP_ENOMEM, "no memory");  // (the old buffer stays, as when hipFree fails)
  free(b.p);
  b.cap = bytes + bytes / 4;
  b.p = malloc(b.cap);
  memset(b.p, 0xA5, b.cap);
  return TFHE_HIP_OK;
}
int claim_scratch(tfhe_hip_ctx *ctx, hipStream_t s) {
  g_log.push_back({'k', s, nullptr, 0});
  return g_fail_claim ? fail(ctx, TFHE_HIP_EHIP, "claim") : TFHE_HIP_OK;
}

static bool all_bytes(const void *p, size_t bytes, unsigned char v) {
  for (size_t i = 0; i < bytes; ++i)
    if (((const unsigned char *)p)[i] != v) return false;
  return true;
}
static void reset() {
  g_log.clear();
  g_fail_claim = g_fail_ensure = g_fail_copy = g_fail_sync = g_fail_memset = false;
}
static long count_ops(char op) {
  long n = 0;
  for (const Event &e : g_log) n += e.op == op;
  return n;
}
static long last_of(char op) {
  long at = -1;
  for (size_t i = 0; i < g_log.size(); ++i)
    if (g_log[i].op == op) at = (long)i;
  return at;
}

enum Path { ALL_WELL, CLAIM_FAILS, ENSURE_FAILS, COPY_FAILS, SYNC_FAILS, LAUNCH_FAILS };
constexpr hipStream_t kStream = 7;
constexpr size_t kImage = 42, kDevice = 100;  // an image that is no multiple of 4, and a slot behind it a kernel fills

// One call's life.  `finish`: the call leaves through finish(rc), else by a plain return.  `drain`: the guard of a key
// generator.  The device buffer starts as an earlier, smaller call left it: 16 stale bytes.
static void guard_path(Path path, bool finish, bool drain) {
  reset();
  tfhe_hip_ctx ctx;
  DevBuf buf;
  buf.cap = 16;
  buf.p = malloc(buf.cap);
  memset(buf.p, 0xA5, buf.cap);
  unsigned char secret[kImage];
  for (size_t i = 0; i < kImage; ++i) secret[i] = (unsigned char)(i + 1);
  g_fail_claim = path == CLAIM_FAILS;
  g_fail_ensure = path == ENSURE_FAILS;
  g_fail_copy = path == COPY_FAILS;
  g_fail_sync = path == SYNC_FAILS;
  int want = TFHE_HIP_OK, ret = TFHE_HIP_OK;
  {
    SecretStage sec(&ctx, buf, kStream, kImage, drain);
    sec.put(secret, 32, 0);
    sec.put(secret + 32, kImage - 32, 32);
    EXPECT(memcmp(sec.host(0), secret, kImage) == 0);
    int rc = sec.land("stand-in: ", kDevice);
    EXPECT(all_bytes(sec.host(0), (kImage + 3) / 4 * 4, 0));  // the host image, whichever way the copy went
    g_fail_sync = false;  // (what failed was the synchronise behind the copy)
    want = path == ALL_WELL || path == LAUNCH_FAILS ? TFHE_HIP_OK : path == ENSURE_FAILS ? TFHE_HIP_ENOMEM : TFHE_HIP_EHIP;
    EXPECT(rc == want);
    if (path == COPY_FAILS || path == SYNC_FAILS) EXPECT(ctx.err == "stand-in: stand-in failure");
    if (path == CLAIM_FAILS) EXPECT(count_ops('e') == 0 && count_ops('c') == 0);
    if (path == ENSURE_FAILS) EXPECT(count_ops('c') == 0);
    if (path == COPY_FAILS) EXPECT(count_ops('s') == 0);
    if (rc == TFHE_HIP_OK) {
      EXPECT(count_ops('c') == 1 && count_ops('s') == 1 && buf.cap >= kDevice);
      EXPECT(memcmp(buf.p, secret, kImage) == 0 && sec.dev<unsigned char>(32) == (unsigned char *)buf.p + 32);
      memset(sec.dev<unsigned char>(kImage), 0x5A, buf.cap - kImage);  // the "kernel" fills its slot, to the end
      g_log.push_back({'l', kStream, nullptr, 0});
      if (path == LAUNCH_FAILS) rc = want = TFHE_HIP_EINVAL;
    }
    if (path == SYNC_FAILS) EXPECT(memcmp(buf.p, secret, kImage) == 0);  // the copy was queued: the secrets are there
    ret = finish ? sec.finish(rc) : rc;
    if (finish) EXPECT(count_ops('m') == 1);
  }
  EXPECT(ret == want);
  EXPECT(buf.cap >= 16 && all_bytes(buf.p, buf.cap, 0));
  const long m = last_of('m');
  EXPECT(count_ops('m') == 1 && m >= 0);
  if (m >= 0) {
    EXPECT(g_log[m].stream == kStream && g_log[m].p == buf.p && g_log[m].bytes == buf.cap);
    EXPECT(m > last_of('l') && m > last_of('c'));
    EXPECT(drain ? (m + 2 == (long)g_log.size() && g_log[m + 1].op == 's' && g_log[m + 1].stream == kStream)
                 : m + 1 == (long)g_log.size());
  }
  free(buf.p);
}

// the wipe's own failure is the call's status only where the call would otherwise return OK
static void finish_reports_the_wipe() {
  for (int rc_in : {TFHE_HIP_OK, TFHE_HIP_EINVAL}) {
    reset();
    tfhe_hip_ctx ctx;
    DevBuf buf;
    uint32_t word = 5;
    {
      SecretStage sec(&ctx, buf, kStream, 4);
      sec.put(&word, 4, 0);
      EXPECT(sec.land("stand-in: ") == TFHE_HIP_OK);
      g_fail_memset = true;
      const int rc = sec.finish(rc_in);
      EXPECT(rc == (rc_in == TFHE_HIP_OK ? TFHE_HIP_EHIP : rc_in));
      EXPECT((rc_in == TFHE_HIP_OK) == (ctx.err == "zeroing the staged secrets: stand-in failure"));
    }
    EXPECT(count_ops('m') == 1);  // (not tried again by the destructor)
    free(buf.p);
  }
  // a guard that never staged anything has nothing to zero
  reset();
  tfhe_hip_ctx ctx;
  DevBuf buf;
  { SecretStage sec(&ctx, buf, kStream, 8); }
  EXPECT(count_ops('m') == 0 && count_ops('k') == 1);
  // an image the guard has no room for is refused, and nothing is written or copied
  reset();
  {
    static unsigned char big[kSecretImageMax + 1];
    SecretStage sec(&ctx, buf, kStream, sizeof(big));
    sec.put(big, sizeof(big), 0);
    EXPECT(sec.land("stand-in: ") == TFHE_HIP_EINVAL && ctx.err == "secret image too large");
  }
  EXPECT(g_log.empty() && !buf.p);
}

struct Slot {
  Staging s;
  unsigned char *dev_mem = nullptr, *pin_mem = nullptr;
  size_t dev_alloc = 0, pin_alloc = 0;
  // buffers of `dev_cap` / `pin_cap` bytes (0: none), each with 16 bytes behind it that are not the slot's
  Slot(size_t dev_cap, size_t pin_cap) : dev_alloc(dev_cap + 16), pin_alloc(pin_cap + 16) {
    if (dev_cap) {
      s.dev.p = dev_mem = (unsigned char *)malloc(dev_alloc);
      s.dev.cap = dev_cap;
      memset(dev_mem, 0xA5, dev_alloc);
    }
    if (pin_cap) {
      s.pin.p = pin_mem = (unsigned char *)malloc(pin_alloc);
      s.pin.cap = pin_cap;
      memset(pin_mem, 0xA5, pin_alloc);
    }
  }
  ~Slot() {
    free(dev_mem);
    free(pin_mem);
  }
  // min(bytes, cap) zero bytes, 0xA5 behind them
  void expect(size_t bytes) const {
    if (dev_mem) {
      const size_t z = bytes < s.dev.cap ? bytes : s.dev.cap;
      EXPECT(all_bytes(dev_mem, z, 0) && all_bytes(dev_mem + z, dev_alloc - z, 0xA5));
    }
    if (pin_mem) {
      const size_t z = bytes < s.pin.cap ? bytes : s.pin.cap;
      EXPECT(all_bytes(pin_mem, z, 0) && all_bytes(pin_mem + z, pin_alloc - z, 0xA5));
    }
  }
};

static void scrub_cases() {
  {
    reset();
    Slot within(64, 64), past_dev(64, 128), past_both(64, 32), odd(32, 32), no_pin(64, 0), no_dev(0, 64), nothing(0, 0);
    scrub(kStream, {{&within.s, 48}, {&past_dev.s, 100}, {&past_both.s, 1000}, {&odd.s, 13}, {&no_pin.s, 48}, {&no_dev.s, 48},
                    {&nothing.s, 48}});
    within.expect(48);
    past_dev.expect(100);
    past_both.expect(1000);
    odd.expect(13);
    no_pin.expect(48);
    no_dev.expect(48);
    EXPECT(count_ops('m') == 5 && count_ops('s') == 1 && last_of('s') > last_of('m'));
    for (const Event &e : g_log) EXPECT(e.stream == kStream);
  }
  {  // a refused memset: still one synchronise, and the arena is wiped all the same
    reset();
    g_fail_memset = true;
    Slot a(64, 64), b(64, 64);
    scrub(kStream, {{&a.s, 40}, {&b.s, 64}});
    EXPECT(count_ops('m') == 2 && count_ops('s') == 1 && last_of('s') > last_of('m'));
    EXPECT(all_bytes(a.dev_mem, 64, 0xA5) && all_bytes(a.pin_mem, 40, 0) && all_bytes(a.pin_mem + 40, 24 + 16, 0xA5));
    EXPECT(all_bytes(b.pin_mem, 64, 0) && all_bytes(b.pin_mem + 64, 16, 0xA5));
  }
  {  // no slot at all: the stream is drained all the same
    reset();
    scrub(kStream, {});
    EXPECT(count_ops('s') == 1 && g_log.size() == 1);
  }
}

int main() {
  for (Path path : {ALL_WELL, CLAIM_FAILS, ENSURE_FAILS, COPY_FAILS, SYNC_FAILS, LAUNCH_FAILS})
    for (int finish = 0; finish < 2; ++finish)
      for (int drain = 0; drain < 2; ++drain) guard_path(path, finish != 0, drain != 0);
  finish_reports_the_wipe();
  scrub_cases();
  if (g_bad) {
    fprintf(stderr, "%d expectation(s) failed\n", g_bad);
    return 1;
  }
  printf("secret stage ok: 24 guard paths, the wipe's status, 3 scrub cases\n");
  return 0;
}
