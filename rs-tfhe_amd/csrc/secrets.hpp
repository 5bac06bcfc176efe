// secrets.hpp -- the one path by which a call's secrets reach the device, and by which secrets, plaintexts and decrypted
// words leave the library's buffers again (host code only).  tests/cpp/test_secret_stage.cpp runs this file as it is,
// over host memory: the including file supplies the HIP runtime's names, std::string and resources.hpp (DevBuf, Staging)
// ahead of it and defines fail, ensure and claim_scratch; the context is opaque here.  Shared between the library's
// translation units (internal.hpp): nothing is in an anonymous namespace.
#pragma once

struct tfhe_hip_ctx;

int fail(tfhe_hip_ctx *ctx, int code, const std::string &msg);
int ensure(tfhe_hip_ctx *ctx, DevBuf &b, size_t bytes);
int claim_scratch(tfhe_hip_ctx *ctx, hipStream_t s);

// zero host memory (4-byte aligned) in stores the compiler may not elide
inline void wipe_host(void *p, size_t bytes) {
  for (size_t i = 0; i < bytes / 4; ++i) ((volatile uint32_t *)p)[i] = 0;
  for (size_t i = bytes & ~(size_t)3; i < bytes; ++i) ((volatile unsigned char *)p)[i] = 0;
}

// The secrets of one call in `buf` (the context's sym_sec) on stream `s`.  Construction claims the scratch; put(), or
// writing at host(), gathers the pieces into one image, held in the guard and zero at first; land() copies it; dev()
// points at a piece.  Leaving scope, whichever way, queues the zeroing of the whole buffer behind what the call queued
// on `s`, and with `drain` (the key generators, on the context's stream) synchronises `s` behind it.
constexpr size_t kSecretImageMax = 12 * 1024;  // (the largest: K and two keys of n <= 1279 words)
class SecretStage {
 public:
  SecretStage(tfhe_hip_ctx *ctx, DevBuf &buf, hipStream_t s, size_t image_bytes, bool drain = false)
      : ctx_(ctx), buf_(buf), s_(s), drain_(drain), bytes_(image_bytes <= kSecretImageMax ? image_bytes : 0) {
    rc_ = bytes_ == image_bytes ? claim_scratch(ctx, s) : fail(ctx, TFHE_HIP_EINVAL, "secret image too large");
    memset(img_, 0, (bytes_ + 3) & ~(size_t)3);
  }
  SecretStage(const SecretStage &) = delete;  // (nor assignable: buf_ is a reference)
  ~SecretStage() {
    wipe_host(img_, bytes_);  // (a call that left before land())
    (void)wipe();
  }

  void *host(size_t at) { return (unsigned char *)img_ + at; }
  void put(const void *src, size_t bytes, size_t at) { if (at + bytes <= bytes_) memcpy(host(at), src, bytes); }
  // One copy to the head of the buffer, grown to `device_bytes` where that is more (slots a kernel fills), and one
  // synchronise: the image is wiped whether or not the copy succeeded.  `what` opens the text of a HIP failure.
  int land(const char *what, size_t device_bytes = 0) {
    int rc = rc_;
    if (rc == TFHE_HIP_OK) rc = ensure(ctx_, buf_, device_bytes > bytes_ ? device_bytes : bytes_);
    if (rc == TFHE_HIP_OK) {
      hipError_t e = hipMemcpyAsync(buf_.p, img_, bytes_, hipMemcpyHostToDevice, s_);
      if (e == hipSuccess) e = hipStreamSynchronize(s_);
      if (e != hipSuccess) rc = fail(ctx_, TFHE_HIP_EHIP, std::string(what) + hipGetErrorString(e));
    }
    wipe_host(img_, bytes_);
    bytes_ = 0;
    return rc;
  }
  template <class T = const uint32_t>
  T *dev(size_t at) const { return (T *)((unsigned char *)buf_.p + at); }
  int finish(int rc) {  // the wipe, now: rc, or where that is OK the wipe's own failure
    const hipError_t e = wipe();
    if (rc != TFHE_HIP_OK || e == hipSuccess) return rc;
    return fail(ctx_, TFHE_HIP_EHIP, std::string("zeroing the staged secrets: ") + hipGetErrorString(e));
  }

 private:
  hipError_t wipe() {  // once
    if (wiped_) return hipSuccess;
    wiped_ = true;
    hipError_t e = buf_.p ? hipMemsetAsync(buf_.p, 0, buf_.cap, s_) : hipSuccess;
    const hipError_t es = drain_ ? hipStreamSynchronize(s_) : hipSuccess;
    return e != hipSuccess ? e : es;
  }
  tfhe_hip_ctx *ctx_;
  DevBuf &buf_;
  hipStream_t s_;
  bool drain_, wiped_ = false;
  size_t bytes_;  // of the image; 0 once it has landed
  int rc_;
  uint32_t img_[kSecretImageMax / 4];
};

// A host form's epilogue on the context's stream `s`: the first `bytes` of each slot -- what the call staged there --
// are zeroed on the device, `s` is synchronised once, and the same bytes of the slot's pinned arena (pool members stage
// large operands through it) are wiped.  Best effort: the call's status is its own.
struct ScrubSlot {
  Staging *slot;
  size_t bytes;
};
inline void scrub(hipStream_t s, std::initializer_list<ScrubSlot> slots) {
  for (const ScrubSlot &x : slots)
    if (x.slot->dev.p) (void)hipMemsetAsync(x.slot->dev.p, 0, x.bytes < x.slot->dev.cap ? x.bytes : x.slot->dev.cap, s);
  (void)hipStreamSynchronize(s);
  for (const ScrubSlot &x : slots)
    if (x.slot->pin.p) wipe_host(x.slot->pin.p, x.bytes < x.slot->pin.cap ? x.bytes : x.slot->pin.cap);
}
