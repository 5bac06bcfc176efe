// decrypt_decode.hpp -- what a phase decrypts to, in one function for the device and the host (include/tfhe_hip.h,
// "decryption").  No HIP header is needed: tests/cpp/test_decrypt_decode.cpp compiles it with a plain C++ compiler and
// holds it to rs-tfhe_amd/client.py, which stays the definition.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TFHE_DECODE_FN __host__ __device__ __forceinline__
#else
#define TFHE_DECODE_FN inline
#endif

// the values of TFHE_HIP_DECRYPT_* (include/tfhe_hip.h; decrypt.hpp asserts that they agree)
constexpr int kDecryptPhase = 0, kDecryptBool = 1, kDecryptMessage = 2;

// PHASE: the phase.  BOOL (tlwe.rs:60-68): the phase read as i32 is non-negative.  MESSAGE (tlwe.rs:111-126):
// ((phase / 2^32) / scale + 0.5) as integer % m with scale = 1 / (2m), all in f64 and in that order: 2m and phase / 2^32
// are exact, both divisions are correctly rounded and a division followed by an add cannot contract, so the device,
// the host and numpy agree on every word.  2 <= m <= 65,536: the value before the truncation is below 2^18.
TFHE_DECODE_FN uint32_t decrypt_decode(uint32_t phase, int mode, uint32_t modulus) {
  if (mode == kDecryptBool) return (int32_t)phase >= 0 ? 1u : 0u;
  if (mode == kDecryptMessage) {
    const double scale = 1.0 / (2.0 * (double)modulus);
    const double v = ((double)phase / 4294967296.0) / scale + 0.5;
    return (uint32_t)((int64_t)v % (int64_t)modulus);
  }
  return phase;
}
