// rs_tfhe packing key switch through the C++ mirror (include/rs_tfhe_hip.hpp) on the GPU: Engine::pack under a
// PackingKey made by the numpy client equals the integer model word for word, the packed results decrypt with s1 to the
// encrypted bits, and a second call reuses the loaded key.  The case (key, inputs, expected words, s1, bits) comes from
// tests/test_gpu_packing.py in one binary file: seed[32], count (u64), bodies, inputs, expected, s1 (u32), bits (u8).
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "rs_tfhe_hip.hpp"

using namespace rs_tfhe;

template <class T>
static bool read_into(std::ifstream &f, std::vector<T> &v, size_t count) {
  v.resize(count);
  return (bool)f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(count * sizeof(T)));
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: test_packing CASE\n");
    return 2;
  }
  const SecurityParams &P = SECURITY_128_BIT;
  std::ifstream f(argv[1], std::ios::binary);
  PackingKey pk;
  pk.params = P;
  uint64_t count = 0;
  std::vector<Torus> in, want, s1;
  std::vector<uint8_t> bits;
  f.read(reinterpret_cast<char *>(pk.mask_seed.data()), 32);
  f.read(reinterpret_cast<char *>(&count), 8);
  const size_t groups = (count + N - 1) / N;
  if (!f || !read_into(f, pk.bodies, (size_t)P.n * P.iks_t * N) || !read_into(f, in, count * (P.n + 1)) ||
      !read_into(f, want, groups * 2 * N) || !read_into(f, s1, N) || !read_into(f, bits, count)) {
    std::fprintf(stderr, "FAIL: short case file\n");
    return 1;
  }
  tfhe_hip_params cp{P.n, P.l, P.bgbit, P.basebit, P.iks_t};
  size_t words = 0;
  if (tfhe_hip_packing_key_words(&cp, &words) != TFHE_HIP_OK || words != pk.bodies.size()) {
    std::fprintf(stderr, "FAIL: sizes\n");
    return 1;
  }
  Engine &e = Engine::for_params(P, 0);
  const std::vector<Torus> out = e.pack(pk, in.data(), count);
  if (out != want || e.pack(pk, in.data(), count) != want) {
    std::fprintf(stderr, "FAIL: packed words differ from the model\n");
    return 1;
  }
  int bad = 0;
  for (size_t m = 0; m < count; ++m) {  // phase j = B[j] - (A (*) s1)[j]
    const Torus *a = &out[(m / N) * 2 * N], *b = a + N;
    const size_t j = m % N;
    Torus acc = b[j];
    for (size_t k = 0; k < N; ++k)
      if (s1[k]) acc += k <= j ? (Torus)0 - a[j - k] : a[j + N - k];
    if (((int32_t)acc >= 0) != (bits[m] != 0)) ++bad;
  }
  if (bad) {
    std::fprintf(stderr, "FAIL: %d of %llu packed results decrypt wrong\n", bad, (unsigned long long)count);
    return 1;
  }
  std::printf("ok: %llu results in %zu TRLWEs (%zu bytes), packing key %zu bytes\n", (unsigned long long)count, groups,
              out.size() * sizeof(Torus), pk.nbytes());
  return 0;
}
