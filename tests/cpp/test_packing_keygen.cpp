// The packing key made from C++ alone (include/rs_tfhe_hip.hpp: PackingKey::generate -> tfhe_hip_gen_packing_key), no
// Python-made key file: generate under a fixed generator key, Engine::pack trivial ciphertexts of bits under it, decode
// them with s1, and print the mask seed and a checksum of the bodies for tests/test_gpu_packing_keygen.py to compare
// with what the Python route got for the same secret key.
// usage: test_packing_keygen n l bgbit basebit t alpha KEYFILE   (KEYFILE: rng_key[32], key_lv0 [n] u32, key_lv1 [N] u32)
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "rs_tfhe_hip.hpp"

using namespace rs_tfhe;

int main(int argc, char **argv) {
  if (argc != 8) {
    std::fprintf(stderr, "usage: test_packing_keygen n l bgbit basebit t alpha KEYFILE\n");
    return 2;
  }
  const double alpha = std::atof(argv[6]);
  const SecurityParams P{0, std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]),
                         2.0e-5, alpha};
  SecretKey sk;
  sk.params = P;
  sk.key_lv0.resize((size_t)P.n);
  sk.key_lv1.resize(N);
  uint8_t K[32];
  std::ifstream f(argv[7], std::ios::binary);
  if (!f.read(reinterpret_cast<char *>(K), 32) || !f.read(reinterpret_cast<char *>(sk.key_lv0.data()), (std::streamsize)(4 * sk.key_lv0.size())) ||
      !f.read(reinterpret_cast<char *>(sk.key_lv1.data()), (std::streamsize)(4 * N))) {
    std::fprintf(stderr, "FAIL: short key file\n");
    return 1;
  }
  const PackingKey pk = PackingKey::generate(sk, 0, K);  // alpha: the set's alpha_lv1
  if (!pk.matches(P)) {
    std::fprintf(stderr, "FAIL: sizes\n");
    return 1;
  }
  // the same K again gives the same key; the OS-keyed call another seed
  const PackingKey again = PackingKey::generate(sk, 0, K, alpha), fresh = PackingKey::generate(sk);
  if (again.mask_seed != pk.mask_seed || again.bodies != pk.bodies || fresh.mask_seed == pk.mask_seed) {
    std::fprintf(stderr, "FAIL: the generator key does not determine the key\n");
    return 1;
  }
  // trivial ciphertexts (mask 0, body +-1/8): 1500 results, two groups
  const size_t count = 1500, w = (size_t)P.n + 1;
  std::vector<Torus> in(count * w, 0u);
  for (size_t m = 0; m < count; ++m) in[m * w + (size_t)P.n] = f64_to_torus(m % 3 == 0 ? 0.125 : -0.125);
  Engine &e = Engine::for_params(P, 0);
  const std::vector<Torus> out = e.pack(pk, in.data(), count);
  int bad = 0;
  for (size_t m = 0; m < count; ++m) {  // phase j = B[j] - (A (*) s1)[j]
    const Torus *a = &out[(m / N) * 2 * N], *b = a + N;
    const size_t j = m % N;
    Torus acc = b[j];
    for (size_t k = 0; k < N; ++k)
      if (sk.key_lv1[k]) acc += k <= j ? (Torus)0 - a[j - k] : a[j + N - k];
    if (((int32_t)acc >= 0) != (m % 3 == 0)) ++bad;
  }
  if (bad) {
    std::fprintf(stderr, "FAIL: %d of %zu packed results decode wrong\n", bad, count);
    return 1;
  }
  uint64_t sum = 0;  // sum of (2 x + 1) w[x] mod 2^64
  for (size_t x = 0; x < pk.bodies.size(); ++x) sum += (2 * (uint64_t)x + 1) * pk.bodies[x];
  std::printf("seed ");
  for (uint8_t b : pk.mask_seed) std::printf("%02x", b);
  std::printf("\nchecksum %llu\nok: %zu results decoded under a key of %zu bytes\n", (unsigned long long)sum, count, pk.nbytes());
  return 0;
}
