// Packed encryption from C++ alone (include/rs_tfhe_hip.hpp: SecretKey::encrypt_packed_batch ->
// tfhe_hip_batch_encrypt_trlwe, SecretKey::expand_seeded_packed -> tfhe_hip_expand_seeded_trlwe): encrypt under a fixed
// generator key, expand the seeded form, decrypt, and print checksums for tests/test_gpu_packed_encrypt.py to compare
// with what the Python route got for the same inputs.
// usage: test_packed_encrypt n l bgbit basebit t alpha count first_group FILE
//   FILE: rng_key[32], mask_seed[32], key_lv1 [N] u32; plaintext m is +1/8 where m % 3 == 0, else -1/8
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "rs_tfhe_hip.hpp"

using namespace rs_tfhe;

static uint64_t checksum(const std::vector<Torus> &w) {  // sum of (2 x + 1) w[x] mod 2^64
  uint64_t sum = 0;
  for (size_t x = 0; x < w.size(); ++x) sum += (2 * (uint64_t)x + 1) * w[x];
  return sum;
}

int main(int argc, char **argv) {
  if (argc != 10) {
    std::fprintf(stderr, "usage: test_packed_encrypt n l bgbit basebit t alpha count first_group FILE\n");
    return 2;
  }
  const double alpha = std::atof(argv[6]);
  const SecurityParams P{0, std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]),
                         2.0e-5, alpha};
  const size_t count = (size_t)std::atoll(argv[7]), groups = (count + (size_t)N - 1) / (size_t)N;
  const uint64_t first_group = std::strtoull(argv[8], nullptr, 10);
  uint8_t K[32], S[32];
  SecretKey sk;
  sk.params = P;
  sk.key_lv0.assign((size_t)P.n, 0);
  sk.key_lv1.resize(N);
  std::ifstream f(argv[9], std::ios::binary);
  const bool ok = (bool)f.read(reinterpret_cast<char *>(K), 32) && (bool)f.read(reinterpret_cast<char *>(S), 32) &&
                  (bool)f.read(reinterpret_cast<char *>(sk.key_lv1.data()), (std::streamsize)(4 * sk.key_lv1.size()));
  if (!ok) {
    std::fprintf(stderr, "FAIL: short input file\n");
    return 1;
  }
  Engine &e = Engine::for_params(P, 0);
  std::vector<double> pts(count);
  for (size_t m = 0; m < count; ++m) pts[m] = m % 3 == 0 ? 0.125 : -0.125;
  std::vector<Torus> bodies;
  const std::vector<Torus> enc = sk.encrypt_packed_batch(e, pts, S, K, first_group, alpha, &bodies);
  if (enc.size() != groups * 2 * (size_t)N || bodies.size() != groups * (size_t)N) {
    std::fprintf(stderr, "FAIL: sizes\n");
    return 1;
  }
  // the same K and groups again give the same words; the OS-keyed call the same masks and other bodies
  const std::vector<Torus> os_keyed = sk.encrypt_packed_batch(e, pts, S, nullptr, first_group, alpha);
  bool same_masks = os_keyed.size() == enc.size(), same_bodies = true;
  for (size_t g = 0; same_masks && g < groups; ++g) {
    same_masks = std::memcmp(&os_keyed[g * 2 * N], &enc[g * 2 * N], 4 * (size_t)N) == 0;
    same_bodies = same_bodies && std::memcmp(&os_keyed[g * 2 * N + N], &enc[g * 2 * N + N], 4 * (size_t)N) == 0;
  }
  if (sk.encrypt_packed_batch(e, pts, S, K, first_group, alpha) != enc || !same_masks || same_bodies) {
    std::fprintf(stderr, "FAIL: the generator key and the mask seed do not determine the ciphertexts\n");
    return 1;
  }
  for (size_t g = 0; g < groups; ++g)
    if (std::memcmp(&bodies[g * N], &enc[g * 2 * N + N], 4 * (size_t)N) != 0) {
      std::fprintf(stderr, "FAIL: group %zu: the bodies are not the b half of the full form\n", g);
      return 1;
    }
  if (SecretKey::expand_seeded_packed(e, S, first_group, bodies) != enc) {
    std::fprintf(stderr, "FAIL: the expansion of the seeded form is not the full form\n");
    return 1;
  }
  const std::vector<Torus> bits = sk.decrypt_packed_batch(e, enc, count, TFHE_HIP_DECRYPT_BOOL);
  for (size_t m = 0; m < count; ++m)
    if (bits[m] != (Torus)(m % 3 == 0)) {
      std::fprintf(stderr, "FAIL: slot %zu decrypts wrong\n", m);
      return 1;
    }
  std::printf("enc_checksum %llu\nbodies_checksum %llu\nok: %zu values in %zu ciphertexts\n", (unsigned long long)checksum(enc),
              (unsigned long long)checksum(bodies), count, groups);
  return 0;
}
