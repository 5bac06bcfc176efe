// Public-key encryption and the asymmetric re-encryption key from C++ alone (include/rs_tfhe_hip.hpp:
// proxy_reenc::PublicKeyLv0::encrypt_batch -> tfhe_hip_batch_pk_encrypt, ProxyReencryptionKey::generate_asymmetric ->
// tfhe_hip_gen_reenc_key_asymmetric): encrypt and generate under a fixed generator key and print checksums for
// tests/test_gpu_pk_encrypt.py to compare with what the Python route got for the same inputs.
// usage: test_pk_encrypt n l bgbit basebit t alpha size count first_index FILE
//   FILE: rng_key[32], key_from [n] u32, encryptions [size][n+1] u32; plaintext m is +1/8 where m % 3 == 0, else -1/8
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
static std::vector<Torus> flatten(const std::vector<Ciphertext> &cts) {
  std::vector<Torus> f;
  for (const Ciphertext &c : cts) f.insert(f.end(), c.p.begin(), c.p.end());
  return f;
}

int main(int argc, char **argv) {
  if (argc != 11) {
    std::fprintf(stderr, "usage: test_pk_encrypt n l bgbit basebit t alpha size count first_index FILE\n");
    return 2;
  }
  const double alpha = std::atof(argv[6]);
  const SecurityParams P{0, std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]),
                         alpha, 2.0e-8};
  const size_t size = (size_t)std::atoll(argv[7]), count = (size_t)std::atoll(argv[8]), w = (size_t)P.n + 1;
  const uint64_t first_index = std::strtoull(argv[9], nullptr, 10);
  uint8_t K[32];
  std::vector<Torus> key_from((size_t)P.n);
  proxy_reenc::PublicKeyLv0 pk;
  pk.params = P;
  pk.encryptions.assign(size, Ciphertext(P.n));
  std::ifstream f(argv[10], std::ios::binary);
  bool ok = (bool)f.read(reinterpret_cast<char *>(K), 32) &&
            (bool)f.read(reinterpret_cast<char *>(key_from.data()), (std::streamsize)(4 * key_from.size()));
  for (size_t i = 0; ok && i < size; ++i) ok = (bool)f.read(reinterpret_cast<char *>(pk.encryptions[i].p.data()), (std::streamsize)(4 * w));
  if (!ok) {
    std::fprintf(stderr, "FAIL: short input file\n");
    return 1;
  }
  Engine &e = Engine::for_params(P, 0);
  std::vector<double> pts(count);
  for (size_t m = 0; m < count; ++m) pts[m] = m % 3 == 0 ? 0.125 : -0.125;
  const std::vector<Torus> enc = flatten(pk.encrypt_batch(e, pts, alpha, K, first_index));
  // the same K and rows again give the same words; the OS-keyed call others
  if (flatten(pk.encrypt_batch(e, pts, alpha, K, first_index)) != enc || flatten(pk.encrypt_batch(e, pts, alpha)) == enc) {
    std::fprintf(stderr, "FAIL: the generator key does not determine the ciphertexts\n");
    return 1;
  }
  const proxy_reenc::ProxyReencryptionKey rk = proxy_reenc::ProxyReencryptionKey::generate_asymmetric(e, key_from, pk, K);
  const proxy_reenc::ProxyReencryptionKey quiet = proxy_reenc::ProxyReencryptionKey::generate_asymmetric(e, key_from, pk, K, -1, false);
  if (rk.key_encryptions.size() != (size_t)P.n * P.iks_t * P.base() * w || !quiet.key_encryptions.empty()) {
    std::fprintf(stderr, "FAIL: sizes\n");
    return 1;
  }
  // both handles re-encrypt to the same words: the one that downloaded its key and the one that did not
  std::vector<Ciphertext> cts(count, Ciphertext(P.n));
  for (size_t m = 0; m < count; ++m) std::memcpy(cts[m].p.data(), &enc[m * w], 4 * w);
  const std::vector<Torus> re = flatten(rk.reencrypt(cts));
  if (flatten(quiet.reencrypt(cts)) != re) {
    std::fprintf(stderr, "FAIL: key_out = NULL left another key on the handle\n");
    return 1;
  }
  std::printf("enc_checksum %llu\nkey_checksum %llu\nreenc_checksum %llu\nok: %zu ciphertexts, a key of %zu bytes\n",
              (unsigned long long)checksum(enc), (unsigned long long)checksum(rk.key_encryptions),
              (unsigned long long)checksum(re), count, rk.key_encryptions.size() * sizeof(Torus));
  return 0;
}
