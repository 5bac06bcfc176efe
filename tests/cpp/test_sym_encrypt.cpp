// Symmetric encryption from C++ alone (include/rs_tfhe_hip.hpp: SecretKey::encrypt_batch -> tfhe_hip_batch_encrypt,
// proxy_reenc::PublicKeyLv0::generate -> tfhe_hip_gen_public_key, ProxyReencryptionKey::generate_symmetric ->
// tfhe_hip_gen_reenc_key_symmetric): encrypt and generate under a fixed generator key and print checksums for
// tests/test_gpu_sym_encrypt.py to compare with what the Python route got for the same inputs.
// usage: test_sym_encrypt n l bgbit basebit t alpha size count first_index FILE
//   FILE: rng_key[32], mask_seed[32], key_from [n] u32, key_to [n] u32; plaintext m is +1/8 where m % 3 == 0, else -1/8
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
    std::fprintf(stderr, "usage: test_sym_encrypt n l bgbit basebit t alpha size count first_index FILE\n");
    return 2;
  }
  const double alpha = std::atof(argv[6]);
  const SecurityParams P{0, std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]),
                         alpha, 2.0e-8};
  const size_t size = (size_t)std::atoll(argv[7]), count = (size_t)std::atoll(argv[8]), w = (size_t)P.n + 1;
  const uint64_t first_index = std::strtoull(argv[9], nullptr, 10);
  uint8_t K[32], S[32];
  SecretKey alice, bob;
  alice.params = bob.params = P;
  alice.key_lv0.resize((size_t)P.n);
  bob.key_lv0.resize((size_t)P.n);
  std::ifstream f(argv[10], std::ios::binary);
  const bool ok = (bool)f.read(reinterpret_cast<char *>(K), 32) && (bool)f.read(reinterpret_cast<char *>(S), 32) &&
                  (bool)f.read(reinterpret_cast<char *>(alice.key_lv0.data()), (std::streamsize)(4 * alice.key_lv0.size())) &&
                  (bool)f.read(reinterpret_cast<char *>(bob.key_lv0.data()), (std::streamsize)(4 * bob.key_lv0.size()));
  if (!ok) {
    std::fprintf(stderr, "FAIL: short input file\n");
    return 1;
  }
  Engine &e = Engine::for_params(P, 0);
  std::vector<double> pts(count);
  for (size_t m = 0; m < count; ++m) pts[m] = m % 3 == 0 ? 0.125 : -0.125;
  std::vector<Torus> bodies;
  const std::vector<Ciphertext> cts = alice.encrypt_batch(e, pts, S, K, first_index, alpha, &bodies);
  const std::vector<Torus> enc = flatten(cts);
  // the same K and rows again give the same words; the OS-keyed call the same masks and other bodies
  const std::vector<Torus> os_keyed = flatten(alice.encrypt_batch(e, pts, S, nullptr, first_index, alpha));
  bool same_masks = os_keyed.size() == enc.size(), same_bodies = true;
  for (size_t m = 0; same_masks && m < count; ++m) {
    same_masks = std::memcmp(&os_keyed[m * w], &enc[m * w], 4 * (w - 1)) == 0;
    same_bodies = same_bodies && os_keyed[m * w + w - 1] == enc[m * w + w - 1];
  }
  if (flatten(alice.encrypt_batch(e, pts, S, K, first_index, alpha)) != enc || !same_masks || same_bodies) {
    std::fprintf(stderr, "FAIL: the generator key and the mask seed do not determine the ciphertexts\n");
    return 1;
  }
  for (size_t m = 0; m < count; ++m)
    if (bodies.size() != count || bodies[m] != enc[m * w + w - 1] || tlwe::decrypt_bool(cts[m], alice.key_lv0) != (m % 3 == 0)) {
      std::fprintf(stderr, "FAIL: ciphertext %zu: bodies or decryption\n", m);
      return 1;
    }
  const proxy_reenc::PublicKeyLv0 pk = proxy_reenc::PublicKeyLv0::generate(e, bob, K, size, alpha);
  if (pk.encryptions.size() != size) {
    std::fprintf(stderr, "FAIL: public key size\n");
    return 1;
  }
  for (const Ciphertext &c : pk.encryptions) {  // encryptions of zero: |phase| within 6 alpha
    const double ph = (double)(int32_t)(c.b() - tlwe::inner_product(c, bob.key_lv0)) / 4294967296.0;
    if (!(ph < 6 * alpha && ph > -6 * alpha)) {
      std::fprintf(stderr, "FAIL: a public key row is no encryption of zero\n");
      return 1;
    }
  }
  const proxy_reenc::ProxyReencryptionKey rk = proxy_reenc::ProxyReencryptionKey::generate_symmetric(e, alice.key_lv0, bob, K, alpha);
  const proxy_reenc::ProxyReencryptionKey quiet =
      proxy_reenc::ProxyReencryptionKey::generate_symmetric(e, alice.key_lv0, bob, K, alpha, false);
  if (rk.key_encryptions.size() != (size_t)P.n * P.iks_t * P.base() * w || !quiet.key_encryptions.empty()) {
    std::fprintf(stderr, "FAIL: sizes\n");
    return 1;
  }
  // both handles re-encrypt to the same words: the one that downloaded its key and the one that did not
  const std::vector<Torus> re = flatten(rk.reencrypt(cts));
  if (flatten(quiet.reencrypt(cts)) != re) {
    std::fprintf(stderr, "FAIL: key_out = NULL left another key on the handle\n");
    return 1;
  }
  std::printf("enc_checksum %llu\npk_checksum %llu\nkey_checksum %llu\nreenc_checksum %llu\nok: %zu ciphertexts, a key of %zu bytes\n",
              (unsigned long long)checksum(enc), (unsigned long long)checksum(flatten(pk.encryptions)),
              (unsigned long long)checksum(rk.key_encryptions), (unsigned long long)checksum(re), count,
              rk.key_encryptions.size() * sizeof(Torus));
  return 0;
}
