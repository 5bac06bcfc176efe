// The C++ mirror of the TRLWE key switch (rs_tfhe::TrlweSwitchKey in include/rs_tfhe_hip.hpp): packed re-encryption from
// one secret key to another, a generated key against its loaded copy word for word, the slot reversal psi_(2N-1) and the
// refused shapes.  Run by tests/test_gpu_trlwe_switch.py on the GPU; built (only) by tests/test_trlwe_switch_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rs_tfhe_hip.hpp"

using namespace rs_tfhe;

#define REQUIRE(cond)                                                  \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int main() {
  const SecurityParams p = SECURITY_128_BIT;
  Engine &e = Engine::for_params(p, 0);
  const SecretKey alice = SecretKey::generate(p, 11), bob = SecretKey::generate(p, 12);
  uint8_t rng_key[32], mask_seed[32];
  for (int i = 0; i < 32; ++i) rng_key[i] = (uint8_t)(29 * i + 3), mask_seed[i] = (uint8_t)(7 * i + 1);

  std::vector<double> plain(2 * (size_t)N);  // two ciphertexts of booleans
  std::vector<bool> bits(plain.size());
  for (size_t i = 0; i < plain.size(); ++i) {
    bits[i] = ((i * 2654435761u) >> 7) & 1u;
    plain[i] = bits[i] ? 0.125 : -0.125;
  }
  const std::vector<Torus> packed = alice.encrypt_packed_batch(e, plain, mask_seed);

  // re-encryption: k = 1, Alice -> Bob
  TrlweSwitchKey rk = TrlweSwitchKey::generate(alice, bob, 1, 4, 6, 0, rng_key);
  REQUIRE(rk.k == 1 && rk.bodies.size() == 6 * (size_t)N && rk.nbytes() == 6 * (size_t)N * 4 + 32);
  const std::vector<Torus> for_bob = rk.switch_batch(packed.data(), 2);
  REQUIRE(for_bob.size() == packed.size());
  const std::vector<Torus> got = bob.decrypt_packed_batch(e, for_bob, plain.size(), TFHE_HIP_DECRYPT_BOOL);
  size_t wrong = 0;
  for (size_t i = 0; i < bits.size(); ++i) wrong += (got[i] != 0) != bits[i];
  REQUIRE(wrong == 0);
  const std::vector<Torus> still_alice = alice.decrypt_packed_batch(e, for_bob, plain.size(), TFHE_HIP_DECRYPT_BOOL);
  size_t same = 0;
  for (size_t i = 0; i < bits.size(); ++i) same += (still_alice[i] != 0) == bits[i];
  REQUIRE(same < bits.size() * 3 / 4);  // Alice no longer reads it

  // the same generator key gives the same key; a copy built from (S, bodies) alone switches to the same words
  TrlweSwitchKey again = TrlweSwitchKey::generate(alice, bob, 1, 4, 6, 0, rng_key);
  REQUIRE(again.mask_seed == rk.mask_seed && again.bodies == rk.bodies);
  TrlweSwitchKey copy;
  copy.params = p, copy.k = rk.k, copy.basebit = rk.basebit, copy.t = rk.t, copy.mask_seed = rk.mask_seed, copy.bodies = rk.bodies;
  copy.load(0);
  REQUIRE(copy.switch_batch(packed.data(), 2) == for_bob);

  // psi_(2N-1) under one key: slot j moves to N - j, negated (slot 0 stays)
  TrlweSwitchKey rev = TrlweSwitchKey::generate(alice, alice, 2 * (int)N - 1, 4, 6, 0, rng_key);
  const std::vector<Torus> reversed = rev.switch_batch(packed.data(), 1);
  const std::vector<Torus> rb = alice.decrypt_packed_batch(e, reversed, (size_t)N, TFHE_HIP_DECRYPT_BOOL);
  REQUIRE((rb[0] != 0) == bits[0]);
  for (size_t j = 1; j < (size_t)N; ++j) REQUIRE((rb[(size_t)N - j] != 0) == !bits[j]);

  // refused shapes
  for (const int bad_k : {0, 2, 2 * (int)N, -1}) {
    bool threw = false;
    try {
      TrlweSwitchKey::generate(alice, bob, bad_k, 4, 6, 0, rng_key);
    } catch (const std::runtime_error &) {
      threw = true;
    }
    REQUIRE(threw);
  }
  for (const auto &bt : {std::pair<int, int>{8, 4}, {0, 4}, {4, 9}, {4, 0}, {1, 65}}) {
    bool threw = false;
    try {
      TrlweSwitchKey::generate(alice, bob, 1, bt.first, bt.second, 0, rng_key);
    } catch (const std::runtime_error &) {
      threw = true;
    }
    REQUIRE(threw);
  }
  std::printf("test_trlwe_switch ok: %zu bits re-encrypted, key %zu bytes\n", bits.size(), rk.nbytes());
  return 0;
}
