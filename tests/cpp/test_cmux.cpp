// The C++ mirror of the packed CMUX (rs_tfhe::Trgsw and rs_tfhe::packing::cmux in include/rs_tfhe_hip.hpp): a selector
// of 0 and one of 1 choose between two packed ciphertexts of booleans in every slot, the same generator key gives the
// same selector, the external product by the bit 1 keeps the message, and the refused shapes throw.  Run by
// tests/test_gpu_cmux.py on the GPU; built (only) by tests/test_cmux_host.py.
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
  Engine &e = Engine::for_params(p, 0);  // no cloud key: the CMUX needs none
  const SecretKey sk = SecretKey::generate(p, 21);
  uint8_t rng_key[32], mask_seed[32];
  for (int i = 0; i < 32; ++i) rng_key[i] = (uint8_t)(31 * i + 9), mask_seed[i] = (uint8_t)(5 * i + 2);

  std::vector<double> plain(2 * (size_t)N);  // two ciphertexts of booleans: d0, then d1
  std::vector<bool> bits(plain.size());
  for (size_t i = 0; i < plain.size(); ++i) {
    bits[i] = ((i * 2654435761u) >> 9) & 1u;
    plain[i] = bits[i] ? 0.125 : -0.125;
  }
  const std::vector<Torus> packed = sk.encrypt_packed_batch(e, plain, mask_seed);
  const Torus *d0 = packed.data(), *d1 = packed.data() + 2 * (size_t)N;

  const Trgsw s0 = Trgsw::encrypt_bool(e, sk, false, 6, 3, rng_key, 0), s1 = Trgsw::encrypt_bool(e, sk, true, 6, 3, rng_key, 6);
  REQUIRE(s0.rows.size() == 6 * 2 * (size_t)N && s1.t == 3 && s1.basebit == 6);
  for (int bit = 0; bit < 2; ++bit) {
    const std::vector<Torus> out = packing::cmux(e, bit ? s1 : s0, d0, d1, 1);
    REQUIRE(out.size() == 2 * (size_t)N);
    const std::vector<Torus> got = sk.decrypt_packed_batch(e, out, (size_t)N, TFHE_HIP_DECRYPT_BOOL);
    size_t wrong = 0;
    for (size_t i = 0; i < (size_t)N; ++i) wrong += (got[i] != 0) != bits[(size_t)bit * N + i];
    REQUIRE(wrong == 0);
  }
  // the same generator key and index: the same selector
  REQUIRE(Trgsw::encrypt_bool(e, sk, true, 6, 3, rng_key, 6).rows == s1.rows);
  REQUIRE(Trgsw::encrypt_bool(e, sk, true, 6, 3, rng_key, 12).rows != s1.rows);
  // the external product by 1 keeps both ciphertexts
  const std::vector<Torus> kept = packing::external_product(e, s1, packed.data(), 2);
  const std::vector<Torus> kb = sk.decrypt_packed_batch(e, kept, plain.size(), TFHE_HIP_DECRYPT_BOOL);
  for (size_t i = 0; i < bits.size(); ++i) REQUIRE((kb[i] != 0) == bits[i]);
  // the reference's digits select as well
  const std::vector<Torus> ref = packing::cmux(e, s1, d0, d1, 1, true);
  const std::vector<Torus> rb = sk.decrypt_packed_batch(e, ref, (size_t)N, TFHE_HIP_DECRYPT_BOOL);
  for (size_t i = 0; i < (size_t)N; ++i) REQUIRE((rb[i] != 0) == bits[(size_t)N + i]);

  // refused shapes
  for (const auto &bt : {std::pair<int, int>{8, 4}, {0, 4}, {4, 9}, {4, 0}, {1, 33}}) {
    bool threw = false;
    try {
      Trgsw::encrypt_bool(e, sk, true, bt.first, bt.second, rng_key);
    } catch (const std::runtime_error &) {
      threw = true;
    }
    REQUIRE(threw);
  }
  Trgsw bad = s1;
  bad.rows.pop_back();
  bool threw = false;
  try {
    packing::cmux(e, bad, d0, d1, 1);
  } catch (const std::runtime_error &) {
    threw = true;
  }
  REQUIRE(threw);
  std::printf("test_cmux ok: %zu slots selected both ways, selector %zu bytes\n", (size_t)N, s1.rows.size() * sizeof(Torus));
  return 0;
}
