// rs_tfhe unpacking key switch through the C++ mirror (include/rs_tfhe_hip.hpp) on the GPU: Engine::unpack of a
// client-packed TRLWE (booleans in the slots, encrypted here with the exact negacyclic product) equals the CPU oracle's
// sample_extract_index followed by identity_key_switching word for word at SECURITY_128_BIT, with slots == nullptr and
// with a selection (duplicates, reversed order, the last slot), and the results decrypt to the encrypted bits.
#include <cstdio>
#include <cstdlib>

#include "rs_tfhe_hip.hpp"

extern "C" {
typedef struct {
  int32_t n, l, bgbit, basebit, t;
  double alpha_lv0, alpha_lv1;
} orc_params;
void orc_init(void);
void orc_gen_secret_key(uint64_t seed, int n, uint32_t *key_lv0, uint32_t *key_lv1);
void orc_gen_bootstrapping_key(uint64_t seed, const orc_params *P, const uint32_t *k0, const uint32_t *k1,
                               double *bsk_fft, uint32_t *bsk_time);
void orc_gen_key_switching_key(uint64_t seed, const orc_params *P, const uint32_t *k0, const uint32_t *k1,
                               uint32_t *ksk);
int orc_tlwe_decrypt_bool(const uint32_t *ct, const uint32_t *key, int dim);
void orc_sample_extract_index(const uint32_t *trlwe, int k, uint32_t *out);
void orc_identity_key_switching(const uint32_t *src, const uint32_t *ksk, const orc_params *P, uint32_t *out);
}

using namespace rs_tfhe;

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");                 \
      std::exit(1);                               \
    }                                             \
  } while (0)

int main() {
  orc_init();
  const SecurityParams P = SECURITY_128_BIT;
  orc_params OP{P.n, P.l, P.bgbit, P.basebit, P.iks_t, P.alpha_lv0, P.alpha_lv1};
  std::vector<Torus> k0(P.n), k1(N);
  orc_gen_secret_key(51, P.n, k0.data(), k1.data());
  CloudKey ck;
  ck.params = P;
  ck.decomposition_offset = gen_decomposition_offset(P);
  ck.blind_rotate_testvec = gen_testvec();
  ck.bootstrapping_key.resize((size_t)P.n * 2 * P.l * 2 * N);
  ck.key_switching_key.resize(N * (size_t)P.iks_t * P.base() * (P.n + 1));
  orc_gen_bootstrapping_key(151, &OP, k0.data(), k1.data(), ck.bootstrapping_key.data(), nullptr);
  orc_gen_key_switching_key(152, &OP, k0.data(), k1.data(), ck.key_switching_key.data());

  // two groups of booleans at +-1/8 under s1: a from a 64-bit LCG, b = a (*) s1 + message (no noise: the key switch adds its own)
  const size_t groups = 2, w = (size_t)P.n + 1;
  std::vector<Torus> trlwe(groups * 2 * N);
  std::vector<int> bits(groups * N);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&]() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (Torus)(s >> 32);
  };
  for (size_t g = 0; g < groups; ++g) {
    Torus *a = &trlwe[g * 2 * N], *b = a + N;
    for (size_t i = 0; i < N; ++i) a[i] = next();
    for (size_t j = 0; j < N; ++j) {
      bits[g * N + j] = (int)(next() & 1u);
      Torus acc = bits[g * N + j] ? 0x20000000u : 0xE0000000u;
      for (size_t k = 0; k < N; ++k)
        if (k1[k]) acc += k <= j ? a[j - k] : (Torus)0 - a[j + N - k];
      b[j] = acc;
    }
  }
  auto model = [&](size_t slot, Torus *out) {
    std::vector<Torus> lv1(N + 1);
    orc_sample_extract_index(&trlwe[(slot / N) * 2 * N], (int)(slot % N), lv1.data());
    orc_identity_key_switching(lv1.data(), ck.key_switching_key.data(), &OP, out);
  };

  const size_t count = N + 5;  // the second group partially
  const std::vector<Torus> got = Engine::unpack(ck, trlwe.data(), groups, nullptr, count);
  CHECK(got.size() == count * w, "unpack returned %zu words", got.size());
  std::vector<Torus> want(w);
  for (size_t m = 0; m < count; ++m) {
    model(m, want.data());
    CHECK(std::equal(want.begin(), want.end(), got.begin() + (long)(m * w)), "slot %zu differs from the oracle", m);
    CHECK(orc_tlwe_decrypt_bool(&got[m * w], k0.data(), P.n) == bits[m], "slot %zu decrypts wrong", m);
  }
  const std::vector<uint32_t> slots = {2047, 2047, 1024, 1023, 517, 1, 0, 2047};
  const std::vector<Torus> sel = Engine::unpack(ck, trlwe.data(), groups, slots.data(), slots.size());
  for (size_t m = 0; m < slots.size(); ++m) {
    model(slots[m], want.data());
    CHECK(std::equal(want.begin(), want.end(), sel.begin() + (long)(m * w)), "selection %zu (slot %u) differs from the oracle", m, slots[m]);
    CHECK(orc_tlwe_decrypt_bool(&sel[m * w], k0.data(), P.n) == bits[slots[m]], "selection %zu decrypts wrong", m);
  }
  bool threw = false;
  const uint32_t bad = 2048;
  try {
    Engine::unpack(ck, trlwe.data(), groups, &bad, 1);
  } catch (const std::runtime_error &) {
    threw = true;
  }
  CHECK(threw, "a slot out of range was accepted");  // (and the process still exits cleanly after a recorded failure)
  std::printf("test_unpack ok: %zu slots and a selection of %zu, bit-exact vs the oracle\n", count, slots.size());
  return 0;
}
