// rs_tfhe encrypted linear layers through the C++ mirror (include/rs_tfhe_hip.hpp) on the GPU, rows = 33, cols = 31,
// groups = 2 at SECURITY_128_BIT: linear::matmul equals the wrapping integer sum word for word; linear::matmul_packed
// without the key switch equals the same sum over the oracle's sample_extract_index rows with the exact negation
// (the oracle's Torus::MAX - a plus one in every negated word), and with the key switch the oracle's
// identity_key_switching of those rows.
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
  orc_gen_secret_key(71, P.n, k0.data(), k1.data());
  CloudKey ck;
  ck.params = P;
  ck.decomposition_offset = gen_decomposition_offset(P);
  ck.blind_rotate_testvec = gen_testvec();
  ck.bootstrapping_key.resize((size_t)P.n * 2 * P.l * 2 * N);
  ck.key_switching_key.resize(N * (size_t)P.iks_t * P.base() * (P.n + 1));
  orc_gen_bootstrapping_key(171, &OP, k0.data(), k1.data(), ck.bootstrapping_key.data(), nullptr);
  orc_gen_key_switching_key(172, &OP, k0.data(), k1.data(), ck.key_switching_key.data());

  const size_t rows = 33, cols = 31, groups = 2, w0 = (size_t)P.n + 1, w1 = N + 1;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&]() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (Torus)(s >> 32);
  };
  std::vector<int8_t> w(rows * cols);
  for (auto &x : w) x = (int8_t)(next() >> 24);
  for (size_t j = 0; j < cols; ++j) w[j] = -128, w[cols + j] = 127, w[2 * cols + j] = 0;
  std::vector<Torus> bias(rows);
  for (auto &x : bias) x = next();
  // out[g][r] = sum_j w[r][j] * in[g][j] + bias[r] on the last word, in[g][j] = src + (g * cols + j) * width
  auto product = [&](const std::vector<Torus> &src, size_t width) {
    std::vector<Torus> out(groups * rows * width, 0);
    for (size_t g = 0; g < groups; ++g)
      for (size_t r = 0; r < rows; ++r) {
        Torus *o = &out[(g * rows + r) * width];
        for (size_t j = 0; j < cols; ++j) {
          const Torus c = (Torus)(int32_t)w[r * cols + j];
          const Torus *row = &src[(g * cols + j) * width];
          for (size_t x = 0; x < width; ++x) o[x] += c * row[x];
        }
        o[width - 1] += bias[r];
      }
    return out;
  };

  // dense form
  std::vector<Torus> in(groups * cols * w0);
  for (auto &x : in) x = next();
  const Torus edges[7] = {0u, 0x80000000u, 0xFFFFFFFFu, 0x7F7F7F7Fu, 0x80808080u, 0x00800080u, 0x7FFFFFFFu};
  for (size_t g = 0; g < groups; ++g)
    for (size_t e = 0; e < 7; ++e) in[(g * cols + e) * w0] = in[(g * cols + e) * w0 + w0 - 1] = edges[e];
  const std::vector<Torus> dense = linear::matmul(ck, w.data(), bias.data(), rows, cols, in.data(), groups);
  CHECK(dense == product(in, w0), "dense product differs from the integer sum");

  // packed form: the exact extraction is the oracle's with one added to every negated word (i > j)
  std::vector<Torus> trlwe(groups * 2 * N);
  for (auto &x : trlwe) x = next();
  for (size_t e = 0; e < 7; ++e) trlwe[e] = trlwe[N + e] = edges[e];
  std::vector<Torus> ext(groups * cols * w1);
  for (size_t g = 0; g < groups; ++g)
    for (size_t j = 0; j < cols; ++j) {
      Torus *row = &ext[(g * cols + j) * w1];
      orc_sample_extract_index(&trlwe[g * 2 * N], (int)j, row);
      for (size_t i = j + 1; i < N; ++i) row[i] += 1u;
    }
  const std::vector<Torus> lv1 = product(ext, w1);
  const std::vector<Torus> packed = linear::matmul_packed(ck, w.data(), bias.data(), rows, cols, trlwe.data(), groups, false);
  CHECK(packed == lv1, "packed product (no key switch) differs from the sum over the exact extraction");
  const std::vector<Torus> switched = linear::matmul_packed(ck, w.data(), bias.data(), rows, cols, trlwe.data(), groups);
  CHECK(switched.size() == groups * rows * w0, "matmul_packed returned %zu words", switched.size());
  std::vector<Torus> want(w0);
  for (size_t m = 0; m < groups * rows; ++m) {
    orc_identity_key_switching(&lv1[m * w1], ck.key_switching_key.data(), &OP, want.data());
    CHECK(std::equal(want.begin(), want.end(), switched.begin() + (long)(m * w0)), "row %zu differs from the oracle's key switch", m);
  }
  bool threw = false;
  try {
    linear::matmul(ck, w.data(), nullptr, 0, cols, in.data(), groups);
  } catch (const std::runtime_error &) {
    threw = true;
  }
  CHECK(threw, "rows == 0 was accepted");
  std::printf("test_matmul ok: dense and packed %zux%zu on %zu groups, bit-exact vs the oracle\n", rows, cols, groups);
  return 0;
}
