// Plaintext polynomial products on packed ciphertexts through the C++ mirror (include/rs_tfhe_hip.hpp) on the GPU:
// linear::polymul equals the header's definition, evaluated here as the schoolbook double sum in wrapping u32
// arithmetic, word for word -- rows = 3, cols = 2, 2 groups with a bias polynomial, and the same without bias --,
// linear::monomial rotates with the negacyclic sign, and every shape the header refuses throws.  The product uses no
// key: the cloud key the mirror binds is all zeros.
#include <cstdio>
#include <cstdlib>

#include "rs_tfhe_hip.hpp"

using namespace rs_tfhe;

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");                 \
      std::exit(1);                               \
    }                                             \
  } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static Torus next_word() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (Torus)(g_state >> 32);
}

// out[g][r][c][i] = sum_j sum_m w[r][j][m] * ext_{in[g][j][c]}[i - m] + (c == b ? bias[r][i] : 0)
static std::vector<Torus> definition(const std::vector<int8_t> &w, const Torus *bias, size_t rows, size_t cols,
                                     const std::vector<Torus> &in, size_t groups) {
  std::vector<Torus> out(groups * rows * 2 * N, 0);
  for (size_t g = 0; g < groups; ++g)
    for (size_t r = 0; r < rows; ++r)
      for (size_t c = 0; c < 2; ++c) {
        Torus *o = &out[((g * rows + r) * 2 + c) * N];
        for (size_t j = 0; j < cols; ++j) {
          const Torus *p = &in[((g * cols + j) * 2 + c) * N];
          const int8_t *wp = &w[(r * cols + j) * N];
          for (size_t m = 0; m < N; ++m) {
            const Torus k = (Torus)(int32_t)wp[m];
            if (!k) continue;
            for (size_t i = 0; i < N; ++i) o[i] += k * (i >= m ? p[i - m] : (Torus)0 - p[N + i - m]);
          }
        }
        if (bias && c == 1)
          for (size_t i = 0; i < N; ++i) o[i] += bias[r * N + i];
      }
  return out;
}

int main() {
  const SecurityParams P = SECURITY_128_BIT;
  CloudKey ck;  // never read by the product
  ck.params = P;
  ck.decomposition_offset = gen_decomposition_offset(P);
  ck.blind_rotate_testvec = gen_testvec();
  ck.bootstrapping_key.resize((size_t)P.n * 2 * P.l * 2 * N);
  ck.key_switching_key.resize(N * (size_t)P.iks_t * P.base() * (P.n + 1));

  const size_t rows = 3, cols = 2, groups = 2;
  std::vector<int8_t> w(rows * cols * N);
  for (auto &x : w) x = (int8_t)(next_word() >> 24);
  for (size_t m = 0; m < N; ++m) w[m] = -128, w[N + m] = 127;  // row 0: the extremes
  std::vector<Torus> bias(rows * N), in(groups * cols * 2 * N);
  for (auto &x : bias) x = next_word();
  for (auto &x : in) x = next_word();
  const Torus edges[7] = {0u, 0x80000000u, 0xFFFFFFFFu, 0x7F7F7F7Fu, 0x80808080u, 0x00800080u, 0x7FFFFFFFu};
  for (size_t q = 0; q < groups * cols * 2; ++q)  // the first and the last word of every polynomial
    in[q * N] = edges[q % 7], in[q * N + N - 1] = edges[(q + 3) % 7];
  for (const Torus *bp : {(const Torus *)bias.data(), (const Torus *)nullptr}) {
    const std::vector<Torus> got = linear::polymul(ck, w.data(), bp, rows, cols, in.data(), groups);
    CHECK(got == definition(w, bp, rows, cols, in, groups), "the product differs from the definition (%s bias)",
          bp ? "with" : "without");
  }

  // X^k and -X^k on one ciphertext: slot i moves to i + k, what passes N comes back negated
  for (size_t k : {(size_t)0, (size_t)1, (size_t)17, (size_t)1023})
    for (int sign : {1, -1}) {
      const std::vector<int8_t> mono = linear::monomial(k, sign);
      const std::vector<Torus> got = linear::polymul(ck, mono.data(), nullptr, 1, 1, in.data(), 1);
      CHECK(got.size() == 2 * N, "monomial: %zu words", got.size());
      for (size_t c = 0; c < 2; ++c)
        for (size_t i = 0; i < N; ++i) {
          const Torus v = i >= k ? in[c * N + i - k] : (Torus)0 - in[c * N + N + i - k];
          CHECK(got[c * N + i] == (sign > 0 ? v : (Torus)0 - v), "monomial %d X^%zu: component %zu word %zu", sign, k, c, i);
        }
    }
  bool threw = false;
  try {
    linear::monomial(N);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  CHECK(threw, "monomial(N) was accepted");

  // every shape the header refuses (TFHE_HIP_EINVAL) throws; then the handle still works
  auto refused = [&](const int8_t *wp, size_t r, size_t c, const Torus *ip, size_t g) {
    try {
      linear::polymul(ck, wp, nullptr, r, c, ip, g);
    } catch (const std::runtime_error &) {
      return true;
    }
    return false;
  };
  CHECK(refused(w.data(), 0, cols, in.data(), groups), "rows == 0 was accepted");
  CHECK(refused(w.data(), rows, 0, in.data(), groups), "cols == 0 was accepted");
  CHECK(refused(w.data(), rows, 65, in.data(), groups), "cols == 65 was accepted");
  CHECK(refused(nullptr, rows, cols, in.data(), groups), "a NULL w was accepted");
  CHECK(refused(w.data(), rows, cols, nullptr, groups), "a NULL trlwe was accepted");
  CHECK(refused(w.data(), (size_t)1 << 16, cols, in.data(), (size_t)1 << 15), "rows * groups > 2^31 - 1 was accepted");
  CHECK(linear::polymul(ck, w.data(), nullptr, rows, cols, in.data(), 0).empty(), "groups == 0 must return nothing");
  const std::vector<int8_t> one = linear::monomial(0);
  const std::vector<Torus> same = linear::polymul(ck, one.data(), nullptr, 1, 1, in.data(), 1);
  CHECK(same == std::vector<Torus>(in.begin(), in.begin() + 2 * N), "the handle no longer works after the refused calls");
  std::printf("test_polymul ok: dense and monomial products bit-exact vs the definition, the refused shapes throw\n");
  return 0;
}
