// rs_tfhe tree bootstrap through the C++ mirror (include/rs_tfhe_hip.hpp) on the GPU, SECURITY_UINT4:
// Engine::pack_table under a PackingKey made by the numpy client equals the integer model word for word, and
// Engine::bootstrap_bivariate with lut::Generator::generate_bivariate_tables equals the same steps made by hand
// (tfhe_hip_batch_lincomb_bootstrap_many, pack_table, tfhe_hip_batch_bootstrap with one table per ciphertext) and
// decrypts to f(x, y).  The case comes from tests/test_gpu_table.py in one binary file: seed[32], m, k, count, rows (u64
// each), bodies, s0, s1, stage-1 words [m][rows][n+1], the expected tables [rows][2][N] (u32).
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

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      std::fprintf(stderr, "FAIL: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");                 \
      return 1;                                   \
    }                                             \
  } while (0)

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: test_bivariate CASE\n");
    return 2;
  }
  const SecurityParams &P = SECURITY_UINT4;
  const size_t w = (size_t)P.n + 1;
  std::ifstream f(argv[1], std::ios::binary);
  PackingKey pk;
  pk.params = P;
  uint64_t head[4] = {0, 0, 0, 0};
  SecretKey sk;
  sk.params = P;
  std::vector<Torus> stage1, want;
  f.read(reinterpret_cast<char *>(pk.mask_seed.data()), 32);
  f.read(reinterpret_cast<char *>(head), sizeof head);
  const int m = (int)head[0], k = (int)head[1];
  const size_t count = head[2], rows = head[3];
  CHECK(f && read_into(f, pk.bodies, (size_t)P.n * P.iks_t * N) && read_into(f, sk.key_lv0, (size_t)P.n) &&
            read_into(f, sk.key_lv1, N) && read_into(f, stage1, (size_t)m * rows * w) && read_into(f, want, rows * 2 * N),
        "short case file");

  // pack_table against the model's words (twice: the second call reuses the loaded key)
  Engine &e = Engine::for_params(P, 0);
  CHECK(e.pack_table(pk, stage1.data(), m, rows) == want, "pack_table differs from the model");
  CHECK(e.pack_table(pk, stage1.data(), m, rows) == want, "pack_table differs from the model on the second call");

  // the tree bootstrap of a random table
  ChaChaRng rng(77);
  std::vector<size_t> T((size_t)m * m), xs(count), ys(count);
  for (auto &v : T) v = rng() % (size_t)m;
  const auto fn = [&](size_t x, size_t y) { return T[x * (size_t)m + y]; };
  const std::vector<Torus> tables = lut::Generator((size_t)m).generate_bivariate_tables(fn, (size_t)k);
  CHECK(tables.size() == (size_t)(m / k) * 2 * N, "generate_bivariate_tables size");
  const CloudKey ck = generate_cloud_key_seeded(sk, 5);
  std::vector<Torus> cx(count * w), cy(count * w);
  for (size_t c = 0; c < count; ++c) {
    xs[c] = rng() % (size_t)m;
    ys[c] = rng() % (size_t)m;
    const Ciphertext a = tlwe::encrypt_lwe_message(xs[c], (size_t)m, P.alpha_lv0, sk.key_lv0, rng);
    const Ciphertext b = tlwe::encrypt_lwe_message(ys[c], (size_t)m, P.alpha_lv0, sk.key_lv0, rng);
    std::copy(a.p.begin(), a.p.end(), cx.begin() + c * w);
    std::copy(b.p.begin(), b.p.end(), cy.begin() + c * w);
  }
  const std::vector<Torus> got = Engine::bootstrap_bivariate(ck, pk, cx.data(), cy.data(), tables, m, k, true, count);
  CHECK(got.size() == count * w, "bootstrap_bivariate size");

  // the same steps by hand, under the same key view
  std::vector<Torus> s1((size_t)m * count * w), hand(count * w);
  Engine::Bound b = Engine::for_key(ck, 0);
  for (int j = 0; j < m / k; ++j)
    b.with_key(ck, [&](tfhe_hip_ctx *h) {
      return tfhe_hip_batch_lincomb_bootstrap_many(h, 1, cy.data(), 0, nullptr, 0, tables.data() + (size_t)j * 2 * N, 0, k, 1,
                                                   s1.data() + (size_t)j * k * count * w, count);
    });
  const std::vector<Torus> tv = e.pack_table(pk, s1.data(), m, count);
  b.with_key(ck, [&](tfhe_hip_ctx *h) { return tfhe_hip_batch_bootstrap(h, cx.data(), tv.data(), 1, 1, hand.data(), count); });
  CHECK(got == hand, "bootstrap_bivariate differs from the steps made by hand");

  int bad = 0;
  for (size_t c = 0; c < count; ++c) {
    Ciphertext o(P.n);
    std::copy(got.begin() + c * w, got.begin() + (c + 1) * w, o.p.begin());
    if (tlwe::decrypt_lwe_message(o, (size_t)m, sk.key_lv0) != fn(xs[c], ys[c])) ++bad;
  }
  CHECK(bad == 0, "%d of %zu outputs decrypt wrong", bad, count);
  std::printf("test_bivariate ok: pack_table (%zu tables, m = %d) word for word, bootstrap_bivariate m = %d, k = %d, %zu inputs\n",
              rows, m, m, k, count);
  return 0;
}
