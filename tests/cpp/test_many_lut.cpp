// rs_tfhe many-LUT bindings (include/rs_tfhe_hip.hpp) on the GPU: LutBootstrap::bootstrap_many_lut and
// Circuit::pbs_many with a two-function table (lut::Generator::generate_many_lookup_table, m = 4), every word against
// the CPU oracle's pre-rounding model (inputs rounded to multiples of 2^22, the ordinary blind rotation,
// sample_extract_index(., j), the key switch) at SECURITY_128_BIT, and the decrypted messages against f_j(x).
#include <cstdio>
#include <cstdlib>
#include <cstring>

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
void orc_tlwe_encrypt_f64(uint64_t seed, double p, double alpha, const uint32_t *key, int dim, uint32_t *out);
int orc_tlwe_decrypt_bool(const uint32_t *ct, const uint32_t *key, int dim);
typedef struct {
  orc_params P;
  uint32_t decomposition_offset;
  const uint32_t *testvec;
  const double *bsk_fft;
  const uint32_t *bsk_time;
  const uint32_t *ksk;
} orc_cloud_key;
void orc_batch_blind_rotate(const orc_cloud_key *ck, const uint32_t *in, const uint32_t *testvec, uint32_t *out, int count,
                            int nthreads);
void orc_sample_extract_index(const uint32_t *trlwe, int k, uint32_t *out);
void orc_identity_key_switching(const uint32_t *src, const uint32_t *ksk, const orc_params *P, uint32_t *out);
int orc_tlwe_decrypt_lwe_message(const uint32_t *ct, int message_modulus, const uint32_t *key, int dim);
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
  orc_gen_secret_key(41, P.n, k0.data(), k1.data());
  CloudKey ck;
  ck.params = P;
  ck.decomposition_offset = gen_decomposition_offset(P);
  ck.blind_rotate_testvec = gen_testvec();
  ck.bootstrapping_key.resize((size_t)P.n * 2 * P.l * 2 * N);
  ck.key_switching_key.resize(N * (size_t)P.iks_t * P.base() * (P.n + 1));
  orc_gen_bootstrapping_key(141, &OP, k0.data(), k1.data(), ck.bootstrapping_key.data(), nullptr);
  orc_gen_key_switching_key(142, &OP, k0.data(), k1.data(), ck.key_switching_key.data());
  const orc_cloud_key ock{OP, ck.decomposition_offset, ck.blind_rotate_testvec.a.data(), ck.bootstrapping_key.data(), nullptr,
                          ck.key_switching_key.data()};

  const int m = 4, k = 2;
  const std::vector<std::function<size_t(size_t)>> fs = {[](size_t x) { return (x + 1) % 4; }, [](size_t x) { return (3 * x) % 4; }};
  const lut::LookupTable tab = lut::Generator(m).generate_many_lookup_table(fs);
  const size_t w = (size_t)P.n + 1;
  // the model: ct -> [k] ciphertexts
  auto model = [&](const Ciphertext &ct) {
    std::vector<Torus> r(w);
    for (size_t i = 0; i < w; ++i) r[i] = (Torus)((((uint64_t)ct.p[i] + (1ull << 21)) >> 22) << 22);
    std::vector<Torus> tr(2 * N), lv1(N + 1);
    orc_batch_blind_rotate(&ock, r.data(), tab.poly.a.data(), tr.data(), 1, 1);
    std::vector<Ciphertext> out(k, Ciphertext(P.n));
    for (int j = 0; j < k; ++j) {
      orc_sample_extract_index(tr.data(), j, lv1.data());
      orc_identity_key_switching(lv1.data(), ck.key_switching_key.data(), &OP, out[j].p.data());
    }
    return out;
  };
  uint64_t seed = 9;
  const int B = 5;
  std::vector<std::vector<Ciphertext>> in(1, std::vector<Ciphertext>(B, Ciphertext(P.n)));
  for (int x = 0; x < B; ++x) orc_tlwe_encrypt_f64(seed++, (double)(x % m) / (2.0 * m), P.alpha_lv0, k0.data(), P.n, in[0][x].p.data());

  // LutBootstrap::bootstrap_many_lut, one ciphertext at a time
  LutBootstrap lb;
  for (int x = 0; x < B; ++x) {
    const auto got = lb.bootstrap_many_lut(in[0][x], tab, k, ck);
    const auto want = model(in[0][x]);
    CHECK(got.size() == (size_t)k, "bootstrap_many_lut returned %zu ciphertexts", got.size());
    for (int j = 0; j < k; ++j) {
      CHECK(got[j].p == want[j].p, "bootstrap_many_lut x = %d, function %d differs from the oracle", x, j);
      const int v = orc_tlwe_decrypt_lwe_message(got[j].p.data(), m, k0.data(), P.n);
      CHECK(v == (int)fs[j](x % m), "bootstrap_many_lut x = %d, function %d decrypted to %d", x, j, v);
    }
  }

  // Circuit::pbs_many: one two-function node over the input, a batch of B in one run
  Circuit circ(1);
  const uint32_t lid = circ.lut(tab.poly);
  const auto wires = circ.pbs_many(1, 0, 0, 0, 0, lid, k);
  CHECK(wires.size() == 2 && wires[1] == wires[0] + 1, "pbs_many wires");
  const auto got = circ.run(ck, in, {wires[0], wires[1]});
  for (int x = 0; x < B; ++x) {
    const auto want = model(in[0][x]);
    for (int j = 0; j < k; ++j) CHECK(got[j][x].p == want[j].p, "pbs_many x = %d, function %d differs from the oracle", x, j);
  }
  std::printf("test_many_lut ok: bootstrap_many_lut and Circuit::pbs_many, k = %d, B = %d, bit-exact vs the oracle\n", k, B);
  return 0;
}
