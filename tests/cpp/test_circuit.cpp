// rs_tfhe::Circuit (include/rs_tfhe_hip.hpp) on the GPU: examples/add_two_numbers.rs's 8-bit addition as a circuit,
// a batch of 7 additions in one run, every wire checked word for word against the CPU oracle evaluating the same gates
// one by one, and the decrypted sums against integer addition.  Key material comes from the oracle library.
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
int orc_batch_gate(const orc_cloud_key *ck, int op, const uint32_t *a, const uint32_t *b, uint32_t *out, int count, int nthreads);
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

  // examples/add_two_numbers.rs:52-80, eight bits, B = 7 independent additions
  const int bits = 8, B = 7;
  Circuit circ(2 * bits + 1);
  std::vector<Circuit::Wire> a, b;
  for (int i = 0; i < bits; ++i) a.push_back(i), b.push_back(bits + i);
  auto sum = circ.add(a, b, 2 * bits);
  const uint32_t xs[B] = {0, 1, 77, 128, 200, 255, 255}, ys[B] = {0, 1, 100, 128, 55, 1, 255};
  const bool cins[B] = {false, true, false, true, false, false, true};
  std::vector<std::vector<Ciphertext>> in(2 * bits + 1, std::vector<Ciphertext>(B, Ciphertext(P.n)));
  uint64_t seed = 7;
  auto enc = [&](bool v, Ciphertext &c) { orc_tlwe_encrypt_f64(seed++, v ? 0.125 : -0.125, P.alpha_lv0, k0.data(), P.n, c.p.data()); };
  for (int j = 0; j < B; ++j) {
    for (int i = 0; i < bits; ++i) {
      enc((xs[j] >> i) & 1, in[i][j]);
      enc((ys[j] >> i) & 1, in[bits + i][j]);
    }
    enc(cins[j], in[2 * bits][j]);
  }
  const uint32_t n_wires = 2 * bits + 1 + 5 * bits;
  std::vector<Circuit::Wire> all;
  for (uint32_t w = 0; w < n_wires; ++w) all.push_back(w);
  const auto got = circ.run(ck, in, all);

  // the oracle, gate by gate in the example's order (full_adder: xor, and, and, xor, or)
  const size_t w = (size_t)P.n + 1;
  std::vector<std::vector<Torus>> ref(n_wires, std::vector<Torus>(B * w));
  for (uint32_t i = 0; i < 2 * bits + 1; ++i)
    for (int j = 0; j < B; ++j) std::memcpy(&ref[i][j * w], in[i][j].p.data(), w * 4);
  uint32_t next = 2 * bits + 1;
  auto gate = [&](int op, uint32_t x, uint32_t y) {
    CHECK(orc_batch_gate(&ock, op, ref[x].data(), ref[y].data(), ref[next].data(), B, 0) == 0, "oracle gate");
    return next++;
  };
  uint32_t carry = 2 * bits;
  for (int i = 0; i < bits; ++i) {
    const uint32_t axb = gate(TFHE_HIP_XOR, a[i], b[i]), aab = gate(TFHE_HIP_AND, a[i], b[i]);
    const uint32_t axbc = gate(TFHE_HIP_AND, axb, carry);
    gate(TFHE_HIP_XOR, axb, carry);
    carry = gate(TFHE_HIP_OR, aab, axbc);
  }
  int wrong = 0;
  for (uint32_t k = 0; k < n_wires; ++k)
    for (int j = 0; j < B; ++j) wrong += std::memcmp(got[k][j].p.data(), &ref[k][j * w], w * 4) != 0;
  CHECK(wrong == 0, "%d of %u ciphertexts differ from the oracle", wrong, n_wires * B);
  for (int j = 0; j < B; ++j) {
    uint32_t v = 0;
    for (int i = 0; i < bits; ++i) v |= (uint32_t)orc_tlwe_decrypt_bool(got[sum.first[i]][j].p.data(), k0.data(), P.n) << i;
    v |= (uint32_t)orc_tlwe_decrypt_bool(got[sum.second][j].p.data(), k0.data(), P.n) << bits;
    CHECK(v == xs[j] + ys[j] + cins[j], "batch element %d: %u + %u + %d decrypted to %u", j, xs[j], ys[j], cins[j], v);
  }
  std::printf("test_circuit ok: 8-bit add, B = %d, %u wires bit-exact vs the oracle, sums correct\n", B, n_wires);
  return 0;
}
