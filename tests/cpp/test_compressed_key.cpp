// rs_tfhe seeded (compressed) cloud keys through the C++ mirror (include/rs_tfhe_hip.hpp) on the GPU:
// SecretKey::compressed_cloud_key generates one, Engine::load_compressed_cloud_key loads it into a resident key view
// of the Engine's registry (found again, not reloaded, on the next call), and a NAND batch under it decrypts to the
// truth table.  The key's sizes are checked against
// tfhe_hip_compressed_key_words.
#include <cstdio>
#include <cstdlib>

#include "rs_tfhe_hip.hpp"

using namespace rs_tfhe;

int main() {
  const SecurityParams &P = SECURITY_128_BIT;
  SecretKey sk = SecretKey::generate(P, 11);
  ChaChaRng rng(12);
  const CompressedCloudKey ck = sk.compressed_cloud_key(rng, 0);
  tfhe_hip_params cp{P.n, P.l, P.bgbit, P.basebit, P.iks_t};
  size_t bw = 0, kw = 0;
  if (tfhe_hip_compressed_key_words(&cp, &bw, &kw) != TFHE_HIP_OK || bw != ck.bsk_bodies.size() || kw != ck.ksk_bodies.size()) {
    std::fprintf(stderr, "FAIL: sizes\n");
    return 1;
  }
  Engine &e = Engine::for_params(P, 0);
  const size_t resident = e.resident_keys();
  Engine::Bound bound = Engine::load_compressed_cloud_key(ck, 0);
  if (e.resident_keys() != resident + 1 || Engine::for_key(ck, 0).handle() != bound.handle()) {
    std::fprintf(stderr, "FAIL: the compressed key's view is not resident in the registry\n");
    return 1;
  }
  const int count = 64;
  std::vector<Torus> a((size_t)count * (P.n + 1)), b(a.size()), out(a.size());
  std::vector<bool> va(count), vb(count);
  for (int i = 0; i < count; ++i) {
    va[i] = (i & 1) != 0;
    vb[i] = (i & 2) != 0;
    const Ciphertext ca = tlwe::encrypt_bool(va[i], P.alpha_lv0, sk.key_lv0, rng);
    const Ciphertext cb = tlwe::encrypt_bool(vb[i], P.alpha_lv0, sk.key_lv0, rng);
    std::copy(ca.p.begin(), ca.p.end(), a.begin() + (size_t)i * (P.n + 1));
    std::copy(cb.p.begin(), cb.p.end(), b.begin() + (size_t)i * (P.n + 1));
  }
  bound.with_key(ck, [&](tfhe_hip_ctx *h) { return tfhe_hip_batch_gate(h, TFHE_HIP_NAND, a.data(), b.data(), out.data(), count); });
  int bad = 0;
  for (int i = 0; i < count; ++i) {
    Ciphertext c(P.n);
    std::copy(out.begin() + (size_t)i * (P.n + 1), out.begin() + (size_t)(i + 1) * (P.n + 1), c.p.begin());
    if (tlwe::decrypt_bool(c, sk.key_lv0) != !(va[i] && vb[i])) ++bad;
  }
  if (bad) {
    std::fprintf(stderr, "FAIL: %d of %d NANDs wrong after a compressed load\n", bad, count);
    return 1;
  }
  std::printf("ok: compressed key %zu bytes, %d NANDs decrypt\n", ck.nbytes(), count);
  return 0;
}
