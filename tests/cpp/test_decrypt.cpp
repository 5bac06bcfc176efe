// Decryption from C++ alone (include/rs_tfhe_hip.hpp: SecretKey::decrypt_batch / phase_batch -> tfhe_hip_batch_decrypt,
// decrypt_packed_batch / packed_phase_batch -> tfhe_hip_batch_decrypt_trlwe): ciphertexts made on the host one at a
// time, decrypted on the GPU in one call, every word compared with the tlwe:: functions of the same header and, for
// the packed form, with the negacyclic product written out as two loops.
// usage: test_decrypt [count]        (SECURITY_128_BIT, device 0)
#include <cstdio>
#include <cstdlib>

#include "rs_tfhe_hip.hpp"

using namespace rs_tfhe;

static int fail(const char *what, size_t at) {
  std::fprintf(stderr, "FAIL: %s at %zu\n", what, at);
  return 1;
}

int main(int argc, char **argv) {
  const size_t count = argc > 1 ? (size_t)std::atoll(argv[1]) : 257;
  const SecurityParams P = SECURITY_128_BIT;
  ChaChaRng rng(11);
  const SecretKey sk = SecretKey::generate(P, rng);
  Engine &e = Engine::for_params(P, 0);

  // booleans: phases, then the decode
  std::vector<Ciphertext> bits;
  for (size_t m = 0; m < count; ++m) bits.push_back(tlwe::encrypt_bool(m % 3 == 0, P.alpha_lv0, sk.key_lv0, rng));
  const std::vector<Torus> ph = sk.phase_batch(e, bits), bo = sk.decrypt_batch(e, bits, TFHE_HIP_DECRYPT_BOOL);
  if (ph.size() != count || bo.size() != count) return fail("sizes", 0);
  for (size_t m = 0; m < count; ++m) {
    if (ph[m] != tlwe::phase(bits[m], sk.key_lv0)) return fail("phase", m);
    if ((bo[m] != 0) != tlwe::decrypt_bool(bits[m], sk.key_lv0) || bo[m] > 1u || (bo[m] != 0) != (m % 3 == 0)) return fail("bool", m);
  }
  // messages
  for (const uint32_t modulus : {2u, 3u, 10u, 16u}) {
    std::vector<Ciphertext> msgs;
    for (size_t m = 0; m < count; ++m) msgs.push_back(tlwe::encrypt_lwe_message(m, modulus, P.alpha_lv0, sk.key_lv0, rng));
    const std::vector<Torus> got = sk.decrypt_batch(e, msgs, TFHE_HIP_DECRYPT_MESSAGE, modulus);
    for (size_t m = 0; m < count; ++m)
      if (got[m] != tlwe::decrypt_lwe_message(msgs[m], modulus, sk.key_lv0) || got[m] != m % modulus) return fail("message", m);
  }
  // packed: three groups of random words, the last one cut short
  const size_t groups = 3, slots = 2 * (size_t)N + 5;
  std::vector<Torus> packed(groups * 2 * (size_t)N);
  for (Torus &w : packed) w = (Torus)rng();
  const std::vector<Torus> pp = sk.packed_phase_batch(e, packed, slots);
  const std::vector<Torus> pb = sk.decrypt_packed_batch(e, packed, slots, TFHE_HIP_DECRYPT_BOOL);
  if (pp.size() != slots || pb.size() != slots) return fail("packed sizes", 0);
  for (size_t i = 0; i < slots; ++i) {
    const Torus *a = &packed[(i / N) * 2 * (size_t)N], *b = a + N;
    const size_t c = i % N;
    Torus prod = 0;  // coefficient c of A (*) s1 mod X^N + 1
    for (size_t j = 0; j < (size_t)N; ++j)
      if (sk.key_lv1[j]) prod += j <= c ? a[c - j] : (Torus)(0u - a[(size_t)N + c - j]);
    if (pp[i] != (Torus)(b[c] - prod)) return fail("packed phase", i);
    if (pb[i] != ((int32_t)pp[i] >= 0 ? 1u : 0u)) return fail("packed bool", i);
  }
  // refusals surface as exceptions: a modulus outside [2, 65536]
  bool threw = false;
  try {
    (void)sk.decrypt_batch(e, bits, TFHE_HIP_DECRYPT_MESSAGE, 1);
  } catch (const std::exception &) {
    threw = true;
  }
  if (!threw) return fail("modulus 1 was accepted", 0);
  std::printf("ok: %zu ciphertexts, 4 moduli, %zu packed slots\n", count, slots);
  return 0;
}
