// Encrypted 2-D convolution through the C++ mirror (include/rs_tfhe_hip.hpp) on the GPU at SECURITY_128_BIT, 2 groups of
// a 5 x 5 map, three 3 x 3 filters, stride 1, padding 1: linear::conv2d equals the header's definition, evaluated here
// loop by loop in wrapping u32 arithmetic, word for word -- with in_c = 20 (K = 180: taps and K-steps cross inside a
// fetch) and with in_c = 16 (one tap per fetch) --, a strided case without bias, and every shape the header refuses
// throws.  The convolution uses no key: the cloud key the mirror binds is all zeros.
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

// out[g][oy][ox][oc][x] = sum_{ky,kx,ic} w[oc][ky][kx][ic] * in[g][oy sh + ky - ph][ox sw + kx - pw][ic][x] + bias on x = n
static std::vector<Torus> definition(const tfhe_hip_conv2d_shape &s, const std::vector<int8_t> &w, const Torus *bias,
                                     const std::vector<Torus> &in, size_t groups, size_t width) {
  const size_t out_h = (s.in_h + 2 * s.pad_h - s.k_h) / s.stride_h + 1, out_w = (s.in_w + 2 * s.pad_w - s.k_w) / s.stride_w + 1;
  std::vector<Torus> out(groups * out_h * out_w * s.out_c * width, 0);
  for (size_t g = 0; g < groups; ++g)
    for (size_t oy = 0; oy < out_h; ++oy)
      for (size_t ox = 0; ox < out_w; ++ox)
        for (size_t oc = 0; oc < s.out_c; ++oc) {
          Torus *o = &out[(((g * out_h + oy) * out_w + ox) * s.out_c + oc) * width];
          for (size_t ky = 0; ky < s.k_h; ++ky)
            for (size_t kx = 0; kx < s.k_w; ++kx) {
              const long iy = (long)(oy * s.stride_h + ky) - (long)s.pad_h, ix = (long)(ox * s.stride_w + kx) - (long)s.pad_w;
              if (iy < 0 || iy >= (long)s.in_h || ix < 0 || ix >= (long)s.in_w) continue;  // padding: zero
              for (size_t ic = 0; ic < s.in_c; ++ic) {
                const Torus c = (Torus)(int32_t)w[((oc * s.k_h + ky) * s.k_w + kx) * s.in_c + ic];
                const Torus *row = &in[(((g * s.in_h + (size_t)iy) * s.in_w + (size_t)ix) * s.in_c + ic) * width];
                for (size_t x = 0; x < width; ++x) o[x] += c * row[x];
              }
            }
          if (bias) o[width - 1] += bias[oc];
        }
  return out;
}

static void run_case(const CloudKey &ck, const tfhe_hip_conv2d_shape &s, size_t groups, bool with_bias, const char *what) {
  const size_t width = (size_t)ck.params.n + 1, K = (size_t)s.k_h * s.k_w * s.in_c;
  std::vector<int8_t> w(s.out_c * K);
  for (auto &x : w) x = (int8_t)(next_word() >> 24);
  for (size_t j = 0; j < K; ++j) w[j] = -128, w[K + j] = 127;  // the first two filters: the extremes
  std::vector<Torus> bias(s.out_c);
  for (auto &x : bias) x = next_word();
  std::vector<Torus> in(groups * s.in_h * s.in_w * s.in_c * width);
  for (auto &x : in) x = next_word();
  const Torus edges[7] = {0u, 0x80000000u, 0xFFFFFFFFu, 0x7F7F7F7Fu, 0x80808080u, 0x00800080u, 0x7FFFFFFFu};
  for (size_t c = 0; c < groups * s.in_h * s.in_w * s.in_c; ++c)  // first and last word of every ciphertext
    in[c * width] = edges[c % 7], in[c * width + width - 1] = edges[(c + 3) % 7];
  const Torus *bp = with_bias ? bias.data() : nullptr;
  const std::vector<Torus> got = linear::conv2d(ck, s, w.data(), bp, in.data(), groups);
  const std::vector<Torus> want = definition(s, w, bp, in, groups, width);
  CHECK(got.size() == want.size(), "%s: %zu words, expected %zu", what, got.size(), want.size());
  CHECK(got == want, "%s: the convolution differs from the definition", what);
}

int main() {
  const SecurityParams P = SECURITY_128_BIT;
  CloudKey ck;  // never read by the convolution
  ck.params = P;
  ck.decomposition_offset = gen_decomposition_offset(P);
  ck.blind_rotate_testvec = gen_testvec();
  ck.bootstrapping_key.resize((size_t)P.n * 2 * P.l * 2 * N);
  ck.key_switching_key.resize(N * (size_t)P.iks_t * P.base() * (P.n + 1));

  run_case(ck, tfhe_hip_conv2d_shape{5, 5, 20, 3, 3, 3, 1, 1, 1, 1}, 2, true, "in_c = 20");
  run_case(ck, tfhe_hip_conv2d_shape{5, 5, 16, 3, 3, 3, 1, 1, 1, 1}, 2, true, "in_c = 16");
  run_case(ck, tfhe_hip_conv2d_shape{7, 8, 3, 2, 3, 2, 2, 3, 0, 1}, 1, false, "stride (2, 3), no bias");

  // every shape the header refuses (TFHE_HIP_EINVAL) throws; then the handle still works
  const tfhe_hip_conv2d_shape good{5, 5, 4, 3, 3, 3, 1, 1, 1, 1};
  std::vector<int8_t> w(3 * 3 * 3 * 4, 1);
  std::vector<Torus> in(2 * 5 * 5 * 4 * ((size_t)P.n + 1), 1u);
  auto refused = [&](tfhe_hip_conv2d_shape s, const int8_t *wp, const Torus *ip, size_t groups) {
    try {
      linear::conv2d(ck, s, wp, nullptr, ip, groups);
    } catch (const std::runtime_error &) {
      return true;
    }
    return false;
  };
  tfhe_hip_conv2d_shape s = good;
  s.in_h = 0;
  CHECK(refused(s, w.data(), in.data(), 2), "in_h == 0 was accepted");
  s = good, s.in_c = 0;
  CHECK(refused(s, w.data(), in.data(), 2), "in_c == 0 was accepted");
  s = good, s.out_c = 0;
  CHECK(refused(s, w.data(), in.data(), 2), "out_c == 0 was accepted");
  s = good, s.k_w = 0;
  CHECK(refused(s, w.data(), in.data(), 2), "k_w == 0 was accepted");
  s = good, s.stride_h = 0;
  CHECK(refused(s, w.data(), in.data(), 2), "stride_h == 0 was accepted");
  s = good, s.k_h = 8;
  CHECK(refused(s, w.data(), in.data(), 2), "a filter taller than the padded map was accepted");
  s = good, s.in_c = 65536 / 9 + 1;
  CHECK(refused(s, w.data(), in.data(), 2), "K > 65,536 was accepted");
  s = good, s.pad_w = 0x7FFFFFFFu;
  CHECK(refused(s, w.data(), in.data(), 2), "a padded map past 2^31 - 1 was accepted");
  CHECK(refused(good, nullptr, in.data(), 2), "a NULL w was accepted");
  CHECK(refused(good, w.data(), nullptr, 2), "a NULL in was accepted");
  CHECK(refused(good, w.data(), in.data(), (size_t)1 << 40), "groups * out_h * out_w * out_c > 2^31 - 1 was accepted");
  CHECK(linear::conv2d(ck, good, w.data(), nullptr, in.data(), 0).empty(), "groups == 0 must return nothing");
  const std::vector<Torus> out = linear::conv2d(ck, good, w.data(), nullptr, in.data(), 2);
  // all-ones weights over all-ones words: every word counts the taps inside the map times in_c (16 at a corner)
  CHECK(out.size() == 2 * 5 * 5 * 3 * ((size_t)P.n + 1) && out[0] == 16u && out[(2 * 5 + 2) * 3 * ((size_t)P.n + 1)] == 36u,
        "the handle no longer works after the refused calls");
  std::printf("test_conv2d ok: three geometries bit-exact vs the definition, the refused shapes throw\n");
  return 0;
}
