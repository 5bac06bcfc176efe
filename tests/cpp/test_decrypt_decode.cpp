// decrypt_decode (rs-tfhe_amd/csrc/decrypt_decode.hpp) compiled for the host: prints the decode of every planted phase
// for tests/test_decrypt_host.py to compare with rs-tfhe_amd/client.py's expressions.  Host code only, its own main:
// the test also builds and runs it once with -fsanitize=address,undefined.
// stdin: lines "mode modulus phase" (decimal).  stdout: one decoded word a line.
#include <cinttypes>
#include <cstdio>

#include "../../rs-tfhe_amd/csrc/decrypt_decode.hpp"

int main() {
  int mode;
  uint32_t modulus, phase;
  size_t lines = 0;
  while (std::scanf("%d %" SCNu32 " %" SCNu32, &mode, &modulus, &phase) == 3) {
    std::printf("%" PRIu32 "\n", decrypt_decode(phase, mode, modulus));
    ++lines;
  }
  return lines ? 0 : 1;
}
