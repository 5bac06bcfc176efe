// rings.hip -- the ring-row family, one translation unit of libtfhe_hip.so: seeded (compressed) cloud keys and
// ciphertexts, packed TRLWE encryption, decryption, the TRLWE key switch and the packed CMUX.
// What it uses of the core is declared in internal.hpp; every kernel of the headers below is emitted here and nowhere else.
#include "internal.hpp"

#include "seeded.hpp"
#include "trlwe_encrypt.hpp"
#include "decrypt.hpp"
#include "trlwe_switch.hpp"
#include "cmux.hpp"

#if TFHE_ABL_CATALOG
TFHE_MUTANT_PUBLISH(rings)
#endif
