// planes.hip -- the byte-plane and matrix-core family, one translation unit of libtfhe_hip.so: the packing key switch
// and its key, the encrypted-table key switch and the tree bootstrap, public-key and symmetric TLWE encryption (the
// public key is byte planes of packing.hpp's layout), the unpacking key switch and the encrypted linear layers.
// What it uses of the core is declared in internal.hpp; every kernel of the headers below is emitted here and nowhere else.
#include "internal.hpp"

#include "packing.hpp"
#include "table.hpp"
#include "packing_keygen.hpp"
#include "pk_encrypt.hpp"
#include "sym_encrypt.hpp"
#include "unpack.hpp"
#include "matmul.hpp"

#if TFHE_ABL_CATALOG
TFHE_MUTANT_PUBLISH(planes)
#endif
