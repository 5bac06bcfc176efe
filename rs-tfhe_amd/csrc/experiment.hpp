// experiment.hpp -- guard for the three mutation switches (NOT product behaviour).
//
// TFHE_ABL_ROUND_LSB / TFHE_ABL_TW_REL falsify one part of the kernels so that the suite can be shown to notice one
// LSB (`make mutation`); the results of such a build are WRONG BY CONSTRUCTION.  TFHE_ABL_CATALOG compiles in the
// catalogue of single defects in the integer kernels (below), of which a run switches on at most one.  They can only
// be switched on together with -DTFHE_EXPERIMENT; such a library reports itself as "hip-gfx950-EXPERIMENT" through
// tfhe_hip_name() and rs_tfhe_amd refuses to load it unless TFHE_HIP_ALLOW_EXPERIMENT=1 is set.
#pragma once
#if (defined(TFHE_ABL_ROUND_LSB) && TFHE_ABL_ROUND_LSB) || (defined(TFHE_ABL_TW_REL) && TFHE_ABL_TW_REL) || \
    (defined(TFHE_ABL_CATALOG) && TFHE_ABL_CATALOG)
#ifndef TFHE_EXPERIMENT
#error "TFHE_ABL_* are mutation switches (results wrong by construction): build with -DTFHE_EXPERIMENT (make mutation)"
#endif
#define TFHE_ABLATED 1
#else
#define TFHE_ABLATED 0
#endif
#ifndef TFHE_ABL_ROUND_LSB  // round_product<false> returns one LSB too much on ~1/1024 of the words, so that
                            // the parity suite can be shown to notice (the l = 1 exact-regime tests must FAIL on this build)
#define TFHE_ABL_ROUND_LSB 0
#endif
#ifndef TFHE_ABL_TW_REL  // in the three fused blind-rotation kernels (not their many-LUT forms, not the stage
                         // kernels, not the host table) ONE pass-2 twiddle entry of the LDS table is multiplied by 1 + 2^-47 -- a
                         // relative error 2^5 above f64's own, invisible where the product is exact (it moves a value of 2^44
                         // by 1/8) and ~2^10 LSB at the 2^57 of the inexact sets: the lock-step tests must FAIL there on this build
#define TFHE_ABL_TW_REL 0
#endif
#ifndef TFHE_ABL_CATALOG  // the catalogue of single defects in the integer kernels (tests/mutants.py says what each one
                          // gets wrong and which tests must fail on it; tests/test_gpu_mutants.py runs them).  All of them
                          // are compiled into ONE library, libtfhe_v_catalog.so, and tfhe_hip_ctx_create switches on the
                          // one TFHE_HIP_MUTANT names (unset or empty: none; an unknown name: TFHE_HIP_EINVAL)
#define TFHE_ABL_CATALOG 0
#endif

// The catalogue.  A site is written `TFHE_MUT(kMut_<name>) ? wrong : right`, and TFHE_MUT(x) is the constant `false` in
// every build without TFHE_ABL_CATALOG: the product's code is the `right` arm alone.
//
// THE RULE FOR EVERY MUTANT: it changes a VALUE only.  It never forms an address that the product build would not form
// in the same launch; it never changes a loop bound, a barrier, a wait count, a launch shape, an allocation size or the
// range of a shift amount.  A defect that could read or write outside what the product touches, or hang, is not
// written: the purpose is wrong words, never a fault.  The blind-rotation kernels, fft512.hpp and the hot loop of
// k_key_switch_mfma carry no site.
//
// One list names the mutants: the enumerators kMut_<name> below, the name table TFHE_HIP_MUTANT is looked up in
// (tfhe_hip.hip) and the names tests/test_mutants_host.py holds tests/mutants.py to are all made from it.
#define TFHE_MUTANT_LIST(X)                                                                                          \
  X(mm_plane_carry) X(mm_a_tail) X(mm_a_sign) X(mm_xcd_rem) X(mm_toeplitz_wrap) X(mm_conv_pad) X(mm_conv_stride)    \
  X(mm_nega_wrap) X(mm_polymul_bias) X(ks_plane_borrow) X(ks_round_split) X(ks_round_digits) X(ts_psi_sign_b)        \
  X(ts_off_top) X(ts_rot3) X(ts_gadget_hi) X(cmux_rnd_b) X(cmux_addend_w) X(trgsw_row_t) X(unpack_diag)              \
  X(dec_tail_bit) X(dec_wrap) X(trlwe_group_hi) X(trgsw_index_hi)
#if TFHE_ABL_CATALOG
#include <hip/hip_runtime.h>
#define TFHE_MUTANT_ENUM(name) kMut_##name,
enum TfheMutant : unsigned { kMutNone = 0, TFHE_MUTANT_LIST(TFHE_MUTANT_ENUM) kMutCount };
#undef TFHE_MUTANT_ENUM
// the selected defect, one word per translation unit (internal.hpp: mutant_publish_*), written once at context creation
static __device__ unsigned g_tfhe_mutant = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#define TFHE_MUT(x) (g_tfhe_mutant == (unsigned)(x))
#else
#define TFHE_MUT(x) false  // (the host pass of a __host__ __device__ function)
#endif
#else
#define TFHE_MUT(x) false
#endif
