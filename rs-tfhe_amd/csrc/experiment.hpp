// experiment.hpp -- guard for the two mutation switches (NOT product behaviour).
//
// TFHE_ABL_ROUND_LSB / TFHE_ABL_TW_REL falsify one part of the kernels so that the suite can be shown to notice one
// LSB (`make mutation`); the results of such a build are WRONG BY CONSTRUCTION.  They can only be switched on
// together with -DTFHE_EXPERIMENT; such a library reports itself as "hip-gfx950-EXPERIMENT" through
// tfhe_hip_name() and rs_tfhe_amd refuses to load it unless TFHE_HIP_ALLOW_EXPERIMENT=1 is set.
#pragma once
#if (defined(TFHE_ABL_ROUND_LSB) && TFHE_ABL_ROUND_LSB) || (defined(TFHE_ABL_TW_REL) && TFHE_ABL_TW_REL)
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
