"""The mutation catalogue: one realistic single defect per entry in the integer kernels (csrc/experiment.hpp
TFHE_ABL_CATALOG, `make mutation` -> libtfhe_v_catalog.so, selected at context creation by TFHE_HIP_MUTANT).

Data only: no tests, no device import.  tests/test_gpu_mutants.py runs one child pytest per entry on the entry's
`killers` (node ids that must FAIL on the defect, with an assertion error of a word-for-word comparison) and `controls`
(node ids of a killer's file that the defect cannot reach and that must pass); tests/test_mutants_host.py holds the names
to the sources and the node ids to the suite.  `seconds` is the wall time of the same child (killers + controls) on the
PRODUCT library on an MI355X, interpreter start included; the child's time limit is three times that, rounded up to ten
seconds (limit_seconds).  `found_by` says whether a test that existed before the catalogue kills the entry ("existing":
all 24, as run on the MI355X), or only a directed test that was added for it ("new": none).  Two killers were added all
the same, as the narrow and deterministic ones: test_the_diagonal_word_is_not_negated and
test_dense_dev_form_writes_every_tile_over_a_sentinel.
"""
import math

_MM = "tests/test_gpu_matmul.py::"
_CV = "tests/test_gpu_conv2d.py::"
_PM = "tests/test_gpu_polymul.py::"
_KS = "tests/test_gpu_ks_shapes.py::"
_PK = "tests/test_gpu_pk_encrypt.py::"
_TS = "tests/test_gpu_trlwe_switch.py::"
_CM = "tests/test_gpu_cmux.py::"
_DE = "tests/test_gpu_decrypt.py::"
_PE = "tests/test_gpu_packed_encrypt.py::"

_DENSE = _MM + "test_dense_equals_the_model[SECURITY_80_BIT]"
_KS_ID = _KS + "test_identity_key_switch_and_unpack_equal_the_model"
_KS_PACK = _KS + "test_pack_and_table_key_switch_equal_the_models"
_SWITCH = _TS + "test_switch_equals_the_model"
_CMUX = _CM + "test_cmux_equals_the_model"
_TRGSW = _CM + "test_generated_selectors_equal_the_model[6-3-1-random]"
_EXT = _CM + "test_external_product_is_the_call_without_d0"


def _m(name, file, kernel, what, killers, controls, seconds, found_by="existing"):
    return {"name": name, "file": file, "kernel": kernel, "what": what, "killers": tuple(killers), "controls": tuple(controls),
            "seconds": seconds, "found_by": found_by}


MUTANTS = (
    # ---- the shared int8 GEMM ------------------------------------------------------------------------------------------------
    _m("mm_plane_carry", "matmul.hpp", "mm_planes",
       "The balanced byte planes are formed without the carry out of plane 1 into plane 2: wrong on words whose byte 1 is >= 0x80.",
       [_DENSE], [_MM + "test_matmul_error_codes"], 4.2),
    _m("mm_a_tail", "matmul.hpp", "k_tlwe_matmul",
       "load_a, unaligned path: the last valid weight byte of a partial fragment reads as 0; shows when cols % 16 != 0.",
       [_DENSE], [_MM + "test_dense_accumulator_bound_at_65536_columns"], 4.1),
    _m("mm_a_sign", "matmul.hpp", "k_tlwe_matmul",
       "load_a, unaligned path: a weight byte is widened with its sign, so a negative weight smears into the higher bytes of its dword.",
       [_DENSE], [_MM + "test_dense_accumulator_bound_at_65536_columns"], 4.3),
    _m("mm_xcd_rem", "matmul.hpp", "k_tlwe_matmul",
       "The virtual workgroup index leaves out min(xcd, rem): when the workgroup count is no multiple of 8 some tiles are "
       "computed twice and others never (every index stays below the count).  (The host-form dense test fails on it too, "
       "on what the staging buffer held; the killer fills the output with a sentinel first.)",
       [_MM + "test_dense_dev_form_writes_every_tile_over_a_sentinel"], [_MM + "test_matmul_error_codes"], 3.9),
    _m("mm_toeplitz_wrap", "matmul.hpp", "MmToeplitz::setup",
       "The wrapped half of the packed form's extension holds the planes of ~a where 0 - a was meant: one LSB per negated word.",
       [_MM + "test_packed_without_key_switch_equals_the_model[SECURITY_128_BIT]"], [_DENSE], 4.2),
    _m("mm_conv_pad", "matmul.hpp", "MmConv::fetch16",
       "Any-in_c path: a padding tap keeps the stand-in word it loaded (word 0 of the image) instead of zero.",
       [_CV + "test_padding_reads_zero_not_a_neighbour"], [_CV + "test_one_by_one_filter_is_the_dense_form_on_the_same_memory"], 3.7),
    _m("mm_conv_stride", "matmul.hpp", "MmConv::setup",
       "The position's first input column is taken with stride_h; shows when the two strides differ (the ix < in_w guard stands).",
       [_CV + "test_every_path_of_the_loader_equals_the_model[SECURITY_80_BIT]"], [_CV + "test_padding_reads_zero_not_a_neighbour"], 3.9),
    _m("mm_nega_wrap", "matmul.hpp", "MmNegacyclic::fetch16",
       "A wrapped term of the negacyclic product is ~v where 0 - v was meant.  (Every word-for-word test of the file "
       "reaches a wrapped term -- the zeros-in, zeros-out line of the error-code test fails too -- so the control is the "
       "end-to-end rotation, which the defect reaches but whose decoding margin of 1/8 one LSB cannot move: wrong words, no more.)",
       [_PM + "test_monomials_rotate_with_the_negacyclic_sign"], [_PM + "test_slot_rotation_end_to_end"], 4.4),
    _m("mm_polymul_bias", "matmul.hpp", "k_polymul_bias",
       "Every output ciphertext past the first group takes bias row 0; shows with two or more groups and two or more rows.",
       [_PM + "test_dense_weights_row_tail_second_row_block_and_bias"], [_PM + "test_accumulator_bound_at_64_polynomials[bound]"], 4.3),
    # ---- the key switch family -----------------------------------------------------------------------------------------------
    _m("ks_plane_borrow", "key_switch_mfma.hpp", "ks_plane_byte (k_ksk_planes, k_pack_planes, k_pke_planes)",
       "A key word's plane p is its plain byte p, with no borrow from the planes below: wrong wherever a lower byte is >= 0x80.",
       [_KS_ID + "[n1_b2_t6-mfma]", _KS_PACK + "[n15_b2_t9]", _PK + "test_words_equal_the_model[255-32-32-0-0.0]"],
       [_KS_ID + "[n3_b10_t3-generic]"], 4.3),
    _m("ks_round_split", "key_switch.hpp", "k_key_switch_split",
       "The rounding addend of the split kernel alone is halved: a quarter of the words decompose into other digits.",
       [_KS_ID + "[n3_b10_t3-split]"], [_KS_ID + "[n3_b10_t3-generic]"], 3.8),
    _m("ks_round_digits", "key_switch.hpp", "k_ks_digits",
       "The rounding addend of the sliced kernel's digit pass alone is halved.",
       [_KS_ID + "[n62_b4_t7-sliced]"], [_KS_ID + "[n62_b4_t7-generic]"], 3.7),
    # ---- the TRLWE key switch ------------------------------------------------------------------------------------------------
    _m("ts_psi_sign_b", "trlwe_switch.hpp", "k_trlwe_switch_digits",
       "psi_k negates the coefficients of a that wrap but not those of b; shows for k != 1.",
       [_SWITCH + "[513-4-6-3]"], [_SWITCH + "[1-4-6-3]"], 3.8),
    _m("ts_off_top", "trlwe_switch.hpp", "k_trlwe_switch_digits",
       "The decomposition offset leaves out the top digit's half base: the top digit is off by B/2.",
       [_SWITCH + "[1-4-6-3]"], [_TS + "test_generated_bodies_equal_the_model[513-1-32-2.220446049250313e-16-False]"], 3.9),
    _m("ts_rot3", "trlwe_switch.hpp", "k_trlwe_switch_digits",
       "The exchange of the `rot & 2` stage is skipped on the lanes whose rotation is 3: their four slots stay out of order.",
       [_SWITCH + "[1-4-6-3]"], [_TS + "test_generated_bodies_equal_the_model[513-1-32-2.220446049250313e-16-False]"], 4.3),
    _m("ts_gadget_hi", "trlwe_switch.hpp", "k_gen_trlwe_switch_key",
       "The gadget coefficient of the high half of a key row is read at the low half's index.",
       [_TS + "test_generated_bodies_equal_the_model[513-1-32-2.220446049250313e-16-False]"], [_SWITCH + "[1-4-6-3]"], 3.9),
    # ---- the packed CMUX -----------------------------------------------------------------------------------------------------
    _m("cmux_rnd_b", "cmux.hpp", "k_cmux_digits",
       "The b half (c = 1) is decomposed with rnd = 0; the reference-digits mode, where rnd is 0 anyway, is not touched.",
       [_CMUX + "[6-3-False]"], [_CMUX + "[6-3-True]"], 4.9),
    _m("cmux_addend_w", "cmux.hpp", "k_cmux_addend",
       "The .w word of every quad of d0 is not added.",
       [_CMUX + "[6-3-False]"], [_EXT], 4.8),
    _m("trgsw_row_t", "cmux.hpp", "k_encrypt_trgsw",
       "on_a = row <= t: row t, the first of the b block, carries its gadget on the a half.",
       [_TRGSW], [_EXT], 4.0),
    # ---- unpack, decrypt and packed encryption -------------------------------------------------------------------------------
    _m("unpack_diag", "unpack.hpp", "k_unpack_extract",
       "The extraction negates at i >= j: the diagonal word a[0] is negated as well.  (The tests that existed notice it "
       "only where the input is a real ciphertext -- test_client_packed_inputs_feed_a_gate, test_gate_pack_unpack_gate_on_the_device -- "
       "and there first in the decryption; the word-for-word unpack inputs against the oracle and in ks_shapes plant 0 at a[0], "
       "and Torus::MAX - 0 rounds to the digits of 0, so they pass.  The directed test is the narrow word-for-word killer.)",
       ["tests/test_gpu_unpack.py::test_the_diagonal_word_is_not_negated", "tests/test_gpu_unpack.py::test_client_packed_inputs_feed_a_gate"],
       ["tests/test_gpu_unpack.py::test_unpack_error_codes"], 5.2),
    _m("dec_tail_bit", "decrypt.hpp", "k_lwe_phase",
       "The tail word of a row is masked with bit 0 of the lane's key register instead of the bit the loop has reached; "
       "shows when n >= 64 and n % 64 != 0.",
       [_DE + "test_lwe_phases_toy_sets[n65-5]"], [_DE + "test_lwe_phases_toy_sets[n33-5]"], 4.8),
    _m("dec_wrap", "decrypt.hpp", "k_trlwe_phase",
       "The negated half of the extension holds ~w where 0 - w was meant.",
       [_DE + "test_packed_phases[1]"], [_DE + "test_lwe_phases_toy_sets[n33-5]"], 4.3),
    _m("trlwe_group_hi", "trlwe_encrypt.hpp", "k_trlwe_rows, k_expand_trlwe",
       "The high word of the 64-bit group index is taken as 0; shows only when first_group + m >= 2^32.",
       [_PE + "test_zero_alpha_is_equality[random]"], [_PE + "test_words_equal_the_model[1-first0]"], 4.2),
    _m("trgsw_index_hi", "cmux.hpp", "k_encrypt_trgsw",
       "The high word of the 64-bit row index is taken as 0; shows only when first_index + r >= 2^32.",
       [_TRGSW], [_EXT], 4.6),
)

NAMES = tuple(m["name"] for m in MUTANTS)


def limit_seconds(seconds):
    """a child's time limit: three times the product library's time, rounded up to ten seconds"""
    return int(math.ceil(3.0 * seconds / 10.0)) * 10


# the `none` case: every killer on the catalogue library with no defect selected
NONE_SECONDS = 6.7


def all_killers():
    seen = []
    for m in MUTANTS:
        for k in m["killers"]:
            if k not in seen:
                seen.append(k)
    return tuple(seen)
