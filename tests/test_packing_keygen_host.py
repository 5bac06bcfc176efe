"""The packing-key generator's model (tests/packing_keygen_model.py) and its checkers proven on the CPU, no device:
the mask seed is not the compressed cloud key's, `make_packing_key(rng=K)` is the model word for word, the recovered noise
passes noise_report, every altered generator (noise from the mask's stream, a nonce without the row, g1 := g0, the gadget
on coefficient 1, g_{l+1} for g_l) FAILS its check, one flipped LSB fails the word comparison, the fixed generator key
keeps every shape the GPU test uses within the cap of 16 borderline samples, the two new exports refuse a NULL handle,
and the C++ program builds."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import keygen_model as KM
import packing_keygen_model as PM
from rs_tfhe_amd import _capi
from rs_tfhe_amd import packing as PK
from rs_tfhe_amd import seeded as S
from rs_tfhe_amd.params import N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = KM.GEN_KEY
ALPHA = KM.ALPHA_BSK  # 2e-8
_CACHE = {}


def _case(shape=KM.SHAPES[0]):
    """(params, secret key, model) at alpha 2e-8 under the fixed generator key"""
    if shape not in _CACHE:
        p = KM.shape_params(shape)
        sk = KM.secret_key(p)
        _CACHE[shape] = (p, sk, PM.model(p, sk.key_lv0, sk.key_lv1, K, ALPHA))
    return _CACHE[shape]


def _report(p, sk, seed, bodies):
    e, a = PM.recover_noise(p, sk.key_lv0, sk.key_lv1, seed, bodies)
    return KM.noise_report(e, ALPHA, KM.REF_SEED, mask=a), e


def test_mask_seed_is_not_the_compressed_cloud_keys():
    """Stream 26, not 20: one K gives two different public seeds; and the seed is the keystream position the header names."""
    assert PM.mask_seed(K) != S.mask_seed_of(K)
    assert PM.mask_seed(K) == S.chacha20_block(K, 0, 0, 26, 0x444553)[:8].astype("<u4").tobytes()
    assert PK.mask_seed_of(K) == PM.mask_seed(K)
    assert PM.mask_seed(bytes(32)) != PM.mask_seed(K)


@pytest.mark.parametrize("shape", [KM.SHAPES[0], KM.SHAPES[2], KM.SHAPES[4], PM.WIDE_SHAPE], ids=str)
def test_make_packing_key_with_a_generator_key_equals_the_model(shape):
    p, sk, m = _case(shape)
    pk = PK.make_packing_key(p, sk.key_lv0, sk.key_lv1, rng=K, alpha=ALPHA)
    assert pk.mask_seed == m.mask_seed
    assert np.array_equal(pk.bodies, m.bodies)
    assert sk.packing_key(rng_key=K, alpha=ALPHA).mask_seed == m.mask_seed
    # the noise sits where the header says: block 2 lane + h, pair m -> lane + 64 (4h + m) and + 512
    w = S.chacha20_block(K, 2 * 5 + 1, 3 % (p.n * p.iks_t), 25, 0x504B53)
    g0, g1 = S.gauss2(w[None, 8:12], ALPHA)
    row = m.e.words[3 % (p.n * p.iks_t)]
    assert row[5 + 64 * (4 + 2)] == S.f64_to_torus(g0)[0] and row[5 + 64 * (4 + 2) + 512] == S.f64_to_torus(g1)[0]
    # ... and the seeds of today's other inputs are untouched by the new case
    a, b = (PK.make_packing_key(p, sk.key_lv0, sk.key_lv1, rng=4, alpha=ALPHA) for _ in range(2))
    assert a.mask_seed == b.mask_seed != m.mask_seed and np.array_equal(a.bodies, b.bodies)
    with pytest.raises(ValueError):
        PK.make_packing_key(p, sk.key_lv0, sk.key_lv1, rng=K[:31])


def test_recovered_noise_is_the_models_and_passes_the_report():
    p, sk, m = _case()
    rep, e = _report(p, sk, m.mask_seed, m.bodies)
    assert np.array_equal(e.view(np.uint32), m.e.words)
    KM.check_report(rep, 5.0, "packing key noise")
    assert rep["rows_distinct"] and rep["M"] == p.n * p.iks_t * N and "mask_corr" in rep
    assert KM.compare_words(m.bodies, m.bodies, m.border) == (0, int(m.border.sum()))


def _altered(**alter):
    p, sk, m = _case()
    bad = PM.model(p, sk.key_lv0, sk.key_lv1, K, ALPHA, **alter)
    with pytest.raises(AssertionError, match="away from any borderline"):
        KM.compare_words(bad.bodies, m.bodies, m.border)
    return _report(p, sk, bad.mask_seed, bad.bodies)[0]


def test_noise_from_the_masks_stream_fails_the_word_comparison():
    """Stream 24 under K is as Gaussian as stream 25: only the comparison with the model can tell (and does)."""
    rep = _altered(stream=PM.MASK_STREAM)
    assert not KM.failures(rep, 5.0)


def test_a_noise_nonce_without_the_row_fails_the_report():
    bad = KM.failures(_altered(no_row=True), 5.0)
    assert "rows_distinct" in bad and "row_corr" in bad


def test_g1_equal_to_g0_fails_the_report():
    bad = KM.failures(_altered(same_pair=True), 5.0)
    assert "pair_corr" in bad and not {"mean", "std", "kurtosis", "tail", "row_std"} & set(bad)


def test_the_gadget_on_coefficient_one_fails_the_report():
    """the recovery subtracts s0[i] g_l from coefficient 0 and finds it on coefficient 1: two words a row of at least
    2^14 where sigma is 86"""
    assert "std" in KM.failures(_altered(gadget_at=1), 5.0)


def test_the_next_digits_gadget_fails_the_report():
    bad = KM.failures(_altered(next_digit=True), 5.0)
    assert "std" in bad and "row_std" in bad


def test_word_comparison_fails_on_one_lsb():
    _, _, m = _case()
    r = tuple(np.argwhere(~m.border)[54321])
    got = m.bodies.copy()
    got[r] ^= 1
    with pytest.raises(AssertionError, match="away from any borderline"):
        KM.compare_words(got, m.bodies, m.border)


@pytest.mark.parametrize("shape", PM.SHAPES, ids=str)
def test_the_fixed_key_stays_within_the_cap(shape):
    """At most 16 borderline samples a key under KM.GEN_KEY at alpha 2e-8 on every shape the GPU test uses: a condition
    the chosen inputs meet, so that compare_words' cap of 16 differing words can never be what lets a key pass."""
    n, _, _, _, t = shape
    e = PM.noise(K, np.arange(n * t), ALPHA)
    differ = e.words != e.ld_words
    assert not (differ & ~e.border).any()
    print("PACKKEYGEN_HOST", shape, "borderline", int(e.border.sum()), "f64 != long double", int(differ.sum()))
    assert int(e.border.sum()) <= KM.MAX_MISMATCHES


def test_the_new_exports_refuse_a_null_handle():
    lib = _capi.lib()
    for fn in ("gen_packing_key", "pool_gen_packing_key"):
        assert "tfhe_hip_" + fn in _capi.SIGNATURES, fn
        f = getattr(lib, "tfhe_hip_" + fn)
        args = [0 if t in (ctypes.c_size_t, ctypes.c_int) else 0.0 if t is ctypes.c_double else None for t in f.argtypes]
        assert f(*args) == _capi.EINVAL, fn


def build_cpp_packing_keygen(outdir):
    """tests/cpp/test_packing_keygen.cpp, built as test_unpack_host.build_cpp_unpack builds its program, without the
    oracle library."""
    exe = os.path.join(outdir, "test_packing_keygen")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_packing_keygen.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-fopenmp", "-pthread"])
    return exe


def test_cpp_packing_keygen_program_builds(tmp_path):
    """The C++ mirror's PackingKey::generate program compiles and links against the header and the library (run on the
    GPU by tests/test_gpu_packing_keygen.py)."""
    assert os.path.exists(build_cpp_packing_keygen(str(tmp_path)))
