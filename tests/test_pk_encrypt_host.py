"""Public-key encryption and the asymmetric re-encryption key in the keyed format of include/tfhe_hip.h, on the CPU, no
device: the selector bits sit at the keystream positions the header states, the package's CPU form
(proxy_reenc.encrypt_rows: a +-1 / 0 matrix times the key in f64) equals the term-by-term model of
tests/pk_encrypt_model.py word for word, the selectors are fair and differ from row to row, `seed=` calls give the words
they gave before the format existed, ciphertexts decrypt, the key has the reference layout, the fixed generator key keeps
every case the GPU test uses within the cap of 16 borderline noise samples, the new exports refuse a NULL handle, and the
C++ program builds."""
import os
import subprocess

import numpy as np
import pytest

import keygen_model as KM
import pk_encrypt_model as PM
from rs_tfhe_amd import _capi
from rs_tfhe_amd import proxy_reenc as PR
from rs_tfhe_amd import seeded as S
from rs_tfhe_amd.client import SecretKey, f64_to_torus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = PM.K


def _pk(n=33, size=66):
    p = PM.params(n)
    return p, KM.secret_key(p), PR.PublicKeyLv0(p, PM.public_key(n, size))


def test_selector_bits_sit_at_the_stated_keystream_positions():
    """Three entries by hand: (row, entry) -> word e / 16 -> block word / 16, word % 16; bits 2 (e % 16) and + 1."""
    size = 600
    for g, e in ((0, 0), (7, 37), (PM.HIGH + 9, 531)):  # the last: a row past 2^32, block 2 of its stream
        word = e // 16
        w = int(S.chacha20_block(K, word // 16, g & 0xFFFFFFFF, g >> 32, 0x504B45)[word % 16])
        take, sign = (w >> (2 * (e % 16))) & 1, (w >> (2 * (e % 16) + 1)) & 1
        want = (-1.0 if sign else 1.0) if take else 0.0
        assert PR.selectors(K, [g], size, PR.DOMAIN_PKE_SEL)[0, e] == want
        t, s = PM.selector_bits(K, [g], size, PM.PKE[0])
        assert (int(t[0, e]), int(s[0, e])) == (take, sign)
    assert (PR.DOMAIN_PKE_SEL, PR.DOMAIN_PKE_NOISE) == PM.PKE == (int.from_bytes(b"PKE", "big"), int.from_bytes(b"PKN", "big"))
    assert (PR.DOMAIN_RKE_SEL, PR.DOMAIN_RKE_NOISE) == PM.RKE == (int.from_bytes(b"RKE", "big"), int.from_bytes(b"RKN", "big"))
    # the noise: g0 of gauss2 over words 0..3 of block 0 of the noise stream
    g0, _ = S.gauss2(S.chacha20_block(K, 0, 7, 0, 0x504B4E)[None, :4], 2e-5)
    assert PM.noise(K, [7], 2e-5, PM.PKE[1]).words[0] == S.f64_to_torus(g0)[0]


@pytest.mark.parametrize("size", [1, 33, 66])
@pytest.mark.parametrize("count,first_index", [(1, 0), (33, 0), (33, PM.HIGH)])
def test_cpu_form_equals_the_term_by_term_model(size, count, first_index):
    p, _, pk = _pk(33, size)
    pt = np.random.default_rng(size + count).uniform(-0.5, 0.5, count)
    for alpha in (0.0, 2e-5, 0.5):
        got = pk.encrypt_f64(pt, alpha, rng_key=K, first_index=first_index)
        want, _ = PM.encrypt(pk.encryptions, K, PM.row_indices(first_index, count), f64_to_torus(pt), alpha)
        assert got.shape == (count, p.n + 1) and np.array_equal(got, want), (size, count, first_index, alpha)
    if count == 33:  # a batch is its rows: the second half alone, at its own first index
        assert np.array_equal(pk.encrypt_f64(pt[16:], 0.5, rng_key=K, first_index=first_index + 16), got[16:])
    assert np.array_equal(pk.encrypt_bool(pt > 0, 0.0, rng_key=K, first_index=first_index),
                          pk.encrypt_f64(np.where(pt > 0, 0.125, -0.125), 0.0, rng_key=K, first_index=first_index))


def test_adversarial_key_words_in_the_cpu_form():
    e = PM.adversarial_key(33, 66)
    got = PR.encrypt_rows(e, K, PM.row_indices(0, 33), np.zeros(33, np.uint32), 0.0, PM.PKE)
    assert np.array_equal(got, PM.encrypt(e, K, PM.row_indices(0, 33), np.zeros(33, np.uint32), 0.0)[0])


def test_selectors_are_fair_and_rows_differ():
    """Shares of take and of sign within 5 standard errors of 1/2 (SE 1 / (2 sqrt(bits))); no two rows share selectors."""
    rows, size = 4096, 1400
    take, sign = PM.selector_bits(K, PM.row_indices(PM.HIGH - 2000, rows), size, PM.PKE[0])
    for name, bits in (("take", take), ("sign", sign), ("sign of the taken", sign[take])):
        se = (bits.mean() - 0.5) * 2.0 * np.sqrt(bits.size)
        assert abs(se) <= 5.0, (name, se)
    both = np.packbits(np.concatenate([take, sign], axis=1), axis=1)
    assert len(np.unique(both, axis=0)) == rows
    # and the two uses of one K do not share them either
    t2, _ = PM.selector_bits(K, PM.row_indices(PM.HIGH - 2000, 64), size, PM.RKE[0])
    assert not np.array_equal(t2, take[:64])


def test_seed_calls_give_the_words_they_gave_before():
    """numpy's generator behind `seed=`: checksums taken from the module as it was before rng_key / device existed."""
    p, sk, _ = _pk()
    pk = PR.PublicKeyLv0.new_with_params(sk, 66, p.alpha_lv0, seed=11)
    assert PM.checksum(pk.encryptions) == 10742119011826723
    assert PM.checksum(pk.encrypt_f64(np.linspace(-0.4, 0.4, 5), 2e-5, seed=12)) == 59264539813851
    assert PM.checksum(pk.encrypt_bool([1, 0, 1], 0.0, seed=14)) == 23252022767837
    key = PR.ProxyReencryptionKey.new_asymmetric(SecretKey.new(p, 77), pk, seed=13)
    assert PM.checksum(key.key_encryptions) == 2633430614171095572
    for kw in ({"rng_key": K}, {"device": 0}):
        with pytest.raises(ValueError):
            pk.encrypt_f64([0.1], 2e-5, seed=1, **kw)
        with pytest.raises(ValueError):
            PR.ProxyReencryptionKey.new_asymmetric(SecretKey.new(p, 77), pk, seed=1, **kw)
    with pytest.raises(ValueError):
        pk.encrypt_f64([0.1], 2e-5, rng_key=b"short")


def test_ciphertexts_decrypt_to_their_plaintexts():
    p, sk, pk = _pk()
    bits = np.random.default_rng(3).integers(0, 2, 200).astype(bool)
    assert np.array_equal(sk.decrypt_bool(pk.encrypt_bool(bits, p.alpha_lv0, rng_key=K, first_index=5)), bits)
    pt = np.random.default_rng(4).uniform(-0.45, 0.45, 200)
    err = (sk.phase(pk.encrypt_f64(pt, p.alpha_lv0, rng_key=K)) - f64_to_torus(pt)).view(np.int32) / 2.0 ** 32
    assert np.abs(err).max() < 6 * p.alpha_lv0 * np.sqrt(66 / 2 + 1) + 1e-9


def test_reenc_key_cpu_form_layout_and_model():
    p, _, pk = _pk()
    frm = SecretKey.new(p, 77)
    key = PR.ProxyReencryptionKey.new_asymmetric(frm, pk, rng_key=K)
    want, _ = PM.reenc_key(p, pk.encryptions, frm.key_lv0, K, p.alpha_lv0)
    assert np.array_equal(key.key_encryptions, want)
    shaped = key.key_encryptions.reshape(p.n, p.iks_t, p.base, p.n + 1)
    assert not shaped[:, :, 0, :].any() and shaped[:, :, 1:, :].any(axis=-1).all()
    # row base t i + base j + k is an encryption of k key_from[i] / 2^((j+1) basebit) under the public key's secret key
    sk = KM.secret_key(p)
    i, j, k = 5, 2, 3
    row = shaped[i, j, k]
    msg = f64_to_torus(((k * int(frm.key_lv0[i])) & 0xFFFFFFFF) / 2.0 ** ((j + 1) * p.basebit))
    err = (sk.phase(row[None, :]) - msg).view(np.int32)[0] / 2.0 ** 32
    assert abs(err) < 6 * p.alpha_lv0 * np.sqrt(66 / 2 + 1) + 1e-9
    # the plaintexts are ProxyReencryptionKey._plaintexts through f64_to_torus
    assert np.array_equal(PM.reenc_plaintexts(p, frm.key_lv0),
                          f64_to_torus(PR.ProxyReencryptionKey._plaintexts(frm.key_lv0, p.basebit, p.iks_t)).reshape(-1))


def test_fixed_key_keeps_the_gpu_cases_within_the_borderline_cap():
    """What tests/test_gpu_pk_encrypt.py relies on: at most 16 borderline noise samples per case under K."""
    for n, size, count, first_index, alpha in PM.CASES:
        assert int(PM.noise(K, PM.row_indices(first_index, count), alpha, PM.PKE[1]).border.sum()) <= KM.MAX_MISMATCHES
    from rs_tfhe_amd.params import SECURITY_128_BIT as P

    for p in (PM.params(33), P):
        rows = np.arange(p.n * p.iks_t * p.base, dtype=np.uint64)
        assert int(PM.noise(K, rows, p.alpha_lv0, PM.RKE[1]).border.sum()) <= KM.MAX_MISMATCHES


def test_exports_refuse_a_null_handle():
    lib = _capi.lib()
    assert lib.tfhe_hip_public_key_is_loaded(None) == 0
    assert lib.tfhe_hip_load_public_key(None, None, 1) == _capi.EINVAL
    assert lib.tfhe_hip_batch_pk_encrypt(None, None, 0, 0.0, None, 0, None) == _capi.EINVAL
    assert lib.tfhe_hip_batch_pk_encrypt_dev(None, None, 0, 0.0, None, 0, None, None) == _capi.EINVAL
    assert lib.tfhe_hip_gen_reenc_key_asymmetric(None, None, 0.0, None, None) == _capi.EINVAL


def build_cpp_pk_encrypt(outdir):
    """tests/cpp/test_pk_encrypt.cpp, built as test_packing_keygen_host.build_cpp_packing_keygen builds its program."""
    exe = os.path.join(outdir, "test_pk_encrypt")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_pk_encrypt.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-fopenmp", "-pthread"])
    return exe


def test_cpp_pk_encrypt_program_builds(tmp_path):
    """The C++ mirror's encrypt_batch / generate_asymmetric program compiles and links against the header and the library
    (run on the GPU by tests/test_gpu_pk_encrypt.py)."""
    assert os.path.exists(build_cpp_pk_encrypt(str(tmp_path)))
