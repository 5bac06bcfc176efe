"""Symmetric encryption in the keyed format of include/tfhe_hip.h ("symmetric encryption"), on the CPU: the package's
numpy form (rs_tfhe_amd.seeded.symmetric_rows behind SecretKey.encrypt_*, PublicKeyLv0.new and
ProxyReencryptionKey.new_symmetric with rng_key=) against the term-by-term model of tests/sym_encrypt_model.py, the
decryption of every row, the reference's own re-encryption bar on the oracle, four deliberately wrong models, and the
borderline cap tests/test_gpu_sym_encrypt.py relies on.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import keygen_model as KM
import sym_encrypt_model as SM
from rs_tfhe_amd import _capi, proxy_reenc as PR, seeded as S
from rs_tfhe_amd.client import SecretKey, f64_to_torus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, SEED = SM.K, SM.SEED
SHAPE = SM.SHAPES[0]


def _sk(shape=SHAPE):
    p = KM.shape_params(shape)
    return p, KM.secret_key(p)


def _phase_error(sk, rows, plain):
    return (sk.phase(rows) - np.asarray(plain, np.uint32)).view(np.int32).astype(np.float64) / 2.0 ** 32


def test_domain_words_are_the_headers():
    assert SM.TLWE == S.DOMAINS_SYM_TLWE == (int.from_bytes(b"EWL", "big"), int.from_bytes(b"EWN", "big"))
    assert SM.PK == S.DOMAINS_SYM_PK == (int.from_bytes(b"PKM", "big"), int.from_bytes(b"PKZ", "big"))
    assert SM.RK == S.DOMAINS_SYM_RK == (int.from_bytes(b"RKM", "big"), int.from_bytes(b"RKS", "big"))
    words = [S.DOMAIN_KSK, S.DOMAIN_BSK, S.DOMAIN_SEED, PR.DOMAIN_PKE_SEL, PR.DOMAIN_PKE_NOISE, PR.DOMAIN_RKE_SEL,
             PR.DOMAIN_RKE_NOISE, *SM.TLWE, *SM.PK, *SM.RK]
    assert len(set(words)) == len(words)


@pytest.mark.parametrize("n", [16, 33, 48, 1279])
@pytest.mark.parametrize("first_index", SM.FIRST)
def test_ewl_masks_are_the_seeded_tlwe_masks(n, first_index):
    rows = SM.PM.row_indices(first_index, 9)
    assert np.array_equal(SM.masks(SEED, rows, n, SM.TLWE[0]), S.tlwe_masks(SEED, first_index, 9, n))


@pytest.mark.parametrize("shape", SM.SHAPES, ids=str)
@pytest.mark.parametrize("first_index", SM.FIRST)
def test_bulk_cpu_form_equals_the_model(shape, first_index):
    p, sk = _sk(shape)
    pt = np.random.default_rng(p.n).uniform(-0.5, 0.5, 37)
    want, _ = SM.bulk(sk.key_lv0, f64_to_torus(pt), first_index, p.alpha_lv0)
    got = sk.encrypt_f64(pt, rng_key=K, first_index=first_index, mask_seed=SEED)
    assert np.array_equal(got, want)
    sc = sk.encrypt_f64_seeded(pt, mask_seed=SEED, first_index=first_index, rng_key=K)
    assert np.array_equal(sc.bodies, want[:, -1]) and np.array_equal(sc.expand(), want)
    # every row decrypts
    assert np.abs(_phase_error(sk, got, f64_to_torus(pt))).max() < 6 * p.alpha_lv0
    bits = np.random.default_rng(p.n + 1).integers(0, 2, 37).astype(bool)
    assert np.array_equal(sk.decrypt_bool(sk.encrypt_bool(bits, rng_key=K, first_index=first_index)), bits)
    msgs = np.arange(37) % 4
    ct = sk.encrypt_lwe_message(msgs, 4, rng_key=K, first_index=first_index, mask_seed=SEED)
    assert np.array_equal(sk.decrypt_lwe_message(ct, 4), msgs)
    assert np.array_equal(sk.encrypt_lwe_message_seeded(msgs, 4, SEED, first_index, rng_key=K).expand(), ct)
    assert np.array_equal(sk.encrypt_bool_seeded(bits, SEED, first_index, rng_key=K).expand(),
                          sk.encrypt_bool(bits, rng_key=K, first_index=first_index, mask_seed=SEED))


def test_zero_alpha_has_no_noise():
    p, sk = _sk()
    pt = np.random.default_rng(5).uniform(-0.5, 0.5, 20)
    got = sk.encrypt_f64(pt, alpha=0.0, rng_key=K, mask_seed=SEED)
    assert np.array_equal(sk.phase(got), f64_to_torus(pt))


def test_seed_with_the_keyed_format_is_refused():
    p, sk = _sk()
    for kw in ({"rng_key": K}, {"device": 0}):
        with pytest.raises(ValueError):
            sk.encrypt_f64([0.1], seed=1, **kw)
        with pytest.raises(ValueError):
            sk.encrypt_bool([1], seed=1, **kw)
        with pytest.raises(ValueError):
            sk.encrypt_lwe_message([1], 4, seed=1, **kw)
        with pytest.raises(ValueError):
            sk.encrypt_f64_seeded([0.1], seed=1, **kw)
        with pytest.raises(ValueError):
            PR.PublicKeyLv0.new(sk, seed=1, **kw)
        with pytest.raises(ValueError):
            PR.ProxyReencryptionKey.new_symmetric(sk, sk, seed=1, **kw)
    with pytest.raises(ValueError):
        sk.encrypt_f64([0.1], rng_key=b"short")
    with pytest.raises(ValueError):
        sk.encrypt_f64([0.1, 0.2], rng_key=K, first_index=(1 << 64) - 1)
    # calls without the new arguments give what they gave before
    assert np.array_equal(sk.encrypt_f64([0.1, 0.2], 3), sk.encrypt_f64([0.1, 0.2], seed=3))


@pytest.mark.parametrize("size", [1, 66])
def test_public_key_cpu_form_equals_the_model(size):
    p, sk = _sk()
    pk = PR.PublicKeyLv0.new_with_params(sk, size, p.alpha_lv0, rng_key=K)
    want, _ = SM.public_key(sk.key_lv0, size, p.alpha_lv0)
    assert np.array_equal(pk.encryptions, want)
    assert np.abs(_phase_error(sk, pk.encryptions, 0)).max() < 6 * p.alpha_lv0
    if size == 66:
        assert np.array_equal(PR.PublicKeyLv0.new(sk, rng_key=K).encryptions, want)
        bits = np.random.default_rng(3).integers(0, 2, 100).astype(bool)
        assert np.array_equal(sk.decrypt_bool(pk.encrypt_bool(bits, p.alpha_lv0, rng_key=K)), bits)


def test_reenc_key_cpu_form_equals_the_model():
    p, to = _sk()
    frm = SecretKey.new(p, 77)
    key = PR.ProxyReencryptionKey.new_symmetric(frm, to, rng_key=K)
    want, _ = SM.reenc_key(p, frm.key_lv0, to.key_lv0, p.alpha_lv0)
    assert np.array_equal(key.key_encryptions, want)
    shaped = key.key_encryptions.reshape(p.n, p.iks_t, p.base, p.n + 1)
    assert not shaped[:, :, 0, :].any() and shaped[:, :, 1:, :].any(axis=-1).all()
    # every live row decrypts to its plaintext under key_to
    rows = np.arange(len(want))
    live = rows % p.base != 0
    err = _phase_error(to, want[live], SM.PM.reenc_plaintexts(p, frm.key_lv0)[live])
    assert np.abs(err).max() < 6 * p.alpha_lv0


def test_symmetric_key_reencrypts_on_the_oracle_at_the_references_bar(O):
    """proxy_reenc.rs:629-634: more than 90 % of 256 bits decode after the re-encryption"""
    from rs_tfhe_amd.params import SECURITY_128_BIT as P

    alice, bob = SecretKey.new(P, 501), SecretKey.new(P, 502)
    key = PR.ProxyReencryptionKey.new_symmetric(alice, bob, rng_key=K)
    bits = np.random.default_rng(503).integers(0, 2, 256).astype(bool)
    cts = alice.encrypt_bool(bits, rng_key=K, first_index=0)
    out = O.reencrypt_tlwe_lv0(O.SECURITY_128_BIT, key.key_encryptions, cts)
    good = int((bob.decrypt_bool(out) == bits).sum())
    print(f"SYMENCRYPT reencrypt on the oracle: {good} of 256 decode")
    assert good > 0.90 * 256


def _checks(words, sk, plain, alpha):
    """what a correct bulk batch satisfies: it decrypts, and no noise word repeats between rows"""
    err = _phase_error(sk, words, plain)
    noise = (sk.phase(words) - np.asarray(plain, np.uint32))
    return bool(np.abs(err).max() < 6 * alpha) and len(np.unique(noise)) > len(noise) // 2


@pytest.mark.parametrize("alter", ["noise_from_mask_domain", "no_row", "ignore_high", "k0_not_zero"])
def test_an_altered_model_fails_its_check(alter):
    p, sk = _sk()
    if alter == "k0_not_zero":
        frm = SecretKey.new(p, 77)
        right, _ = SM.reenc_key(p, frm.key_lv0, sk.key_lv0, p.alpha_lv0)
        wrong, _ = SM.reenc_key(p, frm.key_lv0, sk.key_lv0, p.alpha_lv0, alter=alter)
        k0 = np.arange(len(right)) % p.base == 0
        assert not right[k0].any() and wrong[k0].any(axis=1).all()
        assert np.array_equal(right[~k0], wrong[~k0])
        return
    plain = SM.plaintexts(64, 1)
    first = SM.HIGH if alter == "ignore_high" else 0
    right, _ = SM.bulk(sk.key_lv0, plain, first, p.alpha_lv0)
    wrong, _ = SM.bulk(sk.key_lv0, plain, first, p.alpha_lv0, alter=alter)
    cpu = sk.encrypt_f64(np.zeros(64), rng_key=K, first_index=first, mask_seed=SEED)
    with np.errstate(over="ignore"):
        cpu[:, -1] += plain
    assert np.array_equal(cpu, right) and not np.array_equal(cpu, wrong)
    assert _checks(right, sk, plain, p.alpha_lv0)
    if alter == "noise_from_mask_domain":
        # the noise words of the wrong model are the public mask stream's: whoever holds S strips the noise.  Under the
        # test's K != S the words differ from the right ones on (nearly) every row
        assert (wrong[:, -1] != right[:, -1]).mean() > 0.9
        same_key, _ = SM.bulk(sk.key_lv0, plain, first, p.alpha_lv0, mask_seed=K, alter=alter)
        assert np.array_equal(SM.noise(K, SM.PM.row_indices(first, 64), p.alpha_lv0, SM.TLWE[0]).words,
                              sk.phase(same_key) - plain)
    elif alter == "no_row":
        assert (wrong[:, :-1] == wrong[0, :-1]).all() and not _checks(wrong, sk, plain, p.alpha_lv0)
    else:  # rows past 2^32 repeat the rows 2^32 before them
        low, _ = SM.bulk(sk.key_lv0, plain[5:], 0, p.alpha_lv0)  # (row 5 of the batch is index 2^32)
        assert np.array_equal(wrong[5:], low) and not (right[5:] == low).any(axis=1).any()


def test_fixed_key_keeps_the_gpu_cases_within_the_borderline_cap():
    """What tests/test_gpu_sym_encrypt.py relies on: at most 16 borderline noise samples per case under K."""
    for first in SM.FIRST:
        for count in SM.COUNTS:
            assert int(SM.noise(K, SM.PM.row_indices(first, count), SM.ALPHA, SM.TLWE[1]).border.sum()) <= KM.MAX_MISMATCHES
    for size in (1, 66, 8192):
        assert int(SM.noise(K, np.arange(size), SM.ALPHA, SM.PK[1]).border.sum()) <= KM.MAX_MISMATCHES
    p = KM.shape_params(SHAPE)
    assert int(SM.noise(K, np.arange(p.n * p.iks_t * p.base), SM.ALPHA, SM.RK[1]).border.sum()) <= KM.MAX_MISMATCHES


def test_exports_refuse_a_null_handle():
    lib = _capi.lib()
    assert lib.tfhe_hip_batch_encrypt(None, None, None, 0, 0.0, None, None, 0, None, None) == _capi.EINVAL
    assert lib.tfhe_hip_batch_encrypt_dev(None, None, None, 0, 0.0, None, None, 0, None, None, None) == _capi.EINVAL
    assert lib.tfhe_hip_gen_public_key(None, None, 1, 0.0, None, None) == _capi.EINVAL
    assert lib.tfhe_hip_gen_reenc_key_symmetric(None, None, None, 0.0, None, None) == _capi.EINVAL


def build_cpp_sym_encrypt(outdir):
    """tests/cpp/test_sym_encrypt.cpp, built as test_pk_encrypt_host.build_cpp_pk_encrypt builds its program."""
    exe = os.path.join(outdir, "test_sym_encrypt")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_sym_encrypt.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-fopenmp", "-pthread"])
    return exe


def test_cpp_sym_encrypt_program_builds(tmp_path):
    """The C++ mirror's encrypt_batch / generate / generate_symmetric program compiles and links against the header and
    the library (run on the GPU by tests/test_gpu_sym_encrypt.py)."""
    assert os.path.exists(build_cpp_sym_encrypt(str(tmp_path)))
