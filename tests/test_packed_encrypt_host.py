"""Packed TRLWE encryption in the keyed format of include/tfhe_hip.h ("packed encryption"), on the CPU: the package's
numpy form (rs_tfhe_amd.seeded.symmetric_trlwe_rows behind SecretKey.encrypt_packed_* with rng_key=) against the
term-by-term model of tests/packed_encrypt_model.py, the decryption of every slot, the seeded form, the argument checks,
the un-keyed route's unchanged words, four deliberately wrong models, and the conditions on the fixed generator key that
tests/test_gpu_packed_encrypt.py relies on.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import keygen_model as KM
import packed_encrypt_model as PM
from rs_tfhe_amd import _capi, seeded as S
from rs_tfhe_amd.client import SecretKey, f64_to_torus
from rs_tfhe_amd.params import N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, SEED = PM.K, PM.SEED
P = KM.shape_params(KM.SHAPES[2])  # a small n: the packed calls read key_lv1 only; alpha_lv1 = 2e-8 as SECURITY_128_BIT


def _sk(key="random") -> SecretKey:
    return SecretKey(P, np.zeros(P.n, np.uint32), PM.keys()[key])


def test_domain_words_are_the_headers():
    assert (PM.DOMAIN_MASK, PM.DOMAIN_NOISE) == S.DOMAINS_TRLWE == (int.from_bytes(b"ERL", "big"), int.from_bytes(b"ERN", "big"))
    from rs_tfhe_amd import proxy_reenc as PR

    words = [S.DOMAIN_KSK, S.DOMAIN_BSK, S.DOMAIN_SEED, S.DOMAIN_TLWE, 0x504B53, PR.DOMAIN_PKE_SEL, PR.DOMAIN_PKE_NOISE,
             PR.DOMAIN_RKE_SEL, PR.DOMAIN_RKE_NOISE, *S.DOMAINS_SYM_TLWE[1:], *S.DOMAINS_SYM_PK, *S.DOMAINS_SYM_RK, *S.DOMAINS_TRLWE]
    assert len(set(words)) == len(words)


@pytest.mark.parametrize("first_group", PM.FIRST)
def test_trlwe_masks_are_the_models(first_group):
    assert np.array_equal(S.trlwe_masks(SEED, first_group, 5), PM.masks(SEED, PM.group_indices(first_group, 5)))


def test_ring_product_is_the_exact_product():
    """the model's coefficient-by-coefficient product against the package's rotated-row sum and a schoolbook row"""
    rng = np.random.default_rng(1)
    a = rng.integers(0, 1 << 32, (2, N), dtype=np.uint64).astype(np.uint32)
    s1 = PM.keys()["random"]
    got = PM.ring_product(a, s1)
    assert np.array_equal(got, S.negacyclic_binary(a, s1))
    c = 700
    want = sum(int(s1[j]) * (int(a[1, c - j]) if j <= c else -int(a[1, c - j + N])) for j in range(N)) % (1 << 32)
    assert int(got[1, c]) == want


@pytest.mark.parametrize("first_group", PM.FIRST, ids=["first0", "firstHIGH"])
@pytest.mark.parametrize("count", PM.COUNTS[:5])
def test_cpu_form_equals_the_model(count, first_group):
    sk = _sk()
    plain = PM.plaintexts(count, count)
    idx = PM.group_indices(first_group, PM.groups_of(count))
    want, _ = PM.encrypt(sk.key_lv1, plain, count, first_group, PM.ALPHA)
    got = S.symmetric_trlwe_rows(SEED, K, idx, sk.key_lv1, plain, count, PM.ALPHA)
    assert got.shape == want.shape == (PM.groups_of(count), 2, N)
    assert np.array_equal(got, want)
    assert np.array_equal(S.symmetric_trlwe_rows(SEED, K, idx, sk.key_lv1, plain, count, PM.ALPHA, full=False), want[:, 1])
    # every slot decrypts, and the unused ones of the last group hold noise only
    e, _ = PM.recover_noise(sk.key_lv1, got, plain, count)
    assert np.abs(e).max() < 6 * PM.ALPHA * 2.0 ** 32
    ph = sk.packed_phase(got, PM.groups_of(count) * N)
    assert np.abs((ph[count:]).view(np.int32)).max(initial=0) < 6 * PM.ALPHA * 2.0 ** 32


@pytest.mark.parametrize("key", ["ones", "zeros", "last"])
def test_cpu_form_equals_the_model_for_the_edge_keys(key):
    sk = _sk(key)
    count = N + 1
    plain = PM.plaintexts(count, 3)
    want, _ = PM.encrypt(sk.key_lv1, plain, count, PM.HIGH, PM.ALPHA)
    got = S.symmetric_trlwe_rows(SEED, K, PM.group_indices(PM.HIGH, 2), sk.key_lv1, plain, count, PM.ALPHA)
    assert np.array_equal(got, want)
    if key == "zeros":  # no product: the body is noise + plaintext
        assert np.array_equal(got[:, 1], PM.noise(K, PM.group_indices(PM.HIGH, 2), PM.ALPHA).words + PM.slots(plain, count))


def test_client_methods_are_the_cpu_form():
    sk = _sk()
    pt = np.random.default_rng(5).uniform(-0.5, 0.5, N + 7)
    want, _ = PM.encrypt(sk.key_lv1, f64_to_torus(pt), len(pt), 3, P.alpha_lv1)
    got = sk.encrypt_packed_f64(pt, rng_key=K, first_group=3, mask_seed=SEED)
    assert np.array_equal(got, want)
    sc = sk.encrypt_packed_f64_seeded(pt, SEED, 3, rng_key=K)
    assert isinstance(sc, S.SeededPackedCiphertexts) and (sc.mask_seed, sc.first_group, sc.count, sc.groups) == (SEED, 3, len(pt), 2)
    assert np.array_equal(sc.bodies, want[:, 1]) and np.array_equal(sc.expand(), want)
    assert sc.nbytes == 2 * N * 4 + 48 and len(sc) == len(pt)
    bits = np.random.default_rng(6).integers(0, 2, N + 7).astype(bool)
    cb = sk.encrypt_packed_bool(bits, rng_key=K, first_group=PM.HIGH, mask_seed=SEED)
    assert np.array_equal(sk.decrypt_packed_bool(cb, len(bits)), bits)
    assert np.array_equal(sk.encrypt_packed_bool_seeded(bits, SEED, PM.HIGH, rng_key=K).expand(), cb)
    msgs = np.arange(N + 7) % 16
    cm = sk.encrypt_packed_lwe_message(msgs, 16, rng_key=K, mask_seed=SEED)
    assert np.array_equal(sk.decrypt_packed_lwe_message(cm, len(msgs), 16), msgs)
    assert np.array_equal(sk.encrypt_packed_lwe_message_seeded(msgs, 16, SEED, rng_key=K).expand(), cm)
    # a fresh mask seed per call when none is given: other masks, the same noise under the same (K, group)
    a, b = (sk.encrypt_packed_f64(pt, rng_key=K, alpha=0.0) for _ in range(2))
    assert not np.array_equal(a[:, 0], b[:, 0])


def test_zero_alpha_has_no_noise():
    sk = _sk()
    pt = np.random.default_rng(5).uniform(-0.5, 0.5, 2 * N + 3)
    got = sk.encrypt_packed_f64(pt, alpha=0.0, rng_key=K, mask_seed=SEED, first_group=PM.HIGH)
    ph = sk.packed_phase(got, 3 * N)
    assert np.array_equal(ph[:len(pt)], f64_to_torus(pt)) and not ph[len(pt):].any()


def test_argument_checks():
    sk = _sk()
    for kw in ({"rng_key": K}, {"device": 0}):
        with pytest.raises(ValueError):
            sk.encrypt_packed_f64([0.1], seed=1, **kw)
        with pytest.raises(ValueError):
            sk.encrypt_packed_bool([1], seed=1, **kw)
        with pytest.raises(ValueError):
            sk.encrypt_packed_lwe_message([1], 4, seed=1, **kw)
    with pytest.raises(ValueError):
        sk.encrypt_packed_f64([0.1], rng_key=b"short")
    with pytest.raises(ValueError):
        sk.encrypt_packed_f64([0.1], rng_key=K, mask_seed=b"short")
    with pytest.raises(ValueError):
        sk.encrypt_packed_f64(np.zeros(N + 1), rng_key=K, first_group=(1 << 64) - 1)
    assert sk.encrypt_packed_f64(np.zeros(N), rng_key=K, first_group=(1 << 64) - 1).shape == (1, 2, N)
    # the un-keyed route knows no group index, no mask seed and no seeded form
    with pytest.raises(ValueError):
        sk.encrypt_packed_f64([0.1], first_group=1)
    with pytest.raises(ValueError):
        sk.encrypt_packed_f64([0.1], seed=1, mask_seed=SEED)
    with pytest.raises(ValueError):
        sk.encrypt_packed_f64_seeded([0.1])
    with pytest.raises(ValueError):
        S.SeededPackedCiphertexts(P, SEED, 0, np.zeros((2, N), np.uint32), N)
    with pytest.raises(ValueError):
        S.SeededPackedCiphertexts(P, b"short", 0, np.zeros((1, N), np.uint32), N)
    with pytest.raises(ValueError):
        S.symmetric_trlwe_rows(SEED, K, [0], sk.key_lv1, np.zeros(N + 1, np.uint32), N + 1, 0.0)


@pytest.mark.parametrize("count", [5, N + 3])
def test_the_unkeyed_route_returns_the_words_it_returned(count):
    """With none of the new arguments encrypt_packed_f64(seed=...) is numpy's generator through the expression restated
    here (the product by the model's ring_product)."""
    sk = _sk()
    pt = np.random.default_rng(8).uniform(-0.5, 0.5, count)
    groups = PM.groups_of(count)
    g = np.random.default_rng(41)
    a = g.integers(0, 1 << 32, (groups, N), dtype=np.uint64).astype(np.uint32)
    noise = f64_to_torus(g.normal(0.0, P.alpha_lv1, groups * N)).reshape(groups, N)
    with np.errstate(over="ignore"):
        b = PM.ring_product(a, sk.key_lv1) + PM.slots(f64_to_torus(pt), count) + noise
    got = sk.encrypt_packed_f64(pt, 41)
    assert np.array_equal(got[:, 0], a) and np.array_equal(got[:, 1], b)
    assert np.array_equal(sk.encrypt_packed_f64(pt, seed=41), got)
    bits = pt > 0
    assert np.array_equal(sk.encrypt_packed_bool(bits, 41), sk.encrypt_packed_f64(np.where(bits, 0.125, -0.125), 41))
    msgs = np.arange(count) % 4
    assert np.array_equal(sk.encrypt_packed_lwe_message(msgs, 4, 41), sk.encrypt_packed_f64(msgs / 8.0, 41))


@pytest.mark.parametrize("alter", PM.ALTERS)
def test_an_altered_model_fails_its_check(alter):
    """each slip is caught by the word comparison, and by a check of its own"""
    sk = _sk()
    count, groups = 3 * N + 5, 4
    plain = PM.plaintexts(count, 2)
    first = PM.HIGH if alter == "ignore_high" else 0
    idx = PM.group_indices(first, groups)
    right, border = PM.encrypt(sk.key_lv1, plain, count, first, PM.ALPHA)
    wrong, _ = PM.encrypt(sk.key_lv1, plain, count, first, PM.ALPHA, alter=alter)
    cpu = S.symmetric_trlwe_rows(SEED, K, idx, sk.key_lv1, plain, count, PM.ALPHA)
    assert KM.compare_words(cpu, right, border)[0] == 0
    with pytest.raises(AssertionError):
        KM.compare_words(cpu, wrong, border, alter)
    e_right, a_right = PM.recover_noise(sk.key_lv1, right, plain, count)
    e_wrong, a_wrong = PM.recover_noise(sk.key_lv1, wrong, plain, count)
    rep_right = KM.noise_report(e_right, PM.ALPHA, KM.REF_SEED, mask=a_right)
    assert not KM.failures(rep_right, 5.0), rep_right
    if alter == "ignore_high":  # groups past a multiple of 2^32 repeat the groups 2^32 k before them
        low, _ = PM.encrypt(sk.key_lv1, plain[2 * N:], count - 2 * N, 0, PM.ALPHA)  # (group 2 of the batch has lo = 0)
        with np.errstate(over="ignore"):
            assert np.array_equal(wrong[2:, 0], low[:, 0]) and np.array_equal(e_wrong[2:], PM.recover_noise(sk.key_lv1, low, plain[2 * N:], count - 2 * N)[0])
        assert not (right[2:, 0] == low[:, 0]).all(axis=1).any()
    elif alter == "noise_from_mask_domain":
        # the noise words of the wrong model are the public mask stream's: under K == S whoever holds S strips the noise
        assert (wrong[:, 1] != right[:, 1]).mean() > 0.9
        same_key, _ = PM.encrypt(sk.key_lv1, plain, count, first, PM.ALPHA, mask_seed=K, alter=alter)
        public = PM.noise(K, idx, PM.ALPHA, alter=alter).words
        assert np.array_equal(PM.recover_noise(sk.key_lv1, same_key, plain, count)[0].view(np.uint32), public)
    elif alter == "same_pair":
        rep = KM.noise_report(e_wrong, PM.ALPHA, KM.REF_SEED, mask=a_wrong)
        assert "pair_corr" in KM.failures(rep, 6.0) and abs(rep["pair_corr"]) > 40
    else:  # the neighbour's plaintext: no slot decrypts
        assert np.abs(e_right).max() < 6 * PM.ALPHA * 2.0 ** 32
        assert (np.abs(e_wrong.astype(np.float64)) > 6 * PM.ALPHA * 2.0 ** 32).mean() > 0.9


def test_fixed_key_keeps_the_gpu_cases_within_their_conditions():
    """What tests/test_gpu_packed_encrypt.py relies on: under the fixed K at most 16 borderline noise samples
    per case (about 2^-19 a sample: 0.1 expected in the 66 k of the largest), and every sample within 6 alpha."""
    worst = 0
    for first in PM.FIRST:
        e = PM.noise(K, PM.group_indices(first, PM.groups_of(max(PM.COUNTS))), PM.ALPHA)  # (the smaller cases are its prefixes)
        worst = max(worst, int(e.border.sum()))
        assert int(e.border.sum()) <= KM.MAX_MISMATCHES
        assert np.abs(e.words.view(np.int32)).max() < 6 * PM.ALPHA * 2.0 ** 32
    print(f"PACKEDENCRYPT borderline samples under the fixed key: at most {worst} a case")


def test_exports_refuse_a_null_handle():
    lib = _capi.lib()
    assert lib.tfhe_hip_batch_encrypt_trlwe(None, None, None, 0, 0.0, None, None, 0, None, None) == _capi.EINVAL
    assert lib.tfhe_hip_batch_encrypt_trlwe_dev(None, None, None, 0, 0.0, None, None, 0, None, None, None) == _capi.EINVAL
    assert lib.tfhe_hip_expand_seeded_trlwe(None, None, 0, None, 0, None) == _capi.EINVAL
    assert lib.tfhe_hip_expand_seeded_trlwe_dev(None, None, 0, None, 0, None, None) == _capi.EINVAL


def build_cpp_packed_encrypt(outdir):
    """tests/cpp/test_packed_encrypt.cpp, built as test_decrypt_host.build_cpp_decrypt builds its program."""
    exe = os.path.join(outdir, "test_packed_encrypt")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_packed_encrypt.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-fopenmp", "-pthread"])
    return exe


def test_cpp_packed_encrypt_program_builds(tmp_path):
    """The C++ mirror's encrypt_packed_batch / expand_seeded_packed program compiles and links against the header and the
    library (run on the GPU by tests/test_gpu_packed_encrypt.py)."""
    assert os.path.exists(build_cpp_packed_encrypt(str(tmp_path)))
