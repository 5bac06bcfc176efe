"""Public-key encryption and the asymmetric re-encryption key on the GPU (csrc/pk_encrypt.hpp: k_pke_planes,
k_pke_selectors, k_pke_mfma behind tfhe_hip_load_public_key / tfhe_hip_batch_pk_encrypt[_dev] /
tfhe_hip_gen_reenc_key_asymmetric) held to the term-by-term CPU model of tests/pk_encrypt_model.py.

Under a fixed generator key every selector bit and every noise sample is a keystream position the model knows: at
alpha = 0 the words must be EQUAL; with noise a body may differ from the model's by exactly +-1 LSB only where the
long-double sampler marks its sample borderline, at most 16 words a case (KM.compare_words).  The shapes are the smallest
at which the kernels can go wrong (PM.CASES).  The model could share a mistake with the kernels; decryption under the
secret key and the OS-keyed statistics could not.

Every test prints its figures (`PKENCRYPT {json}` lines; run with -s) before it asserts."""
import json
import subprocess

import numpy as np
import pytest

import keygen_model as KM
import pk_encrypt_model as PM
from test_pk_encrypt_host import build_cpp_pk_encrypt
from rs_tfhe_amd.client import SecretKey, f64_to_torus

pytestmark = pytest.mark.gpu

K = PM.K
_KEYS = {}


def _say(**kv):
    print("PKENCRYPT " + json.dumps(kv, default=float))


def _dev_encrypt(eng, plain, alpha, rng_key, first_index):
    """batch_pk_encrypt_dev on a stream of the caller's, back on the host"""
    import torch

    tp = torch.from_numpy(np.ascontiguousarray(plain, np.uint32).view(np.int32)).cuda()
    to = torch.empty((len(plain), eng.params.n + 1), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.batch_pk_encrypt_dev(tp, to, alpha, rng_key, first_index, s)
    s.synchronize()
    return to.cpu().numpy().view(np.uint32)


def _phase_error(sk, cts, plain):
    return (sk.phase(cts) - np.asarray(plain, np.uint32)).view(np.int32).astype(np.float64) / 2.0 ** 32


# ---- 1. every word against the model --------------------------------------------------------------------------------
@pytest.mark.parametrize("n,size,count,first_index,alpha", PM.CASES, ids=lambda v: str(v))
def test_words_equal_the_model(n, size, count, first_index, alpha):
    import rs_tfhe_amd as R

    p = PM.params(n)
    enc = PM.public_key(n, size)
    plain = np.random.default_rng(n + size + count).integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
    eng = R.Engine(p, 0)
    try:
        assert not eng.public_key_is_loaded()
        eng.load_public_key(enc)
        assert eng.public_key_is_loaded()
        host = eng.batch_pk_encrypt(plain, alpha, K, first_index)
        dev = _dev_encrypt(eng, plain, alpha, K, first_index)
    finally:
        eng.close()
    want, border = PM.encrypt(enc, K, PM.row_indices(first_index, count), plain, alpha)
    _say(case="words", n=n, size=size, count=count, first_index=first_index, alpha=alpha, words=int(want.size),
         host_differing=int((host != want).sum()), dev_differing=int((dev != want).sum()), borderline=int(border.sum()))
    assert host.shape == dev.shape == want.shape == (count, n + 1)
    if alpha == 0.0:
        assert not border.any()
        assert np.array_equal(host, want) and np.array_equal(dev, want)
    for got, form in ((host, "host"), (dev, "dev")):
        mism, _ = KM.compare_words(got, want, border, f"pk_encrypt {form} form n {n} size {size} count {count}")
        assert mism <= KM.MAX_MISMATCHES
    # the ciphertexts are encryptions of `plain` under the secret key behind the public key
    if alpha < 0.1:  # (at 0.5 the noise wraps the torus) 7 sigma of every entry taken, plus a truncation step a term
        err = _phase_error(KM.secret_key(p), host, plain)
        assert np.abs(err).max() <= 7.0 * np.hypot(p.alpha_lv0 * np.sqrt(size), alpha) + (size + 2) * 2.0 ** -32


def test_adversarial_public_key():
    """Words 0x80000000 and 0x7F7F7F80: extreme plane bytes, a carry out of every plane; alpha = 0, so equality."""
    import rs_tfhe_amd as R

    n, size, count = 255, 1399, 33
    enc = PM.adversarial_key(n, size)
    plain = np.arange(count, dtype=np.uint32) * np.uint32(0x01234567)
    eng = R.Engine(PM.params(n), 0)
    try:
        eng.load_public_key(enc)
        host = eng.batch_pk_encrypt(plain, 0.0, K, PM.HIGH)
        dev = _dev_encrypt(eng, plain, 0.0, K, PM.HIGH)
    finally:
        eng.close()
    want, _ = PM.encrypt(enc, K, PM.row_indices(PM.HIGH, count), plain, 0.0)
    _say(case="adversarial", host_differing=int((host != want).sum()), dev_differing=int((dev != want).sum()))
    assert np.array_equal(host, want) and np.array_equal(dev, want)


# ---- 2. state --------------------------------------------------------------------------------------------------------
def test_public_key_state():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi

    n, count = 33, 40
    p = PM.params(n)
    sk = KM.secret_key(p)
    enc, other = PM.public_key(n, 66), PM.public_key(n, 31)
    plain = np.arange(count, dtype=np.uint32) * np.uint32(0x9E3779B9)
    rows = PM.row_indices(3, count)
    want, _ = PM.encrypt(enc, K, rows, plain, 0.0)
    eng = R.Engine(p, 0)
    try:
        with pytest.raises(_capi.TfheHipError, match="public key not loaded") as err:
            eng.batch_pk_encrypt(plain, 0.0, K, 3)
        assert err.value.code == _capi.ENOKEY
        with pytest.raises(_capi.TfheHipError) as err:
            eng.gen_reenc_key_asymmetric(sk.key_lv0, 0.0, K)
        assert err.value.code == _capi.ENOKEY
        eng.load_public_key(enc)
        assert np.array_equal(eng.batch_pk_encrypt(plain, 0.0, K, 3), want)
        # a cloud-key load and a re-encryption-key load leave the public key encrypting the same words
        eng.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=5)
        assert eng.public_key_is_loaded() and np.array_equal(eng.batch_pk_encrypt(plain, 0.0, K, 3), want)
        eng.load_reenc_key(np.zeros((p.n * p.iks_t * p.base, p.n + 1), np.uint32))
        assert eng.reenc_key_is_loaded() and eng.public_key_is_loaded()
        assert np.array_equal(eng.batch_pk_encrypt(plain, 0.0, K, 3), want)
        # a view's public key is its own
        view = eng.new_key_view()
        assert not view.public_key_is_loaded()
        with pytest.raises(_capi.TfheHipError) as err:
            view.batch_pk_encrypt(plain, 0.0, K, 3)
        assert err.value.code == _capi.ENOKEY
        view.load_public_key(other)
        assert np.array_equal(view.batch_pk_encrypt(plain, 0.0, K, 3), PM.encrypt(other, K, rows, plain, 0.0)[0])
        assert np.array_equal(eng.batch_pk_encrypt(plain, 0.0, K, 3), want)
        view.close()
        # refused calls leave the previous key
        for bad in (0, 8193):
            with pytest.raises(_capi.TfheHipError) as err:
                eng.load_public_key(np.zeros((bad, p.n + 1), np.uint32))
            assert err.value.code == _capi.EINVAL
            assert eng.public_key_is_loaded() and np.array_equal(eng.batch_pk_encrypt(plain, 0.0, K, 3), want)
        for bad in (-1.0, float("nan")):
            with pytest.raises(_capi.TfheHipError) as err:
                eng.batch_pk_encrypt(plain, bad, K, 3)
            assert err.value.code == _capi.EINVAL
        assert eng.batch_pk_encrypt(np.zeros(0, np.uint32), 0.0, K, 3).shape == (0, p.n + 1)
        # the largest key: 8192 encryptions, 256 K-steps; and a smaller one after it on the same handle
        big = np.random.default_rng(8).integers(0, 1 << 32, (8192, p.n + 1), dtype=np.uint64).astype(np.uint32)
        eng.load_public_key(big)
        assert np.array_equal(eng.batch_pk_encrypt(plain[:33], 0.0, K, 3), PM.encrypt(big, K, rows[:33], plain[:33], 0.0)[0])
        eng.load_public_key(enc)
        assert np.array_equal(eng.batch_pk_encrypt(plain, 0.0, K, 3), want)
    finally:
        eng.close()


# ---- 3. the asymmetric re-encryption key ----------------------------------------------------------------------------
def _parties(p):
    """(Alice the delegator, Bob the delegatee, Bob's public key of 2n encryptions)"""
    from rs_tfhe_amd import proxy_reenc as PR

    alice, bob = SecretKey.new(p, 77), SecretKey.new(p, 78)
    return alice, bob, PR.PublicKeyLv0.new(bob, seed=79)


def _key_model(p):
    if p.name not in _KEYS:
        alice, _, pk = _parties(p)
        _KEYS[p.name] = PM.reenc_key(p, pk.encryptions, alice.key_lv0, K, p.alpha_lv0)
    return _KEYS[p.name]


def _key_params(which):
    import rs_tfhe_amd as R

    return PM.params(PM.SHAPE[0]) if which == "small" else R.params.SECURITY_128_BIT


@pytest.mark.parametrize("which", ["small", "SECURITY_128_BIT"])
def test_asymmetric_key_equals_the_model(which):
    import rs_tfhe_amd as R

    p = _key_params(which)
    alice, bob, pk = _parties(p)
    want, border = _key_model(p)
    bits = np.random.default_rng(5).integers(0, 2, 70).astype(bool)
    ca = alice.encrypt_bool(bits, 80)
    gen, quiet = R.Engine(p, 0), R.Engine(p, 0)
    try:
        gen.load_public_key(pk)
        key = gen.gen_reenc_key_asymmetric(alice.key_lv0, rng_key=K)
        assert gen.reenc_key_is_loaded() and gen.public_key_is_loaded()
        on_gen = gen.batch_reencrypt(ca)
        other = gen.new_key_view()
        other.load_reenc_key(key)
        on_other = other.batch_reencrypt(ca)
        other.close()
        quiet.load_public_key(pk)
        assert quiet.gen_reenc_key_asymmetric(alice.key_lv0, rng_key=K, download=False) is None
        on_quiet = quiet.batch_reencrypt(ca)
    finally:
        gen.close()
        quiet.close()
    rate = float((bob.decrypt_bool(on_gen) == bits).mean())
    _say(case="asymmetric key", set=p.name, words=int(want.size), words_differing=int((key != want).sum()),
         borderline=int(border.sum()), loaded_equal=bool(np.array_equal(on_gen, on_other)),
         no_download_equal=bool(np.array_equal(on_gen, on_quiet)), decrypt_rate=rate)
    shaped = key.reshape(p.n, p.iks_t, p.base, p.n + 1)
    assert not shaped[:, :, 0, :].any()
    mism, _ = KM.compare_words(key, want, border, f"asymmetric key {p.name}")
    assert mism <= KM.MAX_MISMATCHES
    assert np.array_equal(on_gen, on_other), "the generating handle holds another key than key_out"
    assert np.array_equal(on_gen, on_quiet), "key_out = NULL left another key on the handle"
    assert rate > 0.90


def test_asymmetric_key_refusals_leave_the_keys():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi

    p = _key_params("small")
    alice, _, pk = _parties(p)
    ca = alice.encrypt_bool([1, 0, 1, 1], 81)
    eng = R.Engine(p, 0)
    try:
        eng.load_public_key(pk)
        eng.gen_reenc_key_asymmetric(alice.key_lv0, rng_key=K, download=False)
        before = eng.batch_reencrypt(ca)
        for bad in (-1.0, float("nan")):
            with pytest.raises(_capi.TfheHipError) as err:
                eng.gen_reenc_key_asymmetric(alice.key_lv0, alpha=bad, rng_key=K)
            assert err.value.code == _capi.EINVAL
        assert eng._lib.tfhe_hip_gen_reenc_key_asymmetric(eng._ctx, None, _capi.C.c_double(0.0), None, None) == _capi.EINVAL
        assert eng.reenc_key_is_loaded() and np.array_equal(eng.batch_reencrypt(ca), before)
    finally:
        eng.close()
    big = R.Engine(R.params.SECURITY_UINT7, 0)  # n = 1160: refused with the message load gives
    try:
        big.load_public_key(np.zeros((2, 1161), np.uint32))
        with pytest.raises(_capi.TfheHipError, match="n <= N") as err:
            big.gen_reenc_key_asymmetric(np.zeros(1160, np.uint32), rng_key=K)
        assert err.value.code == _capi.EINVAL
    finally:
        big.close()


# ---- 4. the OS-keyed route ------------------------------------------------------------------------------------------
def test_os_keyed_route():
    """rng_key = NULL at SECURITY_128_BIT: two calls share no row; all 4,096 bits decrypt (noise alpha sqrt(taken + 1) ~
    5e-4 against a margin of 1/8); the phase error's std is within 6 SE of alpha sqrt(size / 2 + 1), SE 1 / sqrt(2 M)."""
    import rs_tfhe_amd as R

    p = R.params.SECURITY_128_BIT
    _, bob, pk = _parties(p)
    bits = np.random.default_rng(12).integers(0, 2, 4096).astype(bool)
    cts = [pk.encrypt_bool(bits, p.alpha_lv0, device=0) for _ in range(2)]
    pk.close()
    both = np.concatenate(cts)
    wrong = [int((bob.decrypt_bool(c) != bits).sum()) for c in cts]
    err = np.concatenate([_phase_error(bob, c, f64_to_torus(np.where(bits, 0.125, -0.125))) for c in cts])
    size = len(pk.encryptions)
    expect = p.alpha_lv0 * np.sqrt(size / 2 + 1)
    se = (err.std() / expect - 1.0) * np.sqrt(2.0 * err.size)
    _say(case="os-keyed", wrong=wrong, std=float(err.std()), expected=float(expect), std_in_se=float(se), M=int(err.size))
    assert len(np.unique(both, axis=0)) == len(both), "two OS-keyed calls share a row"
    assert wrong == [0, 0]
    assert abs(se) <= 6.0


# ---- 5. end to end --------------------------------------------------------------------------------------------------
def test_end_to_end_at_security_128_bit():
    """Alice's 256 bits, a GPU-generated asymmetric key, Bob decrypts: the decoded bits equal, bit for bit, those obtained
    with the CPU form's key under the same K, and the rate meets the reference's own bar (proxy_reenc.rs:629-634)."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import proxy_reenc as PR

    p = R.params.SECURITY_128_BIT
    alice, bob, pk = _parties(p)
    bits = np.random.default_rng(13).integers(0, 2, 256).astype(bool)
    ca = alice.encrypt_bool(bits, 82)
    with PR.ProxyReencryptionKey.new_asymmetric(alice, pk, rng_key=K, device=0) as on_gpu:
        assert on_gpu._view is not None and on_gpu._view[1].reenc_key_is_loaded()  # generated in place: nothing to upload
        got = on_gpu.reencrypt(ca)
        differing = int((on_gpu.key_encryptions != _key_model(p)[0]).sum())
    pk.close()
    with PR.ProxyReencryptionKey.new_asymmetric(alice, pk, rng_key=K) as on_cpu:
        ref = on_cpu.reencrypt(ca)
    err = _phase_error(bob, ref, f64_to_torus(np.where(bits, 0.125, -0.125)))
    rate = float((bob.decrypt_bool(got) == bits).mean())
    _say(case="end to end", decrypt_rate=rate, rate_cpu_key=float((bob.decrypt_bool(ref) == bits).mean()),
         sigma_cpu_key=float(err.std()), key_words_differing_from_model=differing,
         ciphertexts_differing=int((got != ref).any(axis=1).sum()))
    assert np.array_equal(bob.decrypt_bool(got), bob.decrypt_bool(ref))
    assert rate > 0.90


# ---- 6. C++ ---------------------------------------------------------------------------------------------------------
def test_cpp_encrypts_and_generates_the_same_words(tmp_path):
    """encrypt_batch and generate_asymmetric under the fixed K: the checksums the program prints are the Python route's."""
    import rs_tfhe_amd as R

    p = _key_params("small")
    alice, _, pk = _parties(p)
    count, first_index = 70, 9
    plain = f64_to_torus(np.where(np.arange(count) % 3 == 0, 0.125, -0.125))
    eng = R.Engine(p, 0)
    try:
        eng.load_public_key(pk)
        enc = eng.batch_pk_encrypt(plain, p.alpha_lv0, K, first_index)
        key = eng.gen_reenc_key_asymmetric(alice.key_lv0, rng_key=K)
        re = eng.batch_reencrypt(enc)
    finally:
        eng.close()
    blob = tmp_path / "in.bin"
    blob.write_bytes(K + np.ascontiguousarray(alice.key_lv0, "<u4").tobytes() + np.ascontiguousarray(pk.encryptions, "<u4").tobytes())
    exe = build_cpp_pk_encrypt(str(tmp_path))
    args = [str(v) for v in PM.SHAPE] + [repr(p.alpha_lv0), str(len(pk.encryptions)), str(count), str(first_index), str(blob)]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    _say(case="c++", returncode=r.returncode, stdout=r.stdout.strip().splitlines())
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(ln.split(" ", 1) for ln in r.stdout.strip().splitlines())
    assert int(lines["enc_checksum"]) == PM.checksum(enc)
    assert int(lines["key_checksum"]) == PM.checksum(key)
    assert int(lines["reenc_checksum"]) == PM.checksum(re)
    assert lines["ok:"].endswith("bytes")
