"""Seeded (compressed) cloud keys and ciphertexts on the host, no GPU: the numpy ChaCha20 against RFC 8439, the CPU
compressor's rows against the normative format of include/tfhe_hip.h (every row's phase, exactly, at zero noise),
the noise scale at the real alphas, the .npz round trip, the sizes the C ABI reports, and seeded encryption."""
import ctypes
import os

import numpy as np
import pytest

from rs_tfhe_amd import _capi, seeded as S
from rs_tfhe_amd.client import SecretKey
from rs_tfhe_amd.key import CompressedCloudKey
from rs_tfhe_amd.params import N, SECURITY_80_BIT, SECURITY_128_BIT, SECURITY_UINT4, SECURITY_UINT8

K = bytes(range(100, 132))


def test_chacha20_block_matches_rfc8439():
    """RFC 8439 section 2.3.2: key 00..1f, nonce (00:00:00:09, 00:00:00:4a, 00:00:00:00), counter 1."""
    w = S.chacha20_block(bytes(range(32)), 1, 0x09000000, 0x4A000000, 0)
    want = [0xE4E7F110, 0x15593BD1, 0x1FDD0F50, 0xC47120A3, 0xC7F4D1C7, 0x0368C033, 0x9AAA2204, 0x4E6CD4C3,
            0x466482D2, 0x09AA9F07, 0x05D7C214, 0xA2028BD9, 0xD19C12B5, 0xB94E16DE, 0xE883D0CB, 0x4E3C50A2]
    assert [int(x) for x in w] == want
    # vectorised over counters = one block at a time
    many = S.chacha20_block(bytes(range(32)), np.arange(4), 0x09000000, 0x4A000000, 0)
    assert np.array_equal(many[1], w)
    # keystream word x is word x % 16 of block x / 16
    ks = S.keystream(bytes(range(32)), 40, 0x09000000, 0x4A000000, 0)
    assert np.array_equal(ks[16:32], w) and np.array_equal(ks[32:40], many[2][:8])


def test_mask_seed_is_a_prf_of_the_generator_key():
    s = S.mask_seed_of(K)
    assert s == S.mask_seed_of(K) and len(s) == 32
    assert s == S.chacha20_block(K, 0, 0, 20, 0x444553)[:8].astype("<u4").tobytes()
    assert s != S.mask_seed_of(bytes(32)) and s != K


def _exact_negacyclic(a, s1):
    """a (*) s1 through an independent route: a float64 product with s1's negacyclic matrix (|sums| < 2^42: exact)."""
    idx = (np.arange(N)[None, :] - np.arange(N)[:, None])  # M[j, c] multiplies a[j] into coefficient c: s1[c - j]
    m = np.where(idx >= 0, s1[idx % N].astype(np.float64), -s1[idx % N].astype(np.float64))
    return (a.astype(np.float64) @ m).astype(np.int64).astype(np.uint32)


def _secret(p, seed):
    return SecretKey.new(p, seed)


@pytest.mark.parametrize("p", [SECURITY_80_BIT, SECURITY_UINT4], ids=lambda p: p.name)
def test_compressor_rows_follow_the_format_exactly_at_zero_noise(p):
    sk = _secret(p, 5)
    ck = sk.compressed_cloud_key(rng_key=K, alpha_ksk=0.0, alpha_bsk=0.0)
    assert ck.mask_seed == S.mask_seed_of(K)
    # KSK: every row (i, j, k) has phase k s1[i] 2^(32 - (j+1) basebit); the k = 0 bodies are 0
    full = S.expand_ksk(p, ck.mask_seed, ck.ksk_bodies).reshape(-1, p.n + 1)
    r = np.arange(len(full))
    k, j, i = r % p.base, (r // p.base) % p.iks_t, r // (p.base * p.iks_t)
    inner = (full[:, :-1].astype(np.uint64) @ sk.key_lv0.astype(np.uint64)).astype(np.uint32)
    phase = full[:, -1] - inner
    want = ((k * sk.key_lv1[i]).astype(np.uint64) << (32 - (j + 1) * p.basebit).astype(np.uint64)).astype(np.uint32)
    assert np.array_equal(phase[k > 0], want[k > 0])
    assert not full[k == 0].any() and not ck.ksk_bodies.reshape(-1)[k == 0].any()
    # the masks are the keystream of (r, 16, "KSK") under S
    assert np.array_equal(full[7, :p.n], S.keystream(ck.mask_seed, p.n, 7, 16, 0x4B534B))
    # BSK: every row r = i*2l + q has phase -p g_q s1 (q < l) or p g_{q-l} X^0 (q >= l)
    rows = S.expand_bsk_torus(p, ck.mask_seed, ck.bsk_bodies).reshape(-1, 2, N)
    ph = rows[:, 1] - _exact_negacyclic(rows[:, 0], sk.key_lv1)
    rr = np.arange(len(rows))
    q, ii = rr % (2 * p.l), rr // (2 * p.l)
    g = np.array([S.gadget(p, d) for d in range(p.l)], np.uint32)
    pg = sk.key_lv0[ii] * g[q % p.l]
    want = np.zeros_like(ph)
    low = q < p.l
    want[low] = (np.uint32(0) - pg[low])[:, None] * sk.key_lv1[None, :]
    want[~low, 0] = pg[~low]
    assert np.array_equal(ph, want)
    assert np.array_equal(rows[3, 0], S.keystream(ck.mask_seed, N, 3, 18, 0x42534B))


def test_compressor_noise_at_the_real_alphas():
    """Residuals against the zero-noise phases stay within 7 sigma (~10^5 KSK and 3.3 10^6 BSK samples)."""
    p = SECURITY_80_BIT
    sk = _secret(p, 6)
    ck = sk.compressed_cloud_key(rng_key=K)
    ck0 = sk.compressed_cloud_key(rng_key=K, alpha_ksk=0.0, alpha_bsk=0.0)
    assert ck.mask_seed == ck0.mask_seed  # same masks: the bodies differ by the noise alone
    dk = (ck.ksk_bodies - ck0.ksk_bodies).reshape(-1).view(np.int32).astype(np.float64) / 2.0 ** 32
    live = (np.arange(dk.size) % p.base) != 0
    assert np.abs(dk[live]).max() < 7 * p.alpha_lv0
    assert 0.8 * p.alpha_lv0 < dk[live].std() < 1.2 * p.alpha_lv0
    db = (ck.bsk_bodies - ck0.bsk_bodies).reshape(-1).view(np.int32).astype(np.float64) / 2.0 ** 32
    assert np.abs(db).max() < 7 * p.alpha_lv1 + 2.0 ** -31
    assert 0.8 * p.alpha_lv1 < db.std() < 1.2 * p.alpha_lv1


def test_save_load_round_trip_and_sizes(tmp_path):
    p = SECURITY_80_BIT
    ck = _secret(p, 7).compressed_cloud_key(rng_key=K)
    path = tmp_path / "ck.npz"
    ck.save(path)
    back = CompressedCloudKey.load(path)
    assert back.params == p and back.mask_seed == ck.mask_seed
    assert np.array_equal(back.bsk_bodies, ck.bsk_bodies) and np.array_equal(back.ksk_bodies, ck.ksk_bodies)
    assert back.decomposition_offset == ck.decomposition_offset
    assert np.array_equal(back.blind_rotate_testvec, ck.blind_rotate_testvec)
    with pytest.raises(ValueError):
        CompressedCloudKey.load(path, params=SECURITY_128_BIT)
    z = dict(np.load(path))
    z["format_version"] = np.uint32(99)
    np.savez(tmp_path / "v99.npz", **z)
    with pytest.raises(ValueError):
        CompressedCloudKey.load(tmp_path / "v99.npz")
    # the sizes the C ABI reports (no device needed), and the issue's table for SECURITY_128_BIT / UINT8
    lib = _capi.lib()
    for q, mb in ((p, None), (SECURITY_128_BIT, 17.35), (SECURITY_UINT4, 7.11), (SECURITY_UINT8, 11.08)):
        bw, kw = ctypes.c_size_t(), ctypes.c_size_t()
        cp = _capi.Params(q.n, q.l, q.bgbit, q.basebit, q.iks_t)
        assert lib.tfhe_hip_compressed_key_words(ctypes.byref(cp), ctypes.byref(bw), ctypes.byref(kw)) == _capi.OK
        assert bw.value == q.n * 2 * q.l * N and kw.value == N * q.iks_t * q.base
        if q is p:
            assert (bw.value + kw.value) * 4 + 32 == ck.nbytes
        else:
            assert abs(((bw.value + kw.value) * 4 + 32) / 1e6 - mb) < 0.01
    bad = _capi.Params(700, 4, 6, 2, 9)
    bw = ctypes.c_size_t()
    assert lib.tfhe_hip_compressed_key_words(ctypes.byref(bad), ctypes.byref(bw), ctypes.byref(bw)) == _capi.EINVAL
    assert lib.tfhe_hip_compressed_key_words(None, ctypes.byref(bw), ctypes.byref(bw)) == _capi.EINVAL


def test_compressed_entry_points_refuse_null_handles_without_gpu():
    lib = _capi.lib()
    seed = (ctypes.c_uint8 * 32)()
    buf = np.zeros(16, np.uint32)
    p = buf.ctypes.data
    off = ctypes.c_uint32()
    assert lib.tfhe_hip_gen_compressed_cloud_key(None, p, p, 0.0, 0.0, None, ctypes.addressof(seed), p, p,
                                                 ctypes.byref(off)) == _capi.EINVAL
    assert lib.tfhe_hip_load_compressed_cloud_key(None, ctypes.addressof(seed), p, p, 0, p) == _capi.EINVAL
    assert lib.tfhe_hip_pool_load_compressed_cloud_key(None, ctypes.addressof(seed), p, p, 0, p) == _capi.EINVAL
    assert lib.tfhe_hip_expand_seeded_tlwe(None, ctypes.addressof(seed), 0, p, 1, p) == _capi.EINVAL
    assert lib.tfhe_hip_expand_seeded_tlwe_dev(None, ctypes.addressof(seed), 0, p, 1, p, None) == _capi.EINVAL


def test_seeded_encryption_decrypts_and_follows_the_index_rule():
    p = SECURITY_128_BIT
    sk = _secret(p, 8)
    bits = np.arange(37) % 3 == 0
    sc = sk.encrypt_bool_seeded(bits, mask_seed=bytes(32), first_index=(1 << 32) - 5, seed=1)
    assert sc.nbytes == 37 * 4 + 40
    cts = sc.expand()
    assert np.array_equal(sk.decrypt_bool(cts), bits)
    # ciphertext g = first + m: nonce (g & 0xffffffff, g >> 32, "EWL"), across the 2^32 boundary
    for m in (0, 4, 5, 36):
        g = (1 << 32) - 5 + m
        assert np.array_equal(cts[m, :-1], S.keystream(bytes(32), p.n, g & 0xFFFFFFFF, g >> 32, 0x45574C)), m
    # LWE messages too
    msgs = np.arange(20) % 4
    sm = sk.encrypt_lwe_message_seeded(msgs, 4, mask_seed=K, first_index=1000, seed=2)
    assert np.array_equal(sk.decrypt_lwe_message(sm.expand(), 4), msgs)
    # a fresh seed per call when none is given
    a, b = sk.encrypt_f64_seeded([0.125]), sk.encrypt_f64_seeded([0.125])
    assert a.mask_seed != b.mask_seed and len(a.mask_seed) == 32
