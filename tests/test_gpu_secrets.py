"""The host paths that csrc/secrets.hpp carries (SecretStage, scrub), at the smallest sizes that reach them.  No kernel
is under test here: every result is held, word for word, to the same call on a lone Engine.

Pinned-arena path: a member of a pool with several members stages operands and results of 1 MiB or more through its
pinned arenas (via_pin), which the host forms' epilogue now wipes.  262,144 words are exactly 1 MiB, 262,143 stay
below it; the calls go straight to the C ABI on the member's context.

Key generators: their secrets travel through the context's one `sym_sec` buffer, as the encrypting and decrypting
calls' do, in another layout each: one handle runs a cloud-key generation, a host-form encryption and a packing-key
generation in a row, each against the same call on a fresh handle."""
import ctypes as C

import numpy as np
import pytest

import keygen_model as KM
from rs_tfhe_amd import _capi
from rs_tfhe_amd.engine import _ptr
from rs_tfhe_amd.params import N

pytestmark = pytest.mark.gpu

P = KM.shape_params(KM.SHAPES[0])  # (the encrypting and decrypting calls need no key on the handle: a small set serves)
K = KM.GEN_KEY
SEED = bytes((91 * i + 5) & 0xFF for i in range(32))
ALPHA0, ALPHA1 = KM.ALPHA_KSK, KM.ALPHA_BSK
PHASE = _capi.DECRYPT_MODES["phase"]


def _bytes32(b):
    return (C.c_uint8 * 32).from_buffer_copy(b)


def _calls(lib, ctx, sk, plain):
    """The three host-form calls on context `ctx`: bodies-only TLWE encryption, packed encryption writing bodies and out,
    and the PHASE decryption of those groups."""
    count = len(plain)
    groups = -(-count // N)
    rk, seed = _bytes32(K), _bytes32(SEED)
    k0, k1 = np.ascontiguousarray(sk.key_lv0, np.uint32), np.ascontiguousarray(sk.key_lv1, np.uint32)
    bodies = np.full(count, 0xFFFFFFFF, np.uint32)
    _capi.check(ctx, lib.tfhe_hip_batch_encrypt(ctx, _ptr(k0), _ptr(plain), count, C.c_double(ALPHA0), C.addressof(rk),
                                               C.addressof(seed), C.c_uint64(7), _ptr(bodies), None))
    pbodies = np.full((groups, N), 0xFFFFFFFF, np.uint32)
    pout = np.full((groups, 2, N), 0xFFFFFFFF, np.uint32)
    _capi.check(ctx, lib.tfhe_hip_batch_encrypt_trlwe(ctx, _ptr(k1), _ptr(plain), count, C.c_double(ALPHA1), C.addressof(rk),
                                                     C.addressof(seed), C.c_uint64(3), _ptr(pbodies), _ptr(pout)))
    phases = np.full(count, 0xFFFFFFFF, np.uint32)
    _capi.check(ctx, lib.tfhe_hip_batch_decrypt_trlwe(ctx, _ptr(k1), _ptr(pout), groups, count, PHASE, C.c_uint32(0),
                                                     _ptr(phases)))
    return {"bodies": bodies, "packed_bodies": pbodies, "packed": pout, "phases": phases}


@pytest.mark.parametrize("count", [262144, 262143], ids=["at_1MiB", "under_1MiB"])
def test_pool_member_host_forms_equal_a_lone_engine(count):
    import rs_tfhe_amd as R

    sk = KM.secret_key(P)
    plain = np.random.default_rng(count).integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
    pool, lone = R.Pool(P, [0, 0]), R.Engine(P, 0)
    try:
        got = _calls(pool._lib, pool._member_ctx(0), sk, plain)
        again = _calls(pool._lib, pool._member_ctx(0), sk, plain)  # (over buffers the first round scrubbed)
        want = _calls(lone._lib, lone._member_ctx(0), sk, plain)
    finally:
        pool.close()
        lone.close()
    for name, w in want.items():
        assert np.array_equal(got[name], w), name
        assert np.array_equal(again[name], w), name
    assert np.array_equal(want["packed"][:, 1], want["packed_bodies"])
    # the phases are the plaintexts but for the noise: the comparison above is of decryptions, not of 0xFFFFFFFF
    assert np.abs((want["phases"] - plain).view(np.int32)).max() < 1 << 12  # (12 sigma of alpha_lv1 2^32 is 2^10)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_key_generators_share_the_secret_buffer():
    import rs_tfhe_amd as R

    sk = KM.secret_key(P)
    plain = np.array([0x20000000, 0xE0000000, 0x12345678], np.uint32)

    def cloud(e):
        e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=77)
        ck = e.export_cloud_key()
        return ck.bootstrapping_key, ck.key_switching_key

    def encrypt(e):
        return (e.batch_encrypt(sk.key_lv0, plain, ALPHA0, K, SEED, first_index=11),)

    def packing(e):
        pk = e.gen_packing_key(sk.key_lv0, sk.key_lv1, rng_key=K, alpha=ALPHA1)
        return np.frombuffer(pk.mask_seed, np.uint8), pk.bodies

    steps = (cloud, encrypt, packing, encrypt, cloud)  # (every layout once more behind the other two)
    one = R.Engine(P, 0)
    try:
        got = [step(one) for step in steps]
    finally:
        one.close()
    for step in steps[:3]:
        fresh = R.Engine(P, 0)
        try:
            want = step(fresh)
        finally:
            fresh.close()
        assert any(_bits(w).any() for w in want), step.__name__
        for g in (g for s, g in zip(steps, got) if s is step):
            assert len(g) == len(want) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(g, want)), step.__name__
