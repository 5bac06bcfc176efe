"""Packing key switch on the host, no GPU: the integer model (packing.pack_model) against the direct definition of
include/tfhe_hip.h, the signed decomposition identity, every packing-key row's phase at zero noise, client decryption of
model-packed booleans and messages, the sizes and EINVAL cases of the C ABI that need no device, and the .npz round
trip."""
import ctypes

import numpy as np
import pytest

from rs_tfhe_amd import _capi, packing as PK
from rs_tfhe_amd.client import SecretKey
from rs_tfhe_amd.params import N, PARAM_SETS, SECURITY_80_BIT, SECURITY_128_BIT, SECURITY_UINT4, SECURITY_UINT8
from rs_tfhe_amd.seeded import negacyclic_binary

SETS = [SECURITY_128_BIT, SECURITY_80_BIT, SECURITY_UINT4, SECURITY_UINT8]
_KEYS = {}


def _key(p, alpha=None):
    if (p.name, alpha) not in _KEYS:
        sk = SecretKey.new(p, 3)
        pk = sk.packing_key(rng_key=4, alpha=alpha)
        _KEYS[(p.name, alpha)] = (sk, pk, PK.key_rows(p, pk.mask_seed, pk.bodies))
    return _KEYS[(p.name, alpha)]


def _direct(p, rows, cts):
    """The definition input by input: key switch c_m to a TRLWE row (exact int64), times X^j, summed per group."""
    k = rows.astype(np.int64)
    out = np.zeros((-(-len(cts) // N), 2, N), np.int64)
    for m, c in enumerate(cts):
        if not c.any():  # a zero ciphertext has zero digits and a zero body: it adds nothing
            continue
        ks = -(PK.digits(p, c[:p.n]).reshape(-1).astype(np.int64) @ k)
        ks[N] += int(c[p.n])
        g, j = divmod(m, N)
        for h in range(2):
            poly = ks[h * N:(h + 1) * N]
            out[g, h] += np.concatenate([-poly[N - j:], poly[:N - j]])  # X^j poly, negacyclic
    return (out & 0xFFFFFFFF).astype(np.uint32)


@pytest.mark.parametrize("p", SETS, ids=lambda p: p.name)
def test_pack_model_equals_the_direct_definition(p):
    sk, pk, rows = _key(p)
    rng = np.random.default_rng(7)
    small = rng.integers(0, 1 << 32, (6, p.n + 1), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(PK.pack_model(p, pk.mask_seed, pk.bodies, small), _direct(p, rows, small))
    # two groups, the second partial; live inputs on both edges of each group and across the wrap
    sparse = np.zeros((N + 9, p.n + 1), np.uint32)
    for m in (0, 1, 517, N - 1, N, N + 8):
        sparse[m] = rng.integers(0, 1 << 32, p.n + 1, dtype=np.uint64).astype(np.uint32)
    got = PK.pack_model(p, pk.mask_seed, pk.bodies, sparse, rows=rows)
    assert got.shape == (2, 2, N)
    assert np.array_equal(got, _direct(p, rows, sparse))


@pytest.mark.parametrize("p", SETS, ids=lambda p: p.name)
def test_signed_decomposition_identity(p):
    bt, base = p.basebit * p.iks_t, p.base
    edges = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, (1 << (31 - bt)) - 1, 1 << (31 - bt), (1 << 32) - (1 << (31 - bt))]
    words = np.concatenate([np.array(edges, np.uint64), np.random.default_rng(1).integers(0, 1 << 32, 20000, dtype=np.uint64)])
    d = PK.digits(p, words.astype(np.uint32)).astype(np.int64)
    assert d.min() >= -base // 2 and d.max() < base // 2
    abar = ((words + (1 << (31 - bt))) & 0xFFFFFFFF) >> (32 - bt)
    total = (d * PK.gadget(p).astype(np.int64)[None, :]).sum(axis=1) & 0xFFFFFFFF
    assert np.array_equal(total.astype(np.uint64), (abar << (32 - bt)) & 0xFFFFFFFF)


@pytest.mark.parametrize("p", [SECURITY_80_BIT, SECURITY_UINT4], ids=lambda p: p.name)
def test_key_rows_have_the_gadget_phase_at_zero_noise(p):
    sk, pk, rows = _key(p, alpha=0.0)
    assert np.array_equal(rows[:, :N], PK.key_masks(pk.mask_seed, np.arange(p.n * p.iks_t)))
    phase = rows[:, N:] - negacyclic_binary(rows[:, :N], sk.key_lv1)
    r = np.arange(p.n * p.iks_t)
    want = np.zeros_like(phase)
    want[:, 0] = sk.key_lv0[r // p.iks_t] * PK.gadget(p)[r % p.iks_t]
    assert np.array_equal(phase, want)


def test_real_noise_has_the_sets_scale():
    p = SECURITY_80_BIT
    sk, pk, _ = _key(p)
    _, pk0, rows0 = _key(p, alpha=0.0)
    assert pk.mask_seed == pk0.mask_seed  # one rng seed: the same masks, only the noise differs
    e = (pk.bodies - pk0.bodies).reshape(-1).view(np.int32).astype(np.float64) / 2.0 ** 32
    assert 0.9 * p.alpha_lv1 < e.std() < 1.1 * p.alpha_lv1


def test_client_decrypts_model_packed_booleans_and_messages():
    p = SECURITY_128_BIT
    sk, pk, rows = _key(p)
    bits = np.random.default_rng(2).integers(0, 2, 2500).astype(bool)
    packed = PK.pack_model(p, pk.mask_seed, pk.bodies, sk.encrypt_bool(bits, seed=3), rows=rows)
    assert packed.shape == (3, 2, N)
    assert np.array_equal(sk.decrypt_packed_bool(packed, len(bits)), bits)
    # unused slots of the last group: phase 0 plus noise
    rest = sk.packed_phase(packed, 3 * N)[len(bits):].view(np.int32).astype(np.float64) / 2.0 ** 32
    assert np.abs(rest).max() < 2.0 ** -10
    p = SECURITY_UINT4
    sk, pk, rows = _key(p)
    for m in (8, 16):
        msgs = np.arange(1500) % m
        packed = PK.pack_model(p, pk.mask_seed, pk.bodies, sk.encrypt_lwe_message(msgs, m, seed=m), rows=rows)
        assert np.array_equal(sk.decrypt_packed_lwe_message(packed, len(msgs), m), msgs)
    with pytest.raises(ValueError):
        sk.packed_phase(packed, 2 * N + 1)


def test_packing_key_words_and_einval_without_a_device():
    lib = _capi.lib()
    for p in PARAM_SETS.values():
        cp = _capi.Params(p.n, p.l, p.bgbit, p.basebit, p.iks_t)
        w = ctypes.c_size_t()
        assert lib.tfhe_hip_packing_key_words(ctypes.byref(cp), ctypes.byref(w)) == _capi.OK
        assert w.value == p.n * p.iks_t * N
    assert 4 * SECURITY_128_BIT.n * SECURITY_128_BIT.iks_t * N == 25_804_800  # 25.8 MB of bodies
    w = ctypes.c_size_t()
    cp = _capi.Params(700, 3, 6, 2, 9)
    assert lib.tfhe_hip_packing_key_words(None, ctypes.byref(w)) == _capi.EINVAL
    assert lib.tfhe_hip_packing_key_words(ctypes.byref(cp), None) == _capi.EINVAL
    assert lib.tfhe_hip_packing_key_words(ctypes.byref(_capi.Params(0, 3, 6, 2, 9)), ctypes.byref(w)) == _capi.EINVAL
    assert lib.tfhe_hip_packing_key_words(ctypes.byref(_capi.Params(700, 3, 6, 8, 3)), ctypes.byref(w)) == _capi.EINVAL
    for fn in ("load_packing_key", "batch_pack_tlwe", "batch_pack_tlwe_dev", "pool_load_packing_key",
               "pool_batch_pack_tlwe", "pool_batch_pack_tlwe_dev"):
        f = getattr(lib, "tfhe_hip_" + fn)
        args = [0 if t in (ctypes.c_size_t, ctypes.c_int) else None for t in f.argtypes]
        assert f(*args) == _capi.EINVAL, fn
    assert lib.tfhe_hip_packing_key_is_loaded(None) == 0


def test_packing_key_save_load(tmp_path):
    p = SECURITY_UINT4
    _, pk, _ = _key(p)
    assert pk.nbytes == p.n * p.iks_t * N * 4 + 32
    path = tmp_path / "pk.npz"
    pk.save(path)
    back = PK.PackingKey.load(path)
    assert back.params == p and back.mask_seed == pk.mask_seed and np.array_equal(back.bodies, pk.bodies)
    with pytest.raises(ValueError):
        PK.PackingKey.load(path, SECURITY_128_BIT)
    with pytest.raises(ValueError):
        PK.PackingKey(p, bytes(31), pk.bodies)
    with pytest.raises(ValueError):
        PK.PackingKey(p, pk.mask_seed, pk.bodies.reshape(-1)[:-1])
