"""Every route by which a key becomes current on a handle (csrc/key_change.hpp), one after the other on the same
handle and alternating between two unrelated keys, so that a step a route forgets -- stale byte planes of the
matrix-core key switch, a flag left set or cleared, a front-end lane still on the old key -- decrypts wrongly or
differs from the oracle.  After every route the same check: a 64-ciphertext NAND (64 = ks_mfma_min, the smallest batch
that reads the byte planes) and a 2-ciphertext NAND (the merged front end), word for word against the CPU oracle under
the key that should be current, all 64 decrypted, and the loaded flags."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1024
K = bytes(range(50, 82))
_CACHE = {}


class _Key:
    """A key a handle may hold: the secret key its inputs are encrypted under, 64 encrypted operand pairs, and the
    oracle's NAND of the words the check compares (the first 8; the 2-ciphertext call is the first 2 of them)."""

    def __init__(self, O, sk, ock, seed):
        rng = np.random.default_rng(seed)
        self.va, self.vb = rng.integers(0, 2, 64).astype(bool), rng.integers(0, 2, 64).astype(bool)
        self.sk = sk
        self.ca, self.cb = sk.encrypt_bool(self.va, seed=seed + 1), sk.encrypt_bool(self.vb, seed=seed + 2)
        self.want = O.batch_gate(ock, O.GATE_NAND, self.ca[:8], self.cb[:8])


def _oracle_key(O, k):
    """A product-side CloudKey (an exported or CPU-expanded one) as the oracle's."""
    return O.CloudKey.from_arrays(O.SECURITY_128_BIT, k.bootstrapping_key, k.key_switching_key, k.decomposition_offset,
                                  k.blind_rotate_testvec)


def _keys(O, keys128):
    """A: the oracle's own key.  B: a CPU-compressed key (rs-tfhe_amd/seeded.py) and its CPU expansion, under another
    secret key.  Made once for the module (B's expansion is shared with test_gpu_compressed_key)."""
    if "AB" not in _CACHE:
        from tests.test_gpu_compressed_key import _setup
        from tests.test_gpu_parity import _cloud_key

        sk_a, ock_a = keys128
        sk_b, comp_b, full_b, _ = _setup("SECURITY_128_BIT")
        _CACHE["AB"] = {"A": _Key(O, sk_a, ock_a, 8100), "B": _Key(O, sk_b, _oracle_key(O, full_b), 8200),
                        "load_a": _cloud_key(ock_a), "load_b": full_b, "comp_b": comp_b}
    return _CACHE["AB"]


def _flags(handle):
    lib = handle._lib
    members = range(len(handle)) if hasattr(handle, "devices") else range(1)
    return [(lib.tfhe_hip_key_is_loaded(handle._member_ctx(m)), lib.tfhe_hip_reenc_key_is_loaded(handle._member_ctx(m)))
            for m in members]


def _check(O, handle, key, where):
    out = handle.batch_gate(O.GATE_NAND, key.ca, key.cb)
    two = handle.batch_gate(O.GATE_NAND, key.ca[:2], key.cb[:2])
    assert np.array_equal(out[:8], key.want), where
    assert np.array_equal(two, key.want[:2]), where
    assert np.array_equal(key.sk.decrypt_bool(out), ~(key.va & key.vb)), where
    assert all(f == (1, 0) for f in _flags(handle)), where


def test_every_route_in_sequence_on_one_handle(O, keys128):
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi

    ks = _keys(O, keys128)
    A, B = ks["A"], ks["B"]
    P = R.params.SECURITY_128_BIT
    eng, src = R.Engine(P, 0), R.Engine(P, 0)
    try:
        assert _flags(eng) == [(0, 0)]
        eng.load_cloud_key(ks["load_a"])
        _check(O, eng, A, "load A")
        eng.load_compressed_cloud_key(ks["comp_b"])
        _check(O, eng, B, "compressed load B")
        # generated keys: the oracle runs on the exported key, under the secret key the generation was given
        eng.gen_cloud_key(A.sk.key_lv0, A.sk.key_lv1, seed=8301)
        _check(O, eng, _Key(O, A.sk, _oracle_key(O, eng.export_cloud_key()), 8310), "gen_cloud_key")
        eng.gen_compressed_cloud_key(B.sk.key_lv0, B.sk.key_lv1, rng_key=K)
        _check(O, eng, _Key(O, B.sk, _oracle_key(O, eng.export_cloud_key()), 8320), "gen_compressed_cloud_key")
        eng.load_cloud_key(ks["load_a"])
        _check(O, eng, A, "load A again")
        # buffers + device-to-device copy + adopt
        src.load_cloud_key(ks["load_b"])
        *from_b, off = src.cloud_key_device_tensors()
        *into, _ = eng.cloud_key_device_tensors()
        for d, s in zip(into, from_b):
            assert d.shape == s.shape
            d.copy_(s)
        torch.cuda.synchronize()
        eng.adopt_cloud_key(off)
        _check(O, eng, B, "adopt B")
        # a re-encryption key takes the key switch's buffer: no cloud key any more
        bob = O.SecretKey(O.SECURITY_128_BIT, 8401)
        rk = O.gen_reenc_key(O.SECURITY_128_BIT, A.sk.key_lv0, 8402, key_to=bob.key_lv0)
        eng.load_reenc_key(rk)
        assert _flags(eng) == [(0, 1)]
        for count in (64, 2):
            with pytest.raises(_capi.TfheHipError, match="cloud key not loaded"):
                eng.batch_gate(O.GATE_NAND, A.ca[:count], A.cb[:count])
        re = eng.batch_reencrypt(A.ca)
        assert np.array_equal(re, O.reencrypt_tlwe_lv0(O.SECURITY_128_BIT, rk, A.ca))
        assert np.array_equal(bob.decrypt_bool(re), A.va)
        eng.load_cloud_key(ks["load_a"])
        assert not eng.reenc_key_is_loaded()
        with pytest.raises(_capi.TfheHipError, match="re-encryption key not loaded"):
            eng.batch_reencrypt(A.ca)
        _check(O, eng, A, "load A after the re-encryption key")
    finally:
        eng.close()
        src.close()


def test_refused_changes_and_the_packing_key_leave_what_is_loaded(O, keys128):
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi

    ks = _keys(O, keys128)
    A, B = ks["A"], ks["B"]
    P = R.params.SECURITY_128_BIT
    base = R.Engine(P, 0)
    try:
        base.load_cloud_key(ks["load_b"])  # the bystander: the parent's key answers throughout
        view, fresh = base.new_key_view(), base.new_key_view()
        view.load_cloud_key(ks["load_a"])
        lib = _capi.lib()
        k0, k1 = A.sk.key_lv0, A.sk.key_lv1
        comp = ks["comp_b"]
        seed = (ctypes.c_uint8 * 32).from_buffer_copy(comp.mask_seed)
        tv = np.ascontiguousarray(comp.blind_rotate_testvec, np.uint32)
        bodies = np.ascontiguousarray(comp.ksk_bodies, np.uint32)

        def refused(what, text, call):
            with pytest.raises(_capi.TfheHipError, match=text):
                call()
            _check(O, view, A, "after a refused " + what)
            _check(O, base, B, "the parent after a refused " + what)

        refused("load_cloud_key", "null key pointer",
                lambda: view._call("load_cloud_key", None, None, ctypes.c_uint32(0), None))
        refused("load_compressed_cloud_key", "null key pointer",
                lambda: view._call("load_compressed_cloud_key", ctypes.addressof(seed), None, bodies.ctypes.data,
                                   ctypes.c_uint32(0), tv.ctypes.data))
        refused("gen_cloud_key", "negative noise parameter", lambda: view.gen_cloud_key(k0, k1, seed=1, alpha_ksk=-1.0))
        refused("gen_cloud_key_with_key", "negative noise parameter",
                lambda: view.gen_cloud_key(k0, k1, rng_key=K, alpha_bsk=-1.0))
        refused("gen_cloud_key_secure", "negative noise parameter", lambda: view.gen_cloud_key(k0, k1, alpha_ksk=-1.0))
        refused("gen_compressed_cloud_key", "negative noise parameter",
                lambda: view.gen_compressed_cloud_key(k0, k1, rng_key=K, alpha_bsk=-1.0))
        refused("adopt_cloud_key", "tfhe_hip_adopt_cloud_key before tfhe_hip_cloud_key_buffers",
                lambda: fresh.adopt_cloud_key(0))
        assert lib.tfhe_hip_key_is_loaded(fresh._ctx) == 0
        # the packing key lies beside the cloud key: a cloud-key change leaves it, flag and planes
        view.load_packing_key(B.sk.packing_key(rng_key=83))
        packed = view.pack(A.ca[:32])
        view.load_cloud_key(ks["load_b"])
        assert view.packing_key_is_loaded()
        assert np.array_equal(view.pack(A.ca[:32]), packed)
        _check(O, view, B, "A -> B beside a packing key")
        _check(O, base, B, "the parent at the end")
    finally:
        base.close()


@pytest.mark.parametrize("mode,devices,transport", [
    ("0", [0, 0], "peer-copy"),
    ("2", [0, 0], "peer-copy"),  # a communicator takes each device once: two members on one GPU are peer copies whatever the mode
    ("2", [0], "rccl"),          # the broadcast on a communicator of one rank, as the other pool tests run it on one GPU
    ("2", [0, 1], "rccl"),       # the broadcast between two members (prepare_replica / finish_replica)
])
def test_pool_replication_makes_every_member_current(O, keys128, monkeypatch, mode, devices, transport):
    """Both replications, A then B on one pool, checked through the pool handle and through every member borrowed with
    tfhe_hip_pool_ctx.  The transport a case takes is asserted, so that none of them runs another route than it names."""
    import rs_tfhe_amd as R

    if len(set(devices)) > R.engine.device_count():
        pytest.skip("a broadcast between two members needs two GPUs (a communicator takes each device once)")
    ks = _keys(O, keys128)
    monkeypatch.setenv("TFHE_HIP_POOL_RCCL", mode)
    pool = R.Pool(R.params.SECURITY_128_BIT, devices)
    try:
        for name in ("A", "B"):
            pool.load_cloud_key(ks["load_a" if name == "A" else "load_b"])
            assert pool.key_transport == transport
            _check(O, pool, ks[name], f"pool after load {name}")
            for m in range(len(devices)):
                _check(O, R.Engine.from_pool(pool, m), ks[name], f"member {m} after load {name}")
    finally:
        pool.close()
