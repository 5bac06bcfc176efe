"""Seeded (compressed) cloud keys and ciphertexts on the GPU: a CPU-made compressed key expanded by
tfhe_hip_load_compressed_cloud_key is word for word the CPU expansion; tfhe_hip_gen_compressed_cloud_key makes the
same seed and bodies as the CPU compressor at zero noise, at real noise the zero-noise bodies plus the model's noise
sample for sample, and leaves the key load_compressed rebuilds; gates on such a
key are bit-identical to gates on the full key (and to the CPU oracle); key views, pools, seeded inputs, the C++
mirror and the EINVAL cases."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = bytes(range(7, 39))
_CACHE = {}


def _setup(name):
    """(secret key, CPU-compressed key under K, full CloudKey of its CPU expansion with oracle spectra)."""
    if name not in _CACHE:
        import rs_tfhe_amd as R
        from oracle import oracle as O
        from rs_tfhe_amd import seeded as S
        from rs_tfhe_amd.params import PARAM_SETS

        p = PARAM_SETS[name]
        sk = R.SecretKey.new(p, 31)
        ck = sk.compressed_cloud_key(rng_key=K)
        torus = S.expand_bsk_torus(p, ck.mask_seed, ck.bsk_bodies)
        spec = np.stack([O.klemsa_ifft(x) for x in torus.reshape(-1, N)]).reshape(torus.shape)
        full = R.CloudKey(p, spec, S.expand_ksk(p, ck.mask_seed, ck.ksk_bodies), ck.decomposition_offset,
                          ck.blind_rotate_testvec)
        _CACHE[name] = (sk, ck, full, torus)
    return _CACHE[name]


N = 1024


@pytest.mark.parametrize("name", ["SECURITY_128_BIT", "SECURITY_UINT4"])
def test_cpu_compressed_key_expanded_on_the_gpu(name):
    import rs_tfhe_amd as R
    from oracle import oracle as O

    sk, ck, full, torus = _setup(name)
    p = ck.params
    e = R.Engine(p, 0)
    try:
        e.load_compressed_cloud_key(ck)
        ex = e.export_cloud_key()
    finally:
        e.close()
    assert np.array_equal(ex.key_switching_key, full.key_switching_key)
    assert not ex.key_switching_key[:, :, 0, :].any()
    assert ex.decomposition_offset == ck.decomposition_offset
    back = np.stack([O.klemsa_fft(x) for x in ex.bootstrapping_key.reshape(-1, N)]).reshape(torus.shape)
    assert np.array_equal(back, torus)


def test_gpu_generation_equals_cpu_generation():
    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import SECURITY_128_BIT as P

    sk = R.SecretKey.new(P, 32)
    cpu0 = sk.compressed_cloud_key(rng_key=K, alpha_ksk=0.0, alpha_bsk=0.0)
    a, b = R.Engine(P, 0), R.Engine(P, 0)
    try:
        gpu0 = a.gen_compressed_cloud_key(sk.key_lv0, sk.key_lv1, rng_key=K, alpha_ksk=0.0, alpha_bsk=0.0)
        assert gpu0.mask_seed == cpu0.mask_seed
        assert np.array_equal(gpu0.bsk_bodies, cpu0.bsk_bodies)
        assert np.array_equal(gpu0.ksk_bodies, cpu0.ksk_bodies)
        assert gpu0.decomposition_offset == cpu0.decomposition_offset
        # real noise: the generating context holds exactly what a load of its output rebuilds
        ck = a.gen_compressed_cloud_key(sk.key_lv0, sk.key_lv1, rng_key=K)
        b.load_compressed_cloud_key(ck)
        xa, xb = a.export_cloud_key(), b.export_cloud_key()
        assert np.array_equal(xa.bootstrapping_key.view(np.uint64), xb.bootstrapping_key.view(np.uint64))
        assert np.array_equal(xa.key_switching_key, xb.key_switching_key)
        # ... and its noise has the parameter set's scale
        dk = (ck.ksk_bodies - cpu0.ksk_bodies).reshape(-1).view(np.int32)[np.arange(N * P.iks_t * P.base) % P.base != 0]
        db = (ck.bsk_bodies - cpu0.bsk_bodies).reshape(-1).view(np.int32)
        for d, alpha in ((dk, P.alpha_lv0), (db, P.alpha_lv1)):
            d = d.astype(np.float64) / 2.0 ** 32
            assert 0.8 * alpha < d.std() < 1.2 * alpha and np.abs(d).max() < 7 * alpha + 2.0 ** -31
        # ... and IS the model's noise, sample for sample (tests/keygen_model.py): the noise is additive in both bodies,
        # so they are the zero-noise bodies plus f64_to_torus(g) of streams 17 / 19 under K -- off by one LSB only
        # where the long-double sampler marks a sample borderline, at most 16 words in the key
        import keygen_model as KM

        ek, eb = KM.compressed_noise(P, K)
        mb, bb = KM.compare_words(ck.bsk_bodies, cpu0.bsk_bodies + eb.words, eb.border, "SECURITY_128_BIT BSK bodies")
        mk, bk = KM.compare_words(ck.ksk_bodies, cpu0.ksk_bodies + ek.words, ek.border, "SECURITY_128_BIT KSK bodies")
        print(f"KEYGEN SECURITY_128_BIT compressed: mismatches {mb} + {mk}, borderline samples {bb} + {bk}")
        assert mb + mk <= KM.MAX_MISMATCHES
        # GPU-made keys with a drawn generator key differ from call to call
        r1 = a.gen_compressed_cloud_key(sk.key_lv0, sk.key_lv1)
        r2 = a.gen_compressed_cloud_key(sk.key_lv0, sk.key_lv1)
        assert r1.mask_seed != r2.mask_seed
    finally:
        a.close()
        b.close()


def test_gates_on_a_compressed_load_match_the_full_key():
    import rs_tfhe_amd as R
    from oracle import oracle as O

    sk, ck, full, _ = _setup("SECURITY_128_BIT")
    p = ck.params
    rng = np.random.default_rng(5)
    va, vb = rng.integers(0, 2, 4096).astype(bool), rng.integers(0, 2, 4096).astype(bool)
    ca, cb = sk.encrypt_bool(va, seed=1), sk.encrypt_bool(vb, seed=2)
    a, b = R.Engine(p, 0), R.Engine(p, 0)
    try:
        a.load_compressed_cloud_key(ck)
        b.load_cloud_key(full)
        out = a.batch_gate(O.GATE_NAND, ca, cb)
        assert np.array_equal(out, b.batch_gate(O.GATE_NAND, ca, cb))
        assert np.array_equal(sk.decrypt_bool(out), ~(va & vb))
        ock = O.CloudKey.from_arrays(O.SECURITY_128_BIT, full.bootstrapping_key, full.key_switching_key,
                                     full.decomposition_offset, full.blind_rotate_testvec)
        assert np.array_equal(out[:64], O.batch_gate(ock, O.GATE_NAND, ca[:64], cb[:64]))
        for g, f in ((O.GATE_AND, np.logical_and), (O.GATE_XOR, np.logical_xor), (O.GATE_OR, np.logical_or)):
            assert np.array_equal(sk.decrypt_bool(a.batch_gate(g, ca[:256], cb[:256])), f(va[:256], vb[:256]))
        # the single-gate (latency / combining) path after a compressed load
        one = a.batch_gate(O.GATE_NAND, ca[:1], cb[:1])
        assert np.array_equal(one, out[:1])
    finally:
        a.close()
        b.close()


def test_uint4_lut_bootstrap_after_a_compressed_load():
    import rs_tfhe_amd as R
    from rs_tfhe_amd.lut import Generator

    sk, ck, _, _ = _setup("SECURITY_UINT4")
    e = R.Engine(ck.params, 0)
    try:
        e.load_compressed_cloud_key(ck)
        msgs = np.arange(64) % 4
        tv = Generator(4).generate_lookup_table(lambda x: (x + 1) % 4).poly
        out = e.batch_bootstrap(sk.encrypt_lwe_message(msgs, 4, seed=3), testvec=tv)
        assert np.array_equal(sk.decrypt_lwe_message(out, 4), (msgs + 1) % 4)
    finally:
        e.close()


def test_key_views_and_pools():
    import rs_tfhe_amd as R
    from oracle import oracle as O

    sk, ck, full, _ = _setup("SECURITY_128_BIT")
    p = ck.params
    base = R.Engine(p, 0)
    try:
        v1, v2 = base.new_key_view(), base.new_key_view()
        v1.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=9)
        before = v1.export_cloud_key()
        v2.load_compressed_cloud_key(ck)
        after = v1.export_cloud_key()
        assert np.array_equal(before.key_switching_key, after.key_switching_key)
        assert np.array_equal(before.bootstrapping_key.view(np.uint64), after.bootstrapping_key.view(np.uint64))
        ca, cb = sk.encrypt_bool(np.arange(600) % 2 == 0, seed=4), sk.encrypt_bool(np.arange(600) % 3 == 0, seed=5)
        single = v2.batch_gate(O.GATE_NAND, ca, cb)
    finally:
        base.close()
    pool = R.Pool(p, [0, 0])
    try:
        pool.load_compressed_cloud_key(ck)
        m0, m1 = pool.export_cloud_key(0), pool.export_cloud_key(1)
        assert np.array_equal(m0.key_switching_key, m1.key_switching_key)
        assert np.array_equal(m0.bootstrapping_key.view(np.uint64), m1.bootstrapping_key.view(np.uint64))
        assert np.array_equal(m0.key_switching_key, full.key_switching_key)
        assert np.array_equal(pool.batch_gate(O.GATE_NAND, ca, cb), single)
    finally:
        pool.close()


def test_seeded_inputs_expand_on_the_gpu():
    import torch

    import rs_tfhe_amd as R
    from oracle import oracle as O

    sk, ck, _, _ = _setup("SECURITY_128_BIT")
    p = ck.params
    va, vb = np.arange(1000) % 2 == 0, np.arange(1000) % 5 < 2
    sa = sk.encrypt_bool_seeded(va, mask_seed=K, first_index=(1 << 32) - 300, seed=6)
    sb = sk.encrypt_bool_seeded(vb, mask_seed=K, first_index=(1 << 32) + 700, seed=7)
    e = R.Engine(p, 0)
    try:
        e.load_compressed_cloud_key(ck)
        ha = e.expand_seeded(sa)
        assert np.array_equal(ha, sa.expand())
        bodies = torch.from_numpy(sb.bodies.view(np.int32)).to("cuda:0")
        out = torch.empty((len(sb), p.n + 1), dtype=torch.int32, device="cuda:0")
        e.expand_seeded_dev(sb.mask_seed, sb.first_index, bodies, out)
        torch.cuda.synchronize()
        hb = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(hb, sb.expand())
        g = e.batch_gate(O.GATE_NAND, ha, hb)
        assert np.array_equal(g, e.batch_gate(O.GATE_NAND, sa.expand(), sb.expand()))
        assert np.array_equal(sk.decrypt_bool(g), ~(va & vb))
        empty = R.seeded.SeededCiphertexts(p, K, 0, np.zeros(0, np.uint32))
        assert e.expand_seeded(empty).shape == (0, p.n + 1)
        with pytest.raises(ValueError):  # another parameter set's ciphertexts are refused, not expanded to this n
            e.expand_seeded(R.seeded.SeededCiphertexts(R.params.SECURITY_80_BIT, K, 0, np.zeros(4, np.uint32)))
    finally:
        e.close()


@pytest.mark.parametrize("n", [1, 16, 33, 1279])
def test_seeded_expansion_at_the_edges_of_the_row_walk(n):
    """expand_seeded_dev == SeededCiphertexts.expand(), word for word (no noise is drawn), where the wave-per-row walk
    changes path: n = 1 (one word), 16 (exactly one keystream block), 33 (a ragged tail), 1279 (80 blocks: a wave's
    second pass); 1, 17 and 257 rows (below, across and well past the 16 rows of a workgroup, none a multiple of it);
    first_index 0 and 2^32 - 3, where the nonce's high word changes inside the batch."""
    import torch

    import keygen_model as KM
    import rs_tfhe_amd as R

    p = KM.shape_params((n, 1, 10, 2, 2))
    rng = np.random.default_rng(n)
    e = R.Engine(p, 0)
    try:
        for count in (1, 17, 257):
            for first in (0, (1 << 32) - 3):
                sc = R.seeded.SeededCiphertexts(p, K, first, rng.integers(0, 1 << 32, count, dtype=np.uint32))
                bodies = torch.from_numpy(sc.bodies.view(np.int32)).to("cuda:0")
                out = torch.zeros((count, n + 1), dtype=torch.int32, device="cuda:0")
                e.expand_seeded_dev(sc.mask_seed, sc.first_index, bodies, out)
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy().view(np.uint32), sc.expand()), (n, count, first)
    finally:
        e.close()


def test_invalid_arguments_on_a_live_context():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi
    from rs_tfhe_amd.params import SECURITY_80_BIT as P

    e = R.Engine(P, 0)
    try:
        lib, ctx = _capi.lib(), e._ctx
        seed = (ctypes.c_uint8 * 32)()
        k0, k1 = np.zeros(P.n, np.uint32), np.zeros(N, np.uint32)
        bsk, ksk = np.zeros(P.n * 2 * P.l * N, np.uint32), np.zeros(N * P.iks_t * P.base, np.uint32)
        tv = np.zeros(2 * N, np.uint32)
        off = ctypes.c_uint32()
        sp, ptr = ctypes.addressof(seed), (lambda a: a.ctypes.data)
        gen = lib.tfhe_hip_gen_compressed_cloud_key
        assert gen(ctx, ptr(k0), ptr(k1), -1.0, 0.0, None, sp, ptr(bsk), ptr(ksk), ctypes.byref(off)) == _capi.EINVAL
        assert gen(ctx, ptr(k0), ptr(k1), 0.0, -1.0, None, sp, ptr(bsk), ptr(ksk), ctypes.byref(off)) == _capi.EINVAL
        assert gen(ctx, None, ptr(k1), 0.0, 0.0, None, sp, ptr(bsk), ptr(ksk), ctypes.byref(off)) == _capi.EINVAL
        assert gen(ctx, ptr(k0), ptr(k1), 0.0, 0.0, None, None, ptr(bsk), ptr(ksk), ctypes.byref(off)) == _capi.EINVAL
        assert gen(ctx, ptr(k0), ptr(k1), 0.0, 0.0, None, sp, ptr(bsk), ptr(ksk), None) == _capi.EINVAL
        load = lib.tfhe_hip_load_compressed_cloud_key
        assert load(ctx, None, ptr(bsk), ptr(ksk), 0, ptr(tv)) == _capi.EINVAL
        assert load(ctx, sp, None, ptr(ksk), 0, ptr(tv)) == _capi.EINVAL
        assert load(ctx, sp, ptr(bsk), ptr(ksk), 0, None) == _capi.EINVAL
        assert lib.tfhe_hip_key_is_loaded(ctx) == 0
        assert lib.tfhe_hip_expand_seeded_tlwe(ctx, None, 0, ptr(tv), 1, ptr(bsk)) == _capi.EINVAL
        assert lib.tfhe_hip_expand_seeded_tlwe(ctx, sp, 0, None, 1, ptr(bsk)) == _capi.EINVAL
        assert lib.tfhe_hip_expand_seeded_tlwe(ctx, sp, 0, None, 0, None) == _capi.OK
        assert lib.tfhe_hip_expand_seeded_tlwe_dev(ctx, sp, 0, None, 1, None, None) == _capi.EINVAL
        assert lib.tfhe_hip_expand_seeded_tlwe_dev(ctx, sp, 0, None, 0, None, None) == _capi.OK
    finally:
        e.close()


def test_cpp_mirror_compressed_key(tmp_path):
    exe = str(tmp_path / "test_compressed_key")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_compressed_key.cpp"), "-L" + os.path.join(ROOT, "rs-tfhe_amd"),
        "-ltfhe_hip", "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
        "-lamdhip64", "-pthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok:" in r.stdout
