"""Packing key switch on the GPU: tfhe_hip_batch_pack_tlwe equals the integer model (packing.pack_model) word for word
on four parameter sets and on an adversarial key / input pair, packed gate and LUT outputs decrypt on the client, a
packed TRLWE round-trips through sample extraction and the identity key switch, the _dev form on a side stream, key
views, pools and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1024
COUNTS = (1, 7, 1023, 1024, 1025, 3000)
_CACHE = {}


def _setup(name):
    """(secret key, packing key, its key rows) of a parameter set, made once."""
    if name not in _CACHE:
        from rs_tfhe_amd import packing as PK
        from rs_tfhe_amd.client import SecretKey
        from rs_tfhe_amd.params import PARAM_SETS

        p = PARAM_SETS[name]
        sk = SecretKey.new(p, 21)
        pk = sk.packing_key(rng_key=22)
        _CACHE[name] = (sk, pk, PK.key_rows(p, pk.mask_seed, pk.bodies))
    return _CACHE[name]


def _words(p, count, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, (count, p.n + 1), dtype=np.uint64).astype(np.uint32)


def _unsplit_count():
    """A count whose launch does not cut K.  A launch has ceil(count / 32) row blocks times 64 / 8 = 8 column groups
    (the 64 tiles of a key row, 8 a workgroup) and cuts K over workgroups while that is below 4 per CU, as for every
    count of COUNTS on 256 CUs.  The fewest row blocks on the other side are ceil(4 CUs / 8); that many full blocks plus 4
    rows: on 256 CUs 128 * 32 + 4 = 4100 inputs, 129 row blocks, the last with four live rows, and five groups, the
    last partial."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tile_groups = (2 * N // 32) // 8
    count = 32 * -(-4 * cus // tile_groups) + 4
    assert -(-count // 32) * tile_groups >= 4 * cus  # the unsplit side
    return count


@pytest.mark.parametrize("name", ["SECURITY_128_BIT", "SECURITY_80_BIT", "SECURITY_UINT4", "SECURITY_UINT8"])
def test_gpu_pack_equals_the_model(name):
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK

    sk, pk, rows = _setup(name)
    p = sk.params
    e = R.Engine(p, 0)
    try:
        e.load_packing_key(pk)
        assert e.packing_key_is_loaded()
        counts = COUNTS
        if name == "SECURITY_UINT4":  # n = 820: the last 32-coefficient block is partial; base 32, t = 3
            counts += (_unsplit_count(),)
        for count in counts:
            cts = _words(p, count, count)
            got = e.pack(cts)
            assert got.shape == (-(-count // N), 2, N)
            assert np.array_equal(got, PK.pack_model(p, pk.mask_seed, pk.bodies, cts, rows=rows)), count
        assert e.pack(np.zeros((0, p.n + 1), np.uint32)).shape == (0, 2, N)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["SECURITY_128_BIT", "SECURITY_UINT8"])
def test_gpu_pack_adversarial_exactness(name):
    """Bodies all 0x80000000 (every byte plane at its extreme) and inputs whose digits are all -B/2: the largest
    accumulators the bound allows, still word for word."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK

    sk, _, _ = _setup(name)
    p = sk.params
    pk = PK.PackingKey(p, bytes(range(40, 72)), np.full((p.n, p.iks_t, N), 0x80000000, np.uint32))
    bt, half = p.basebit * p.iks_t, p.base // 2
    off = sum(half << (p.basebit * q) for q in range(p.iks_t))
    word = (((1 << bt) - off) % (1 << bt)) << (32 - bt)  # a_bar + off = 0 (mod 2^bt): every digit -B/2
    assert (PK.digits(p, np.array([word], np.uint32)) == -half).all()
    cts = np.full((N + 3, p.n + 1), word, np.uint32)
    cts[:, p.n] = 0x80000000
    e = R.Engine(p, 0)
    try:
        e.load_packing_key(pk)
        assert np.array_equal(e.pack(cts), PK.pack_model(p, pk.mask_seed, pk.bodies, cts))
    finally:
        e.close()


def test_packed_nand_and_lut_outputs_decrypt():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.lut import Generator

    sk, pk, rows = _setup("SECURITY_128_BIT")
    p = sk.params
    ck = sk.cloud_key(seed=5)
    rng = np.random.default_rng(6)
    va, vb = rng.integers(0, 2, 4096).astype(bool), rng.integers(0, 2, 4096).astype(bool)
    out = R.gates.batch_nand(sk.encrypt_bool(va, seed=1), sk.encrypt_bool(vb, seed=2), ck)
    packed = PK.pack(out, ck, pk)
    assert packed.shape == (4, 2, N)
    assert np.array_equal(packed, PK.pack_model(p, pk.mask_seed, pk.bodies, out, rows=rows))
    assert np.array_equal(sk.decrypt_packed_bool(packed, 4096), ~(va & vb))
    assert np.array_equal(PK.pack(out[:5], ck, pk), PK.pack_model(p, pk.mask_seed, pk.bodies, out[:5], rows=rows))
    # UINT4, message modulus 8: LUT outputs
    sk4, pk4, _ = _setup("SECURITY_UINT4")
    e = R.Engine(sk4.params, 0)
    try:
        e.gen_cloud_key(sk4.key_lv0, sk4.key_lv1, seed=7)
        e.load_packing_key(pk4)
        msgs = np.arange(2048) % 8
        f = lambda x: (3 * x + 1) % 8  # noqa: E731
        tv = Generator(8).generate_lookup_table(f).poly
        res = e.batch_bootstrap(sk4.encrypt_lwe_message(msgs, 8, seed=8), testvec=tv)
        assert np.array_equal(sk4.decrypt_packed_lwe_message(e.pack(res), len(msgs), 8), f(msgs))
    finally:
        e.close()


def test_server_round_trip_through_sample_extract_and_key_switch():
    import rs_tfhe_amd as R

    sk, pk, _ = _setup("SECURITY_128_BIT")
    p = sk.params
    e = R.Engine(p, 0)
    try:
        e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=9)
        e.load_packing_key(pk)
        bits = np.random.default_rng(10).integers(0, 2, 1500).astype(bool)
        packed = e.pack(sk.encrypt_bool(bits, seed=11))
        for j in (0, 1, 511, 1023, 1024, 1499):
            lv1 = e.batch_sample_extract(packed[j // N][None], k=j % N)
            back = e.batch_identity_key_switch(lv1)
            assert sk.decrypt_bool(back)[0] == bits[j], j
    finally:
        e.close()


def test_pack_dev_on_a_side_stream_equals_pack():
    import torch

    import rs_tfhe_amd as R

    sk, pk, _ = _setup("SECURITY_UINT4")
    p = sk.params
    cts = _words(p, 2100, 12)
    e = R.Engine(p, 0)
    try:
        e.load_packing_key(pk)
        want = e.pack(cts)
        side = torch.cuda.Stream(device=0)
        t_in = torch.from_numpy(cts.view(np.int32)).to("cuda:0")
        out = torch.full((3, 2, N), -1, dtype=torch.int32, device="cuda:0")
        side.wait_stream(torch.cuda.current_stream(0))
        e.pack_dev(t_in, out, stream=side)
        side.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
        with pytest.raises(ValueError):
            e.pack_dev(t_in, out[:2])
    finally:
        e.close()


def test_key_views_hold_their_own_packing_keys():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi, packing as PK

    sk, pk, rows = _setup("SECURITY_80_BIT")
    p = sk.params
    pk2 = sk.packing_key(rng_key=23)
    cts = _words(p, 1500, 13)
    base = R.Engine(p, 0)
    try:
        v1, v2, v3 = base.new_key_view(), base.new_key_view(), base.new_key_view()
        v1.load_packing_key(pk)
        v2.load_packing_key(pk2)
        o1, o2 = v1.pack(cts), v2.pack(cts)
        assert not np.array_equal(o1, o2)
        assert np.array_equal(o1, PK.pack_model(p, pk.mask_seed, pk.bodies, cts, rows=rows))
        assert np.array_equal(o2, PK.pack_model(p, pk2.mask_seed, pk2.bodies, cts))
        # a cloud-key load (and a generation) leaves the packing key in place
        v1.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=14)
        v1.load_cloud_key(v1.export_cloud_key())
        assert v1.packing_key_is_loaded() and np.array_equal(v1.pack(cts), o1)
        # a handle without one
        assert not v3.packing_key_is_loaded() and not base.packing_key_is_loaded()
        with pytest.raises(_capi.TfheHipError) as ei:
            v3.pack(cts)
        assert ei.value.code == _capi.ENOKEY
        assert _capi.lib().tfhe_hip_batch_pack_tlwe(v3._ctx, None, 0, None) == _capi.ENOKEY
        assert _capi.lib().tfhe_hip_batch_pack_tlwe(v1._ctx, None, 5, None) == _capi.EINVAL
        assert _capi.lib().tfhe_hip_batch_pack_tlwe(v1._ctx, None, 0, None) == _capi.OK
        v1.close()
        assert np.array_equal(v2.pack(cts), o2)
    finally:
        base.close()


def test_pool_host_and_dev_forms_equal_the_single_context():
    import torch

    import rs_tfhe_amd as R

    sk, pk, _ = _setup("SECURITY_128_BIT")
    p = sk.params
    cts = _words(p, 3 * N + 5, 15)
    e = R.Engine(p, 0)
    try:
        e.load_packing_key(pk)
        want = e.pack(cts)
    finally:
        e.close()
    pool = R.Pool(p, [0, 0])
    try:
        pool.load_packing_key(pk)
        assert pool.packing_key_is_loaded()
        assert np.array_equal(pool.pack(cts), want)
        assert np.array_equal(pool.pack(cts[:N]), want[:1])
        t_in = torch.from_numpy(cts.view(np.int32)).to("cuda:0")
        out = torch.zeros((4, 2, N), dtype=torch.int32, device="cuda:0")
        pool.pack_dev(t_in, out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
        out2 = torch.zeros((2, 2, N), dtype=torch.int32, device="cuda:0")
        pool.pack_dev(t_in[:2 * N], out2)
        torch.cuda.synchronize()
        assert np.array_equal(out2.cpu().numpy().view(np.uint32), want[:2])
    finally:
        pool.close()


def test_cpp_mirror_packing(tmp_path):
    sk, pk, _ = _setup("SECURITY_128_BIT")
    p = sk.params
    bits = np.arange(1500) % 3 == 0
    cts = sk.encrypt_bool(bits, seed=16)
    from rs_tfhe_amd import packing as PK

    want = PK.pack_model(p, pk.mask_seed, pk.bodies, cts)
    blob = tmp_path / "case.bin"
    with open(blob, "wb") as f:
        f.write(pk.mask_seed)
        f.write(np.uint64(len(cts)).tobytes())
        for a in (pk.bodies, cts, want, sk.key_lv1.astype(np.uint32)):
            f.write(np.ascontiguousarray(a, np.uint32).tobytes())
        f.write(bits.astype(np.uint8).tobytes())
    exe = str(tmp_path / "test_packing")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_packing.cpp"), "-L" + os.path.join(ROOT, "rs-tfhe_amd"),
        "-ltfhe_hip", "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
        "-lamdhip64", "-pthread"])
    r = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok:" in r.stdout
