"""Encrypted-table key switch and the tree bootstrap on the GPU: tfhe_hip_batch_pack_table equals the integer model
(packing.table_model) word for word on four parameter sets, on both sides of the launch plan's K split and on an
adversarial key / input pair; the composite tfhe_hip_batch_bootstrap_bivariate equals the CPU oracle's composition at
SECURITY_128_BIT and the same steps made by hand on the same handle, decrypts to f(x, y), and is unchanged by chunking,
the _dev form and a pool; the error codes; the C++ mirror."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1024
# a block straddling ciphertexts (m < 32), a partial last block, a ciphertext spanning several blocks (m > 32), W = 2
SHAPES = ((2, 1), (2, 17), (4, 9), (16, 3), (16, 33), (64, 1), (64, 3), (512, 1))
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


def _keyed(name):
    """An engine of the set with a generated cloud key and the packing key of _setup (the caller closes it)."""
    import rs_tfhe_amd as R

    sk, pk, _ = _setup(name)
    e = R.Engine(sk.params, 0)
    e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=7)
    e.load_packing_key(pk)
    return e


def _words(shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def _table(m, seed):
    T = np.random.default_rng(seed).integers(0, m, (m, m))
    return T, (lambda x, y: int(T[x, y]))


# ---- pack_table against table_model ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SECURITY_128_BIT", "SECURITY_80_BIT", "SECURITY_UINT4", "SECURITY_UINT8"])
def test_gpu_pack_table_equals_the_model(name):
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK

    sk, pk, rows = _setup(name)
    p = sk.params
    e = R.Engine(p, 0)
    try:
        e.load_packing_key(pk)  # no cloud key: the call needs none
        for m, count in SHAPES:
            s1 = _words((m, count, p.n + 1), 100 * m + count)
            got = e.pack_table(s1, m)
            assert got.shape == (count, 2, N)
            assert np.array_equal(got, PK.table_model(p, pk.mask_seed, pk.bodies, s1, m, rows=rows)), (m, count)
        assert e.pack_table(np.zeros((4, 0, p.n + 1), np.uint32), 4).shape == (0, 2, N)
    finally:
        e.close()


@pytest.mark.parametrize("count", [500, 512])
def test_gpu_pack_table_on_both_sides_of_the_k_split(count):
    """SECURITY_UINT4, m = 16: 8,000 rows are 250 row blocks (1,000 workgroups, under four per CU: K is split), 8,192
    rows are 256 (the unsplit launch)."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK

    sk, pk, rows = _setup("SECURITY_UINT4")
    p = sk.params
    s1 = _words((16, count, p.n + 1), count)
    e = R.Engine(p, 0)
    try:
        e.load_packing_key(pk)
        got = e.pack_table(s1, 16)
    finally:
        e.close()
    assert np.array_equal(got, PK.table_model(p, pk.mask_seed, pk.bodies, s1, 16, rows=rows))


@pytest.mark.parametrize("name", ["SECURITY_128_BIT", "SECURITY_UINT8"])
def test_gpu_pack_table_adversarial_exactness(name):
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
    e = R.Engine(p, 0)
    try:
        e.load_packing_key(pk)
        for m, count in ((2, 3), (16, 5), (512, 1)):
            s1 = np.full((m, count, p.n + 1), word, np.uint32)
            s1[..., p.n] = 0x80000000
            assert np.array_equal(e.pack_table(s1, m), PK.table_model(p, pk.mask_seed, pk.bodies, s1, m)), (m, count)
    finally:
        e.close()


def test_gpu_pack_table_trivial_inputs_and_dev_form():
    """a = 0, b = v_x gives the generator's table of v, key-free; the _dev form on a side stream equals the host form."""
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd.lut import Generator

    sk, pk, _ = _setup("SECURITY_UINT4")
    p = sk.params
    e = R.Engine(p, 0)
    try:
        e.load_packing_key(pk)
        for m in (2, 4, 64, 512):
            v = _words((m, 3), 40 + m)
            s1 = np.zeros((m, 3, p.n + 1), np.uint32)
            s1[..., p.n] = v
            got = e.pack_table(s1, m)
            for c in range(3):
                assert not got[c, 0].any()
                assert np.array_equal(got[c, 1], Generator(m)._assemble(v[:, c]).poly[1]), (m, c)
        s1 = _words((8, 41, p.n + 1), 50)
        want = e.pack_table(s1, 8)
        side = torch.cuda.Stream(device=0)
        t_in = _t(s1)
        out = torch.full((41, 2, N), -1, dtype=torch.int32, device="cuda:0")
        side.wait_stream(torch.cuda.current_stream(0))
        e.pack_table_dev(t_in, 8, out, stream=side)
        side.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
        with pytest.raises(ValueError):
            e.pack_table_dev(t_in, 4, out)
    finally:
        e.close()


# ---- the composite ---------------------------------------------------------------------------------------------------
def test_composite_equals_the_oracle_composition(O):
    """SECURITY_128_BIT (the set whose blind rotation is the oracle's word for word), m = 2, k = 1, count = 8, under the
    engine's exported key: stage 1 on the oracle, table_model, then the oracle's per-ciphertext bootstrap."""
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.lut import Generator

    sk, pk, rows = _setup("SECURITY_128_BIT")
    p = sk.params
    m, count = 2, 8
    e = _keyed("SECURITY_128_BIT")
    try:
        ck = e.export_cloud_key()
        ock = O.CloudKey.from_arrays(O.SECURITY_128_BIT, ck.bootstrapping_key, ck.key_switching_key, ck.decomposition_offset,
                                     ck.blind_rotate_testvec)
        T, f = _table(m, 60)
        rng = np.random.default_rng(61)
        xs, ys = rng.integers(0, m, count), rng.integers(0, m, count)
        cx, cy = sk.encrypt_lwe_message(xs, m, seed=62), sk.encrypt_lwe_message(ys, m, seed=63)
        tabs = Generator(m).generate_bivariate_tables(f)
        stage1 = np.stack([O.batch_bootstrap(ock, cy, testvec=tabs[x]) for x in range(m)])
        tv = PK.table_model(p, pk.mask_seed, pk.bodies, stage1, m, rows=rows)
        for ks in (True, False):
            want = O.batch_bootstrap(ock, cx, testvec=tv, keyswitch=ks)
            got = e.batch_bootstrap_bivariate(cx, cy, tabs, m, n_luts=1, keyswitch=ks)
            assert np.array_equal(got, want), ks
        assert np.array_equal(sk.decrypt_lwe_message(e.batch_bootstrap_bivariate(cx, cy, tabs, m), m), T[xs, ys])
    finally:
        e.close()


def _by_hand(e, cx, cy, tabs, m, k, keyswitch=True):
    """The composite's definition through the existing calls plus pack_table, on the same handle."""
    stage1 = np.concatenate([e.batch_lincomb_bootstrap_many(1, cy, 0, None, 0, tabs[j], n_luts=k) for j in range(m // k)])
    return e.batch_bootstrap(cx, testvec=e.pack_table(stage1, m), keyswitch=keyswitch)


def test_composite_equals_the_steps_by_hand_and_decrypts(monkeypatch):
    """SECURITY_UINT4, random 2-D tables: the words of the composition by hand, every output decrypting to f(x, y) (the
    CPU reference has no error in 64 .. 128 inputs at these shapes, worst phase error 0.24 of the half-interval at
    m = 16: DESIGN section 9), a count above a forced chunk of 16, and the _dev form."""
    import torch

    from rs_tfhe_amd.lut import Generator

    sk, _, _ = _setup("SECURITY_UINT4")
    p = sk.params
    e = _keyed("SECURITY_UINT4")
    try:
        for m, k, count in ((4, 4, 64), (16, 1, 64), (8, 2, 33)):
            T, f = _table(m, 70 + m)
            rng = np.random.default_rng(71 + m)
            xs, ys = rng.integers(0, m, count), rng.integers(0, m, count)
            cx, cy = sk.encrypt_lwe_message(xs, m, seed=72 + m), sk.encrypt_lwe_message(ys, m, seed=73 + m)
            tabs = Generator(m).generate_bivariate_tables(f, n_luts=k)
            got = e.batch_bootstrap_bivariate(cx, cy, tabs, m, n_luts=k)
            assert np.array_equal(got, _by_hand(e, cx, cy, tabs, m, k)), (m, k)
            assert np.array_equal(sk.decrypt_lwe_message(got, m), T[xs, ys]), (m, k)
            nks = e.batch_bootstrap_bivariate(cx, cy, tabs, m, n_luts=k, keyswitch=False)
            assert np.array_equal(nks, _by_hand(e, cx, cy, tabs, m, k, keyswitch=False)), (m, k)
            # chunks of 16: 33 = 16 + 16 + 1, 64 = 4 x 16 -- chunking changes no word
            monkeypatch.setenv("TFHE_HIP_BIVARIATE_CHUNK", "16")
            assert np.array_equal(e.batch_bootstrap_bivariate(cx, cy, tabs, m, n_luts=k), got), (m, k, "chunked")
            monkeypatch.delenv("TFHE_HIP_BIVARIATE_CHUNK")
            out = torch.full((count, p.n + 1), -1, dtype=torch.int32, device="cuda:0")
            e.batch_bootstrap_bivariate_dev(_t(cx), _t(cy), _t(tabs), m, out, n_luts=k)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), got), (m, k, "dev")
    finally:
        e.close()


def test_composite_uint8_m16_decrypts():
    from rs_tfhe_amd.lut import Generator

    sk, _, _ = _setup("SECURITY_UINT8")
    m, count = 16, 32
    e = _keyed("SECURITY_UINT8")
    try:
        T, f = _table(m, 80)
        rng = np.random.default_rng(81)
        xs, ys = rng.integers(0, m, count), rng.integers(0, m, count)
        cx, cy = sk.encrypt_lwe_message(xs, m, seed=82), sk.encrypt_lwe_message(ys, m, seed=83)
        got = e.batch_bootstrap_bivariate(cx, cy, Generator(m).generate_bivariate_tables(f), m)
        assert np.array_equal(sk.decrypt_lwe_message(got, m), T[xs, ys])
    finally:
        e.close()


def test_bootstrap_func2_convenience():
    from rs_tfhe_amd import packing as PK

    sk, pk, _ = _setup("SECURITY_UINT4")
    m = 4
    T, f = _table(m, 90)
    rng = np.random.default_rng(91)
    xs, ys = rng.integers(0, m, 20), rng.integers(0, m, 20)
    ck = sk.cloud_key(seed=5)
    out = PK.bootstrap_func2(sk.encrypt_lwe_message(xs, m, seed=92), sk.encrypt_lwe_message(ys, m, seed=93), f, m, ck, pk,
                             n_luts=2)
    assert np.array_equal(sk.decrypt_lwe_message(out, m), T[xs, ys])


def test_errors():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi

    sk, pk, _ = _setup("SECURITY_UINT4")
    p = sk.params
    lib = _capi.lib()
    w = p.n + 1
    cts = _words((4, w), 95)
    s1 = _words((4, 4, w), 96)
    tabs = _words((4, 2, N), 97)
    out, tout = np.empty((4, w), np.uint32), np.empty((4, 2, N), np.uint32)
    ptr = lambda a: a.ctypes.data  # noqa: E731
    e = R.Engine(p, 0)
    try:
        # nothing loaded: ENOKEY from both (count 0 included)
        assert lib.tfhe_hip_batch_pack_table(e._ctx, ptr(s1), 4, 4, ptr(tout)) == _capi.ENOKEY
        assert lib.tfhe_hip_batch_pack_table(e._ctx, None, 4, 0, None) == _capi.ENOKEY
        assert lib.tfhe_hip_batch_bootstrap_bivariate(e._ctx, ptr(cts), ptr(cts), ptr(tabs), 4, 1, 1, ptr(out), 4) == _capi.ENOKEY
        # the packing key alone: pack_table runs, the composite still lacks the cloud key
        e.load_packing_key(pk)
        assert lib.tfhe_hip_batch_pack_table(e._ctx, ptr(s1), 4, 4, ptr(tout)) == _capi.OK
        assert lib.tfhe_hip_batch_bootstrap_bivariate(e._ctx, ptr(cts), ptr(cts), ptr(tabs), 4, 1, 1, ptr(out), 4) == _capi.ENOKEY
        # the cloud key alone (a view of its own): the composite lacks the packing key
        v = e.new_key_view()
        v.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=7)
        assert lib.tfhe_hip_batch_bootstrap_bivariate(v._ctx, ptr(cts), ptr(cts), ptr(tabs), 4, 1, 1, ptr(out), 4) == _capi.ENOKEY
        with pytest.raises(_capi.TfheHipError) as ei:
            v.batch_bootstrap_bivariate(cts, cts, tabs, 4)
        assert ei.value.code == _capi.ENOKEY
        v.load_packing_key(pk)
        assert lib.tfhe_hip_batch_bootstrap_bivariate(v._ctx, ptr(cts), ptr(cts), ptr(tabs), 4, 1, 1, ptr(out), 4) == _capi.OK
        for m in (0, 1, 3, 1024):
            assert lib.tfhe_hip_batch_pack_table(v._ctx, ptr(s1), m, 4, ptr(tout)) == _capi.EINVAL, m
            assert lib.tfhe_hip_batch_pack_table_dev(v._ctx, None, m, 0, None, None) == _capi.EINVAL, m
            assert lib.tfhe_hip_batch_bootstrap_bivariate(v._ctx, ptr(cts), ptr(cts), ptr(tabs), m, 1, 1, ptr(out), 4) == _capi.EINVAL, m
        for k in (0, 3, 16):
            assert lib.tfhe_hip_batch_bootstrap_bivariate(v._ctx, ptr(cts), ptr(cts), ptr(tabs), 4, k, 1, ptr(out), 4) == _capi.EINVAL, k
            assert lib.tfhe_hip_batch_bootstrap_bivariate_dev(v._ctx, None, None, ptr(tabs), 4, k, 1, None, 0, None) == _capi.EINVAL, k
        assert lib.tfhe_hip_batch_bootstrap_bivariate(v._ctx, ptr(cts), ptr(cts), ptr(tabs), 4, 8, 1, ptr(out), 4) == _capi.EINVAL  # k > m
        assert lib.tfhe_hip_batch_bootstrap_bivariate(v._ctx, ptr(cts), ptr(cts), None, 4, 1, 1, ptr(out), 4) == _capi.EINVAL
        assert lib.tfhe_hip_batch_bootstrap_bivariate(v._ctx, None, ptr(cts), ptr(tabs), 4, 1, 1, ptr(out), 4) == _capi.EINVAL
        assert lib.tfhe_hip_batch_pack_table(v._ctx, None, 4, 4, ptr(tout)) == _capi.EINVAL
        # count == 0
        assert lib.tfhe_hip_batch_pack_table(v._ctx, None, 4, 0, None) == _capi.OK
        assert lib.tfhe_hip_batch_pack_table_dev(v._ctx, None, 4, 0, None, None) == _capi.OK
        assert lib.tfhe_hip_batch_bootstrap_bivariate(v._ctx, None, None, ptr(tabs), 4, 1, 1, None, 0) == _capi.OK
        assert lib.tfhe_hip_batch_bootstrap_bivariate_dev(v._ctx, None, None, ptr(tabs), 4, 1, 1, None, 0, None) == _capi.OK
    finally:
        e.close()


@pytest.mark.parametrize("members", [1, 2])
def test_pool_composite_equals_the_engine(members):
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi
    from rs_tfhe_amd.lut import Generator

    sk, pk, _ = _setup("SECURITY_UINT4")
    m, k = 4, 2
    T, f = _table(m, 110)
    rng = np.random.default_rng(111)
    xs, ys = rng.integers(0, m, 600), rng.integers(0, m, 600)
    cx, cy = sk.encrypt_lwe_message(xs, m, seed=112), sk.encrypt_lwe_message(ys, m, seed=113)
    tabs = Generator(m).generate_bivariate_tables(f, n_luts=k)
    e = _keyed("SECURITY_UINT4")
    try:
        ck = e.export_cloud_key()
        want = e.batch_bootstrap_bivariate(cx, cy, tabs, m, n_luts=k)
    finally:
        e.close()
    pool = R.Pool(sk.params, [0] * members)
    try:
        pool.load_cloud_key(ck)
        with pytest.raises(_capi.TfheHipError) as ei:  # no packing key yet
            pool.batch_bootstrap_bivariate(cx[:33], cy[:33], tabs, m, n_luts=k)
        assert ei.value.code == _capi.ENOKEY
        pool.load_packing_key(pk)
        for count in (33, 600):  # one member's call, and a batch cut over the members
            got = pool.batch_bootstrap_bivariate(cx[:count], cy[:count], tabs, m, n_luts=k)
            assert np.array_equal(got, want[:count]), count
        with pytest.raises(_capi.TfheHipError) as ei:
            pool.batch_bootstrap_bivariate(cx[:33], cy[:33], tabs, m, n_luts=3)
        assert ei.value.code == _capi.EINVAL
    finally:
        pool.close()


def test_cpp_bivariate_program(tmp_path):
    """tests/cpp/test_bivariate.cpp: Engine::pack_table against the model's words and Engine::bootstrap_bivariate against
    the steps made by hand, SECURITY_UINT4, m = 8, k = 2, 24 inputs; the packing key and the model's case travel in a file."""
    from rs_tfhe_amd import packing as PK
    from test_table_host import build_cpp_bivariate

    sk, pk, rows = _setup("SECURITY_UINT4")
    p = sk.params
    m, k, count, tables = 8, 2, 24, 5
    s1 = _words((m, tables, p.n + 1), 120)
    want = PK.table_model(p, pk.mask_seed, pk.bodies, s1, m, rows=rows)
    blob = tmp_path / "case.bin"
    with open(blob, "wb") as f:
        f.write(pk.mask_seed)
        f.write(np.array([m, k, count, tables], np.uint64).tobytes())
        for a in (pk.bodies, sk.key_lv0, sk.key_lv1, s1, want):
            f.write(np.ascontiguousarray(a, np.uint32).tobytes())
    exe = build_cpp_bivariate(str(tmp_path))
    r = subprocess.run([exe, str(blob)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test_bivariate ok" in r.stdout
