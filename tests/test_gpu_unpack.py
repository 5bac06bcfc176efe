"""Unpacking key switch on the GPU: tfhe_hip_batch_unpack_trlwe equals the oracle's sample_extract_index followed by
identity_key_switching word for word on four parameter sets (under the engine's own exported key), with and without a
selection, under every key-switch kernel a set can run, through the host, _dev and pool forms; gate outputs survive
pack_dev -> unpack_dev on the device, client-packed inputs feed a gate, and the error codes."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1024
COUNTS = (1, 7, 1024, 1025, 3000)
BASE_GROUPS = 3  # distinct groups of random words: the oracle's share of a case is BASE_GROUPS * N rows, made once a set
KEY_SEED = 33
_CACHE = {}


def _case(O, name):
    """(client secret key, oracle cloud key of the engine's generated key, [3][2][N] random TRLWE words, the oracle's
    unpacking of all their 3 N slots), made once per parameter set."""
    if name not in _CACHE:
        import rs_tfhe_amd as R
        from rs_tfhe_amd.client import SecretKey
        from rs_tfhe_amd.params import PARAM_SETS

        p = PARAM_SETS[name]
        sk = SecretKey.new(p, 31)
        e = R.Engine(p, 0)
        try:
            e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=KEY_SEED)
            ck = e.export_cloud_key()
        finally:
            e.close()
        ock = O.CloudKey.from_arrays(getattr(O, name), ck.bootstrapping_key, ck.key_switching_key, ck.decomposition_offset,
                                     ck.blind_rotate_testvec)
        trlwe = np.random.default_rng(32).integers(0, 1 << 32, (BASE_GROUPS, 2, N), dtype=np.uint32)
        # the negation's and the rounding's edges; at `half` Torus::MAX - a and 0 - a round to different digits
        half = 1 << (31 - p.basebit * p.iks_t)
        trlwe[:, 0, :6] = (0, 1 << 31, 0xFFFFFFFF, half - 1, half, 3 * half)
        rows = np.stack([O.sample_extract_index(trlwe[s // N], s % N) for s in range(BASE_GROUPS * N)])
        _CACHE[name] = (sk, ock, trlwe, O.batch_identity_key_switching(ock, rows))
    return _CACHE[name]


def _engine(name):
    import rs_tfhe_amd as R

    sk = _CACHE[name][0]
    e = R.Engine(sk.params, 0)
    e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=KEY_SEED)  # the seeded generator: the key _case exported
    return e


def _selection(groups, count, seed):
    """Slots in any order with duplicates, the first and the last slot of the input among them."""
    s = np.random.default_rng(seed).integers(0, groups * N, max(count, 4)).astype(np.uint32)
    s[:4] = (groups * N - 1, groups * N - 1, 0, N - 1)
    return s[:count]


@pytest.mark.parametrize("name", ["SECURITY_128_BIT", "SECURITY_80_BIT", "SECURITY_UINT4", "SECURITY_UINT8"])
def test_gpu_unpack_equals_the_oracle_composition(O, name):
    sk, ock, trlwe, want = _case(O, name)
    p = sk.params
    e = _engine(name)
    try:
        for count in COUNTS:
            got = e.unpack(trlwe, count)
            assert got.shape == (count, p.n + 1)
            assert np.array_equal(got, want[:count]), count
            slots = _selection(BASE_GROUPS, count, count)
            assert np.array_equal(e.unpack(trlwe, slots=slots), want[slots]), count
        assert np.array_equal(e.unpack(trlwe), want)  # count=None: every slot
        assert e.unpack(trlwe, 0).shape == (0, p.n + 1)
    finally:
        e.close()


def test_gpu_unpack_65536_slots(O):
    """64 groups, each one of the three base groups (in no regular order), so every one of the 65,536 rows has its oracle
    words; then a selection across all 64 groups."""
    sk, ock, trlwe, want = _case(O, "SECURITY_128_BIT")
    which = np.random.default_rng(9).integers(0, BASE_GROUPS, 64)
    assert len(set(zip(which[:-1].tolist(), which[1:].tolist()))) == BASE_GROUPS ** 2  # every neighbour pair occurs
    big = np.ascontiguousarray(trlwe[which])
    ref = want.reshape(BASE_GROUPS, N, -1)[which].reshape(64 * N, -1)
    e = _engine("SECURITY_128_BIT")
    try:
        assert np.array_equal(e.unpack(big, 65536), ref)
        slots = _selection(64, 5000, 64)
        assert np.array_equal(e.unpack(big, slots=slots), ref[slots])
    finally:
        e.close()


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import rs_tfhe_amd as R
from rs_tfhe_amd.client import SecretKey
from rs_tfhe_amd.params import PARAM_SETS
name, kernel, path = sys.argv[2:5]
p = PARAM_SETS[name]
z = np.load(path)
sk = SecretKey.new(p, 31)
e = R.Engine(p, 0)
e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=int(z["key_seed"]))
assert ("key_switch=" + kernel) in e.describe_dispatch(1025), e.describe_dispatch(1025)
np.savez(path + ".out.npz", plain=e.unpack(z["trlwe"], 1025), small=e.unpack(z["trlwe"], 7), sel=e.unpack(z["trlwe"], slots=z["slots"]))
e.close()
"""


@pytest.mark.parametrize("name,kernel", [
    ("SECURITY_128_BIT", "mfma"), ("SECURITY_128_BIT", "b4"), ("SECURITY_128_BIT", "generic"), ("SECURITY_128_BIT", "split"),
    ("SECURITY_UINT4", "sliced"), ("SECURITY_UINT4", "generic"), ("SECURITY_UINT4", "split"),
])
def test_gpu_unpack_under_every_key_switch_kernel(O, tmp_path, name, kernel):
    """TFHE_HIP_KS_KERNEL is read when a context is created: a fresh child process per value."""
    sk, ock, trlwe, want = _case(O, name)
    slots = _selection(BASE_GROUPS, 300, 5)
    path = str(tmp_path / "case.npz")
    np.savez(path, trlwe=trlwe, slots=slots, key_seed=KEY_SEED)
    env = dict(os.environ, TFHE_HIP_KS_KERNEL=kernel)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name, kernel, path], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.load(path + ".out.npz")
    assert np.array_equal(out["plain"], want[:1025])
    assert np.array_equal(out["small"], want[:7])
    assert np.array_equal(out["sel"], want[slots])


def test_host_dev_and_pool_forms_give_the_same_words(O):
    import torch

    import rs_tfhe_amd as R

    name = "SECURITY_80_BIT"
    sk, ock, trlwe, want = _case(O, name)
    p = sk.params
    count = 2 * N + 77
    slots = _selection(BASE_GROUPS, 1500, 6)
    e = _engine(name)
    try:
        t_in = torch.from_numpy(trlwe.view(np.int32)).to("cuda:0")
        t_sl = torch.from_numpy(slots.view(np.int32)).to("cuda:0")
        out = torch.full((count, p.n + 1), -1, dtype=torch.int32, device="cuda:0")
        side = torch.cuda.Stream(device=0)
        side.wait_stream(torch.cuda.current_stream(0))
        e.unpack_dev(t_in, out, count, stream=side)
        side.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want[:count])
        out_s = torch.full((len(slots), p.n + 1), -1, dtype=torch.int32, device="cuda:0")
        e.unpack_dev(t_in, out_s, len(slots), slots=t_sl)
        torch.cuda.synchronize()
        assert np.array_equal(out_s.cpu().numpy().view(np.uint32), want[slots])
        with pytest.raises(ValueError):
            e.unpack_dev(t_in, out[:5], 6)
        with pytest.raises(ValueError):
            e.unpack_dev(t_in, out_s, len(slots), slots=t_sl[:-1])
    finally:
        e.close()
    pool = R.Pool(p, [0, 0])
    try:
        pool.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=KEY_SEED)
        assert np.array_equal(pool.unpack(trlwe, count), want[:count])
        assert np.array_equal(pool.unpack(trlwe, 5), want[:5])
        assert np.array_equal(pool.unpack(trlwe, slots=slots), want[slots])
        out = torch.full((count, p.n + 1), -1, dtype=torch.int32, device="cuda:0")
        pool.unpack_dev(t_in, out, count)
        pool.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want[:count])
        out_s = torch.full((len(slots), p.n + 1), -1, dtype=torch.int32, device="cuda:0")
        pool.unpack_dev(t_in, out_s, len(slots), slots=t_sl)
        pool.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(out_s.cpu().numpy().view(np.uint32), want[slots])
    finally:
        pool.close()


def test_gate_pack_unpack_gate_on_the_device():
    """batch_gate -> pack_dev -> unpack_dev -> batch_gate over 4,096 booleans, all device-resident: the plaintext truth,
    no error allowed."""
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.engine import NAND, XOR
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    sk = SecretKey.new(p, 41)
    pk = sk.packing_key(rng_key=42)
    rng = np.random.default_rng(43)
    va, vb = rng.integers(0, 2, 4096).astype(bool), rng.integers(0, 2, 4096).astype(bool)
    e = R.Engine(p, 0)
    try:
        e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=44)
        e.load_packing_key(pk)
        ta = torch.from_numpy(sk.encrypt_bool(va, seed=45).view(np.int32)).to("cuda:0")
        tb = torch.from_numpy(sk.encrypt_bool(vb, seed=46).view(np.int32)).to("cuda:0")
        t1, t2, t3 = torch.empty_like(ta), torch.empty_like(ta), torch.empty_like(ta)
        packed = torch.empty((4, 2, N), dtype=torch.int32, device="cuda:0")
        e.batch_gate_dev(NAND, ta, tb, t1)
        e.pack_dev(t1, packed)
        e.unpack_dev(packed, t2, 4096)
        e.batch_gate_dev(XOR, t2, ta, t3)
        torch.cuda.synchronize()
        nand = ~(va & vb)
        assert np.array_equal(sk.decrypt_packed_bool(packed.cpu().numpy().view(np.uint32), 4096), nand)
        assert np.array_equal(sk.decrypt_bool(t2.cpu().numpy().view(np.uint32)), nand)
        assert np.array_equal(sk.decrypt_bool(t3.cpu().numpy().view(np.uint32)), nand ^ va)
    finally:
        e.close()


def test_client_packed_inputs_feed_a_gate():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    sk = SecretKey.new(p, 51)
    ck = sk.cloud_key(seed=52)
    rng = np.random.default_rng(53)
    va, vb = rng.integers(0, 2, 1500).astype(bool), rng.integers(0, 2, 1500).astype(bool)
    a = PK.unpack(sk.encrypt_packed_bool(va, seed=54), ck, len(va))
    b = PK.unpack(sk.encrypt_packed_bool(vb, seed=55), ck, len(vb))
    assert a.shape == (1500, p.n + 1)
    assert np.array_equal(sk.decrypt_bool(a), va)
    assert np.array_equal(sk.decrypt_bool(R.gates.batch_nand(a, b, ck)), ~(va & vb))
    assert np.array_equal(a, PK.unpack_model(p, ck.key_switching_key, sk.encrypt_packed_bool(va, seed=54), len(va)))


def test_the_diagonal_word_is_not_negated():
    """Word i = j of the row of slot j is a[0], the one word on the boundary between the plain and the negated part of
    the extraction: it is negated strictly past the diagonal (i > j).  The word-for-word unpack inputs of random words (_case
    above, ks_shapes.build_trlwe) plant 0 at a[0], and Torus::MAX - 0 = 0xFFFFFFFF rounds to the digits of 0: a kernel
    that negated at i >= j gives the same words there (mutant unpack_diag of tests/mutants.py passes them; the tests on
    real ciphertexts, test_gate_pack_unpack_gate_on_the_device and test_client_packed_inputs_feed_a_gate, notice it, in
    their decryptions).  This is the narrow case: a[0] is 0x40000000 and a random word, whose negations have other
    digits -- the test first checks that the model of the wrong kernel differs in every row -- on a toy key (n = 3,
    basebit 10, t = 3), every slot against packing.unpack_model."""
    import ks_shapes as S
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK

    case = S.case((3, 10, 3))
    p = case.params
    trlwe = np.random.default_rng(71).integers(0, 1 << 32, (2, 2, N), dtype=np.uint32)
    trlwe[:, 0, 0] = (0x40000000, 0x9E3779B9)
    slots = np.array([0, 1, 5, N - 1, N, N + 64, 2 * N - 1], np.int64)
    rows = PK.extract_rows(trlwe, slots)
    want = PK.key_switch_model(p, case.ksk, rows)
    assert np.array_equal(want, PK.unpack_model(p, case.ksk, trlwe, slots=slots))
    wrong = rows.copy()
    wrong[np.arange(len(slots)), slots % N] = ~rows[np.arange(len(slots)), slots % N]  # the diagonal negated as well
    assert (PK.key_switch_model(p, case.ksk, wrong) != want).any(axis=1).all()
    e = R.Engine(p, 0)
    try:
        e.load_cloud_key(case.cloud_key())
        assert np.array_equal(e.unpack(trlwe, slots=slots), want)
        assert np.array_equal(e.unpack(trlwe), PK.unpack_model(p, case.ksk, trlwe))  # every slot of both groups
    finally:
        e.close()


def test_unpack_error_codes():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import SECURITY_80_BIT as p

    lib = _capi.lib()
    sk = SecretKey.new(p, 61)
    trlwe = np.random.default_rng(62).integers(0, 1 << 32, (2, 2, N), dtype=np.uint32)
    tp = trlwe.ctypes.data_as(_capi.C.c_void_p)
    out = np.empty((2 * N + 1, p.n + 1), np.uint32)
    op = out.ctypes.data_as(_capi.C.c_void_p)
    e = R.Engine(p, 0)
    try:
        with pytest.raises(_capi.TfheHipError) as ei:  # no key yet
            e.unpack(trlwe, 5)
        assert ei.value.code == _capi.ENOKEY
        assert lib.tfhe_hip_batch_unpack_trlwe(e._ctx, None, 0, None, 0, None) == _capi.ENOKEY
        assert lib.tfhe_hip_batch_unpack_trlwe_dev(e._ctx, None, 0, None, 0, None, None) == _capi.ENOKEY
        view = e.new_key_view()  # a re-encryption key is no cloud key
        view.load_reenc_key(np.random.default_rng(63).integers(0, 1 << 32, (p.n, p.iks_t, p.base, p.n + 1), dtype=np.uint32))
        with pytest.raises(_capi.TfheHipError) as ei:
            view.unpack(trlwe, 5)
        assert ei.value.code == _capi.ENOKEY
        e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=64)
        for bad in ([2 * N], [0, 5, 2 * N, 1], [0xFFFFFFFF]):
            with pytest.raises(_capi.TfheHipError) as ei:
                e.unpack(trlwe, slots=np.array(bad, np.uint32))
            assert ei.value.code == _capi.EINVAL, bad
        with pytest.raises(_capi.TfheHipError) as ei:
            e.unpack(trlwe, 2 * N + 1)
        assert ei.value.code == _capi.EINVAL
        assert lib.tfhe_hip_batch_unpack_trlwe_dev(e._ctx, tp, 2, None, 2 * N + 1, op, None) == _capi.EINVAL
        assert lib.tfhe_hip_batch_unpack_trlwe(e._ctx, None, 2, None, 5, op) == _capi.EINVAL
        assert lib.tfhe_hip_batch_unpack_trlwe(e._ctx, tp, 2, None, 5, None) == _capi.EINVAL
        assert lib.tfhe_hip_batch_unpack_trlwe(e._ctx, None, 0, None, 0, None) == _capi.OK
        assert lib.tfhe_hip_batch_unpack_trlwe_dev(e._ctx, None, 0, None, 0, None, None) == _capi.OK
        assert e.unpack(trlwe, 2 * N).shape == (2 * N, p.n + 1)  # the handle still works after the refusals
    finally:
        e.close()
    pool = R.Pool(p, [0, 0])
    try:
        with pytest.raises(_capi.TfheHipError) as ei:
            pool.unpack(trlwe, 5)
        assert ei.value.code == _capi.ENOKEY
        pool.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=64)
        with pytest.raises(_capi.TfheHipError) as ei:
            pool.unpack(trlwe, slots=np.array([1, 2 * N], np.uint32))
        assert ei.value.code == _capi.EINVAL
        with pytest.raises(_capi.TfheHipError) as ei:
            pool.unpack(trlwe, 2 * N + 1)
        assert ei.value.code == _capi.EINVAL
        assert pool.unpack(trlwe, 0).shape == (0, p.n + 1)
    finally:
        pool.close()


def test_cpp_mirror_unpack(O):
    """tests/cpp/test_unpack.cpp: Engine::unpack against the oracle library."""
    import tempfile

    from test_unpack_host import build_cpp_unpack

    with tempfile.TemporaryDirectory() as d:
        exe = build_cpp_unpack(d)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test_unpack ok" in r.stdout
