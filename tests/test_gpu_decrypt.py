"""Decryption on the GPU (include/tfhe_hip.h, "decryption"; csrc/decrypt.hpp) against rs-tfhe_amd/client.py's numpy path:
every comparison is np.array_equal, there are no tolerances.

The shapes are the smallest at which the kernels can go wrong.  LWE rows: n = 33 and 48 (the lane tail of a wave's
pass), 64 (exactly one pass) and 65 (one word into the second pass), SECURITY_128_BIT (701-word rows: every 4-byte
alignment phase occurs within 4 rows), SECURITY_UINT7 (n = 1,160 > 1,024) and lv1 rows of 1,025 words under key_lv1;
counts 1, 5, 257 and 4,099 (fewer rows than waves, a partly filled last workgroup) -- at these a wave of the grid,
which is sized from the CU count (8 workgroups of 4 waves a CU), has at most one row, so the grid-stride loop and its
tail are taken by test_lwe_grid_stride_loop at a row count derived from the device's CU count.  Packed: 1, 3 and 64
groups cut at 1, N - 1, N, N + 1 and groups N results.  The planted phases of the decode are those of tests/test_decrypt_host.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import keygen_model as KM
import sym_encrypt_model as SM
from test_decrypt_host import BOOL, MESSAGE, MODULI, PHASE, boundary_phases, build_cpp_decrypt, numpy_message
from rs_tfhe_amd.client import SecretKey
from rs_tfhe_amd.params import N, PARAM_SETS

pytestmark = pytest.mark.gpu

TOY = (SM.SHAPES[0], SM.SHAPES[2], (64, 2, 10, 2, 8), (65, 2, 10, 2, 8))  # n = 33, 48, 64, 65
COUNTS = (1, 5, 257, 4099)
_ENGINES = {}


def _engine(p):
    """one engine a parameter set for the module (no key is needed)"""
    import rs_tfhe_amd as R

    if p not in _ENGINES:
        _ENGINES[p] = R.Engine(p, 0)
    return _ENGINES[p]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _words(shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def _rows(count, width, seed, plant=True):
    """random rows; with room for them, one row of all 0xFFFFFFFF and one of all 0x80000000"""
    cts = _words((count, width), seed)
    if plant and count >= 5:
        cts[1] = 0xFFFFFFFF
        cts[count - 2] = 0x80000000
    return cts


def _keys(n, seed):
    last = np.zeros(n, np.uint32)
    last[-1] = 1
    return {"random": np.random.default_rng(seed).integers(0, 2, n).astype(np.uint32), "ones": np.ones(n, np.uint32),
            "zeros": np.zeros(n, np.uint32), "last": last}


def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _lwe_case(p, count, lv1=False):
    """phases of the four keys through the host form, and of the random key through the _dev form"""
    import torch

    e = _engine(p)
    n = N if lv1 else p.n
    cts = _rows(count, n + 1, 1000 * n + count)
    for name, key in _keys(n, n).items():
        sk = SecretKey(p, np.zeros(p.n, np.uint32), key) if lv1 else SecretKey(p, key, np.zeros(N, np.uint32))
        want = sk.phase_lv1(cts) if lv1 else sk.phase(cts)
        got = e.batch_decrypt(key, cts)
        assert got.dtype == np.uint32 and got.shape == (count,)
        assert np.array_equal(got, want), (name, n, count, int((got != want).sum()))
        if name == "random":
            out = torch.full((count,), -1, dtype=torch.int32, device="cuda:0")
            e.batch_decrypt_dev(key, _t(cts), out)
            torch.cuda.synchronize()
            assert np.array_equal(_host(out), want), ("_dev", n, count)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("shape", TOY, ids=lambda s: f"n{s[0]}")
def test_lwe_phases_toy_sets(shape, count):
    _lwe_case(KM.shape_params(shape), count)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name,lv1", [("SECURITY_128_BIT", False), ("SECURITY_UINT7", False), ("SECURITY_128_BIT", True)],
                         ids=["n700", "n1160", "lv1_rows"])
def test_lwe_phases_real_sets(name, lv1, count):
    _lwe_case(PARAM_SETS[name], count, lv1)


@pytest.mark.parametrize("shape", [TOY[0], (700, 3, 6, 2, 9)], ids=lambda s: f"n{s[0]}")
def test_lwe_grid_stride_loop(shape):
    """More rows than the grid has waves: k_lwe_phase runs on at most 8 workgroups of 4 waves a CU (csrc/decrypt.hpp,
    kDecBlocksPerCu x kDecWaves), so at 2 x 32 x CUs + 3 rows every wave walks two rows and three waves a third -- the
    stride, the key register's survival from row to row and the loop's tail.  Host and _dev form, the planted rows, the
    four keys."""
    import torch

    waves = 8 * 4 * torch.cuda.get_device_properties(0).multi_processor_count
    count = 2 * waves + 3
    p = KM.shape_params(shape)
    e = _engine(p)
    cts = _rows(count, p.n + 1, 31 + p.n)
    cts[waves + 1] = 0xFFFFFFFF  # (a planted row in the second pass too)
    tc = _t(cts)
    for name, key in _keys(p.n, 7 + p.n).items():
        want = SecretKey(p, key, np.zeros(N, np.uint32)).phase(cts)
        got = e.batch_decrypt(key, cts)
        assert np.array_equal(got, want), (name, p.n, count, np.flatnonzero(got != want)[:8])
        out = torch.full((count,), -1, dtype=torch.int32, device="cuda:0")
        e.batch_decrypt_dev(key, tc, out)
        torch.cuda.synchronize()
        assert np.array_equal(_host(out), want), ("_dev", name, p.n, count)
    # the phases differ from row to row (here: of the last key), so a wave that repeated or skipped a row showed above
    assert len(np.unique(want)) > count - 16


@pytest.mark.parametrize("shape", TOY + ((700, 3, 6, 2, 9),), ids=lambda s: f"n{s[0]}")
def test_a_wrong_body_would_show_in_every_row(shape):
    """The input itself tells the body's position apart: with row r - 1's or row r + 1's body, or with word n - 1, taken
    for the body, the phase of EVERY row would differ from the right one -- asserted on the input, then the kernel is
    held to the right one."""
    p = KM.shape_params(shape)
    n, count = p.n, 257
    cts = _rows(count, n + 1, 77 + n, plant=False)
    key = _keys(n, n)["random"]
    body = cts[:, n]
    assert (body[1:] != body[:-1]).all(), "a neighbour's body equals the row's own"
    assert (cts[:, n - 1] != body).all(), "word n - 1 equals the body"
    # (the sum over the mask is the same in all three mistakes, so the phases differ exactly where the bodies do)
    want = SecretKey(p, key, np.zeros(N, np.uint32)).phase(cts)
    assert np.array_equal(_engine(p).batch_decrypt(key, cts), want)


def test_modes_on_ciphertexts():
    """BOOL and MESSAGE on ciphertexts of encrypt_bool / encrypt_lwe_message: the numpy path's words, and the messages"""
    p = PARAM_SETS["SECURITY_128_BIT"]
    sk = SecretKey.new(p, 41)
    _engine(p)  # (engine_for's own engine serves device=0; this one only keeps the module's habit)
    bits = np.random.default_rng(42).integers(0, 2, 257).astype(bool)
    cts = sk.encrypt_bool(bits, seed=43)
    got = sk.decrypt_bool(cts, device=0)
    assert got.dtype == np.bool_ and np.array_equal(got, sk.decrypt_bool(cts)) and np.array_equal(got, bits)
    ph = sk.phase(cts, device=0)
    assert ph.dtype == np.uint32 and np.array_equal(ph, sk.phase(cts))
    for m in (2, 3, 16, 10):
        msgs = np.random.default_rng(44 + m).integers(0, m, 257)
        c = sk.encrypt_lwe_message(msgs, m, seed=45 + m)
        got = sk.decrypt_lwe_message(c, m, device=0)
        assert got.dtype == np.int64 and np.array_equal(got, sk.decrypt_lwe_message(c, m)) and np.array_equal(got, msgs), m


@pytest.mark.parametrize("m", MODULI)
def test_modes_on_planted_phases(m):
    """a = 0, b = phase forces any phase: the decode at every planted boundary, through both kernels"""
    p = KM.shape_params(TOY[0])
    e = _engine(p)
    ph = boundary_phases(m)
    cts = np.zeros((len(ph), p.n + 1), np.uint32)
    cts[:, -1] = ph
    key = _keys(p.n, 3)["random"]
    assert np.array_equal(e.batch_decrypt(key, cts, PHASE), ph)
    assert np.array_equal(e.batch_decrypt(key, cts, "bool"), (ph.view(np.int32) >= 0).astype(np.uint32))
    got = e.batch_decrypt(key, cts, "message", m)
    assert np.array_equal(got.astype(np.int64), numpy_message(ph, m)), m
    # the packed kernel: A = 0, B = the phases
    groups = -(-len(ph) // N)
    slots = np.zeros(groups * N, np.uint32)
    slots[:len(ph)] = ph
    packed = np.zeros((groups, 2, N), np.uint32)
    packed[:, 1, :] = slots.reshape(groups, N)
    key1 = _keys(N, 4)["random"]
    assert np.array_equal(e.batch_decrypt_trlwe(key1, packed, len(ph), MESSAGE, m).astype(np.int64), numpy_message(ph, m))
    assert np.array_equal(e.batch_decrypt_trlwe(key1, packed, len(ph), BOOL), (ph.view(np.int32) >= 0).astype(np.uint32))


@pytest.mark.parametrize("groups", [1, 3, 64])
def test_packed_phases(groups):
    p = PARAM_SETS["SECURITY_128_BIT"]
    e = _engine(p)
    packed = _words((groups, 2, N), 500 + groups)
    packed[0, 0, :7] = 0xFFFFFFFF
    packed[-1, 0, -7:] = 0x80000000
    counts = sorted({c for c in (1, N - 1, N, N + 1, groups * N) if c <= groups * N})
    keys = _keys(N, 9)
    for name in ("ones", "zeros", "random"):
        sk = SecretKey(p, np.zeros(p.n, np.uint32), keys[name])
        want = sk.packed_phase(packed, groups * N)  # once a key; the cuts are its prefixes
        for count in counts:
            got = e.batch_decrypt_trlwe(keys[name], packed, count)
            assert got.shape == (count,) and np.array_equal(got, want[:count]), (name, groups, count)
            assert np.array_equal(sk.packed_phase(packed, count, device=0), want[:count])


def test_packed_round_trips():
    p = PARAM_SETS["SECURITY_128_BIT"]
    sk = SecretKey.new(p, 51)
    count = N + 5
    bits = np.random.default_rng(52).integers(0, 2, count).astype(bool)
    packed = sk.encrypt_packed_bool(bits, seed=53)
    got = sk.decrypt_packed_bool(packed, count, device=0)
    assert got.dtype == np.bool_ and np.array_equal(got, bits) and np.array_equal(got, sk.decrypt_packed_bool(packed, count))
    msgs = np.random.default_rng(54).integers(0, 10, count)
    pm = sk.encrypt_packed_lwe_message(msgs, 10, seed=55)
    got = sk.decrypt_packed_lwe_message(pm, count, 10, device=0)
    assert got.dtype == np.int64 and np.array_equal(got, msgs) and np.array_equal(got, sk.decrypt_packed_lwe_message(pm, count, 10))


def test_dev_forms_on_a_side_stream():
    """torch tensor in, torch tensor out, queued on a stream of the caller's; equal to the host form in every mode"""
    import torch

    p = PARAM_SETS["SECURITY_128_BIT"]
    e = _engine(p)
    sk = SecretKey.new(p, 61)
    cts, rows, packed = _rows(257, p.n + 1, 62), _rows(33, N + 1, 63), _words((3, 2, N), 64)
    tc, tr, tp = _t(cts), _t(rows), _t(packed)
    side = torch.cuda.Stream(device=0)
    for mode, m in (("phase", None), ("bool", None), ("message", 10)):
        jobs = [(lambda o: e.batch_decrypt_dev(sk.key_lv0, tc, o, mode, m, stream=side), 257, e.batch_decrypt(sk.key_lv0, cts, mode, m)),
                (lambda o: e.batch_decrypt_dev(sk.key_lv1, tr, o, mode, m, stream=side), 33, e.batch_decrypt(sk.key_lv1, rows, mode, m)),
                (lambda o: e.batch_decrypt_trlwe_dev(sk.key_lv1, tp, 2 * N + 9, o, mode, m, stream=side), 2 * N + 9,
                 e.batch_decrypt_trlwe(sk.key_lv1, packed, 2 * N + 9, mode, m))]
        for job, count, host in jobs:
            out = torch.full((count,), -1, dtype=torch.int32, device="cuda:0")
            side.wait_stream(torch.cuda.current_stream(0))
            job(out)
            side.synchronize()
            assert np.array_equal(_host(out), host), mode
    # SecretKey with a tensor: a tensor on that device comes back, in the dtypes of the numpy path
    torch.cuda.synchronize()
    got = sk.phase(tc, device=0)
    assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(_host(got), sk.phase(cts))
    got = sk.decrypt_bool(tc, device=0)
    assert got.is_cuda and got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), sk.decrypt_bool(cts))
    got = sk.decrypt_lwe_message(tc, 10, device=0)
    assert got.is_cuda and got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), sk.decrypt_lwe_message(cts, 10))
    assert np.array_equal(_host(sk.phase_lv1(tr, device=0)), sk.phase_lv1(rows))
    assert np.array_equal(_host(sk.packed_phase(tp, 2 * N + 9, device=0)), sk.packed_phase(packed, 2 * N + 9))
    assert np.array_equal(sk.decrypt_packed_bool(tp, N + 1, device=0).cpu().numpy(), sk.decrypt_packed_bool(packed, N + 1))
    assert np.array_equal(sk.decrypt_packed_lwe_message(tp, N + 1, 16, device=0).cpu().numpy(),
                          sk.decrypt_packed_lwe_message(packed, N + 1, 16))


def test_end_to_end_gates():
    """encrypt_bool(device=0) -> batch_nand -> decrypt_bool(device=0); and the same gate stage by stage up to its lv1
    rows (NAND's linear prep, blind rotation, sample extraction: [count][N+1] under key_lv1) read with
    phase_lv1(device=0): their signs agree with the key-switched output's.  (The _nks gate calls themselves return
    sample_extract_index_2 rows of n + 1 words, which no key decrypts: DESIGN section 1, Q5.)"""
    import rs_tfhe_amd as R
    from rs_tfhe_amd.bootstrap import keyed_engine

    p = PARAM_SETS["SECURITY_128_BIT"]
    sk = SecretKey.new(p, 71)
    ck = sk.cloud_key(seed=72, device=0)
    rng = np.random.default_rng(73)
    A, B = rng.integers(0, 2, 257).astype(bool), rng.integers(0, 2, 257).astype(bool)
    ca, cb = sk.encrypt_bool(A, device=0, first_index=0), sk.encrypt_bool(B, device=0, first_index=257)
    out = R.gates.batch_nand(ca, cb, ck)
    got = sk.decrypt_bool(out, device=0)
    assert np.array_equal(got, ~(A & B)) and np.array_equal(got, sk.decrypt_bool(out))
    with keyed_engine(ck, 0) as eng:
        prep = eng.batch_tlwe_lincomb(-1, ca, -1, cb, 0x20000000)  # 1/8 - a - b (gates.rs: nand)
        lv1 = eng.batch_sample_extract(eng.batch_blind_rotate(prep), 0)
        ks = eng.batch_identity_key_switch(lv1)
    assert lv1.shape == (257, N + 1)
    ph1 = sk.phase_lv1(lv1, device=0)
    assert np.array_equal(ph1, sk.phase_lv1(lv1))
    assert np.array_equal(ph1.view(np.int32) >= 0, sk.phase(ks, device=0).view(np.int32) >= 0)
    assert np.array_equal(ph1.view(np.int32) >= 0, ~(A & B))


def test_error_codes():
    from rs_tfhe_amd import _capi

    p = PARAM_SETS["SECURITY_128_BIT"]
    e = _engine(p)
    lib, n = e._lib, p.n
    key, key1 = _keys(n, 1)["random"], _keys(N, 2)["random"]
    cts, packed = _rows(5, n + 1, 3), _words((2, 2, N), 4)
    out = np.full(2 * N + 8, 0xDEADBEEF, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    lwe = lambda k, klen, i, cnt, mode, m, o: lib.tfhe_hip_batch_decrypt(e._ctx, k, klen, i, cnt, mode, m, o)  # noqa: E731
    lwe_dev = lambda k, klen, i, cnt, mode, m, o: lib.tfhe_hip_batch_decrypt_dev(e._ctx, k, klen, i, cnt, mode, m, o, None)  # noqa: E731
    pk = lambda k, t, g, cnt, mode, m, o: lib.tfhe_hip_batch_decrypt_trlwe(e._ctx, k, t, g, cnt, mode, m, o)  # noqa: E731
    pk_dev = lambda k, t, g, cnt, mode, m, o: lib.tfhe_hip_batch_decrypt_trlwe_dev(e._ctx, k, t, g, cnt, mode, m, o, None)  # noqa: E731
    for f in (lwe, lwe_dev):  # (every refusal comes before a pointer is followed on the device: host arrays serve both)
        assert f(ptr(key), n + 1, ptr(cts), 5, PHASE, 0, ptr(out)) == _capi.EINVAL  # a key_len that is neither n nor N
        assert f(ptr(key), 0, ptr(cts), 5, PHASE, 0, ptr(out)) == _capi.EINVAL
        bad = key.copy()
        bad[n // 2] = 2
        assert f(ptr(bad), n, ptr(cts), 5, PHASE, 0, ptr(out)) == _capi.EINVAL
        assert b"binary" in lib.tfhe_hip_last_error(e._ctx)
        for m in (0, 1, 65537):
            assert f(ptr(key), n, ptr(cts), 5, MESSAGE, m, ptr(out)) == _capi.EINVAL, m
        for mode in (-1, 3):
            assert f(ptr(key), n, ptr(cts), 5, mode, 0, ptr(out)) == _capi.EINVAL, mode
        assert f(None, n, ptr(cts), 5, PHASE, 0, ptr(out)) == _capi.EINVAL
        assert f(ptr(key), n, None, 5, PHASE, 0, ptr(out)) == _capi.EINVAL
        assert f(ptr(key), n, ptr(cts), 5, PHASE, 0, None) == _capi.EINVAL
        assert f(ptr(key), n, ptr(cts), 1 << 31, PHASE, 0, ptr(out)) == _capi.EINVAL
        assert f(ptr(key), n, ptr(cts), 0, PHASE, 0, ptr(out)) == _capi.OK
        assert f(ptr(key), n, ptr(cts), 0, MESSAGE, 65536, ptr(out)) == _capi.OK
    for f in (pk, pk_dev):
        assert f(ptr(key1), ptr(packed), 2, 2 * N + 1, PHASE, 0, ptr(out)) == _capi.EINVAL  # count > groups N
        assert f(ptr(key1), ptr(packed), 0, 1, PHASE, 0, ptr(out)) == _capi.EINVAL
        bad = key1.copy()
        bad[-1] = 0xFFFFFFFF
        assert f(ptr(bad), ptr(packed), 2, 5, PHASE, 0, ptr(out)) == _capi.EINVAL
        assert f(ptr(key1), ptr(packed), 2, 5, MESSAGE, 1, ptr(out)) == _capi.EINVAL
        assert f(ptr(key1), ptr(packed), 2, 5, MESSAGE, 65537, ptr(out)) == _capi.EINVAL
        assert f(ptr(key1), ptr(packed), 2, 5, 7, 0, ptr(out)) == _capi.EINVAL
        assert f(None, ptr(packed), 2, 5, PHASE, 0, ptr(out)) == _capi.EINVAL
        assert f(ptr(key1), None, 2, 5, PHASE, 0, ptr(out)) == _capi.EINVAL
        assert f(ptr(key1), ptr(packed), 2, 5, PHASE, 0, None) == _capi.EINVAL
        assert f(ptr(key1), ptr(packed), 2, 0, PHASE, 0, ptr(out)) == _capi.OK
        assert f(ptr(key1), ptr(packed), 0, 0, PHASE, 0, ptr(out)) == _capi.OK
        assert f(ptr(key1), ptr(packed), (1 << 64) - 1, 0, PHASE, 0, ptr(out)) == _capi.OK  # count == 0: whatever groups is
        assert f(ptr(key1), ptr(packed), (1 << 63), 1 << 31, PHASE, 0, ptr(out)) == _capi.EINVAL  # count too large
    assert (out == 0xDEADBEEF).all(), "a refused or empty call wrote to its output"
    assert lib.tfhe_hip_batch_decrypt(None, ptr(key), n, ptr(cts), 5, PHASE, 0, ptr(out)) == _capi.EINVAL
    # the largest modulus is accepted, and the handle still works
    assert np.array_equal(e.batch_decrypt(key, cts, "message", 65536).astype(np.int64),
                          numpy_message(SecretKey(p, key, np.zeros(N, np.uint32)).phase(cts), 65536))
    with pytest.raises(ValueError):
        e.batch_decrypt(key, cts, "message")
    with pytest.raises(ValueError):
        e.batch_decrypt(key, cts, "signs")


def test_cpp_mirror_program(tmp_path):
    """tests/cpp/test_decrypt.cpp, run once: SecretKey::decrypt_batch / phase_batch and the packed pair of the C++ mirror"""
    exe = build_cpp_decrypt(str(tmp_path))
    r = subprocess.run([exe, "257"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), r.stdout + r.stderr
