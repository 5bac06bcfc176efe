"""Unpacking key switch on the host, no GPU: the integer model (packing.unpack_model) against the oracle's
sample_extract_index followed by identity_key_switching, word for word on four parameter sets; the client's packed
encryption read back by decrypt_packed_*; gate and LUT outputs through pack_model and unpack_model decrypting without
an error; the exported entry points, their prototypes, the EINVAL cases of the C ABI that need no device, and the C++
mirror program's build."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from rs_tfhe_amd import _capi, packing as PK
from rs_tfhe_amd.client import SecretKey
from rs_tfhe_amd.params import N, PARAM_SETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ["SECURITY_128_BIT", "SECURITY_80_BIT", "SECURITY_UINT4", "SECURITY_UINT8"]
COUNTS = (1, 7, 1024, 1025)
# duplicates, reversed order, both edges of both groups, the last slot of the last group
SLOTS = (2047, 2047, 1025, 1024, 1023, 517, 1, 0, 0, 2047)
ENTRY_POINTS = ("batch_unpack_trlwe", "batch_unpack_trlwe_dev", "pool_batch_unpack_trlwe", "pool_batch_unpack_trlwe_dev")


def oracle_unpack(O, ock, trlwe, slots):
    """The reference composition: sample_extract_index(trlwe_G, j), then identity_key_switching, per slot."""
    trlwe = np.asarray(trlwe, np.uint32).reshape(-1, 2, N)
    rows = np.stack([O.sample_extract_index(trlwe[s // N], s % N) for s in slots])
    return O.batch_identity_key_switching(ock, rows)


@pytest.mark.parametrize("name", SETS)
def test_unpack_model_equals_the_oracle_composition(O, name):
    """Random TRLWE words under a key-switching key of random words (the identity is word for word under any key)."""
    p, op = PARAM_SETS[name], getattr(O, name)
    rng = np.random.default_rng(31)
    ksk = rng.integers(0, 1 << 32, (N, p.iks_t, p.base, p.n + 1), dtype=np.uint32)
    ock = O.CloudKey.from_arrays(op, np.zeros((p.n, 2 * p.l, 2, N)), ksk, 0, np.zeros((2, N), np.uint32))
    trlwe = rng.integers(0, 1 << 32, (2, 2, N), dtype=np.uint32)
    # the negation's and the rounding's edges; the last is where Torus::MAX - a and 0 - a round to different digits
    half = 1 << (31 - p.basebit * p.iks_t)
    trlwe[0, 0, :6] = (0, 1 << 31, 0xFFFFFFFF, half - 1, half, 3 * half)
    want = oracle_unpack(O, ock, trlwe, range(max(COUNTS)))  # output m depends on slot m alone: every count is a prefix
    for count in COUNTS:
        got = PK.unpack_model(p, ksk, trlwe, count)
        assert got.shape == (count, p.n + 1) and got.dtype == np.uint32
        assert np.array_equal(got, want[:count]), count
    got = PK.unpack_model(p, ksk, trlwe, slots=SLOTS)
    assert np.array_equal(got, oracle_unpack(O, ock, trlwe, SLOTS))
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[-1], got[0])
    assert PK.unpack_model(p, ksk, trlwe[:0]).shape == (0, p.n + 1)  # count=None: every slot
    with pytest.raises(ValueError):
        PK.unpack_model(p, ksk, trlwe, 2 * N + 1)
    with pytest.raises(ValueError):
        PK.unpack_model(p, ksk, trlwe, slots=[2 * N])
    with pytest.raises(ValueError):
        PK.unpack_model(p, ksk, trlwe, 3, slots=[0, 1])


def test_extract_rows_is_sample_extract_index(O):
    trlwe = np.random.default_rng(32).integers(0, 1 << 32, (3, 2, N), dtype=np.uint32)
    slots = [0, 1, 1023, 1024, 2000, 3071]
    rows = PK.extract_rows(trlwe, slots)
    for r, s in zip(rows, slots):
        assert np.array_equal(r, O.sample_extract_index(trlwe[s // N], s % N)), s


def test_unpack_model_does_not_need_the_oracle():
    import ast

    with open(PK.__file__) as f:
        tree = ast.parse(f.read())
    names = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    names += [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert not [m for m in names if m.split(".")[0] == "oracle"]


def test_client_packed_encryption_reads_back():
    p = PARAM_SETS["SECURITY_128_BIT"]
    sk = SecretKey.new(p, 3)
    bits = np.random.default_rng(2).integers(0, 2, 2500).astype(bool)
    packed = sk.encrypt_packed_bool(bits, seed=4)
    assert packed.shape == (3, 2, N) and packed.dtype == np.uint32
    assert np.array_equal(sk.decrypt_packed_bool(packed, len(bits)), bits)
    # the unused slots of the last group encrypt 0; every slot carries noise at alpha_lv1
    rest = sk.packed_phase(packed, 3 * N)[len(bits):].view(np.int32).astype(np.float64) / 2.0 ** 32
    assert 0 < np.abs(rest).max() < 8 * p.alpha_lv1
    err = sk.packed_phase(packed, len(bits)) - np.where(bits, 1 << 29, 7 << 29).astype(np.uint32)
    assert 0.8 * p.alpha_lv1 < (err.view(np.int32) / 2.0 ** 32).std() < 1.2 * p.alpha_lv1
    # the same seed gives the same words; the masks are not all alike; alpha = 0 is the plain phase
    assert np.array_equal(sk.encrypt_packed_bool(bits, seed=4), packed)
    assert not np.array_equal(packed[0, 0], packed[1, 0])
    exact = sk.encrypt_packed_f64([0.25, -0.125], seed=5, alpha=0.0)
    assert exact.shape == (1, 2, N)
    assert np.array_equal(sk.packed_phase(exact, 3), np.array([1 << 30, 7 << 29, 0], np.uint32))
    p = PARAM_SETS["SECURITY_UINT4"]
    sk = SecretKey.new(p, 5)
    for m in (8, 16):
        msgs = np.arange(1500) % m
        packed = sk.encrypt_packed_lwe_message(msgs, m, seed=m)
        assert packed.shape == (2, 2, N)
        assert np.array_equal(sk.decrypt_packed_lwe_message(packed, len(msgs), m), msgs)


@pytest.mark.parametrize("name", ["SECURITY_128_BIT", "SECURITY_80_BIT"])
def test_gate_outputs_survive_pack_and_unpack(O, name):
    """1,024 NAND outputs -> pack_model -> unpack_model: every one decrypts, and so does a gate over them.  The CPU
    check behind the feature found the worst phase error at 0.32 of the half-interval 1/8 on these sets."""
    from conftest import oracle_keys

    op = getattr(O, name)
    osk, ock = oracle_keys(O, op)
    p = PARAM_SETS[name]
    sk = SecretKey(p, osk.key_lv0, osk.key_lv1)
    rng = np.random.default_rng(5)
    va, vb = rng.integers(0, 2, N).astype(bool), rng.integers(0, 2, N).astype(bool)
    out = O.batch_gate(ock, O.GATE_NAND, sk.encrypt_bool(va, seed=6), sk.encrypt_bool(vb, seed=7))
    pk = sk.packing_key(rng_key=8)
    packed = PK.pack_model(p, pk.mask_seed, pk.bodies, out)
    back = PK.unpack_model(p, ock.key_switching_key, packed, N)
    assert np.array_equal(sk.decrypt_bool(back), ~(va & vb))
    assert np.array_equal(back, oracle_unpack(O, ock, packed, range(N))[:N])
    sel = np.arange(0, N, 16)
    xor = O.batch_gate(ock, O.GATE_XOR, back[sel], back[sel[::-1]])
    assert np.array_equal(sk.decrypt_bool(xor), (~(va & vb))[sel] ^ (~(va & vb))[sel[::-1]])


@pytest.mark.parametrize("name,m,source", [("SECURITY_UINT4", 8, "pbs"), ("SECURITY_UINT8", 16, "pbs"),
                                           ("SECURITY_UINT8", 256, "fresh")])
def test_lut_outputs_survive_pack_and_unpack(O, name, m, source):
    """Packing's safe moduli: 1,024 results -> pack_model -> unpack_model decode without an error
    (profiles/unpack_noise.json has the margins over 30,720 inputs).  The results are programmable-bootstrap outputs
    where one bootstrap can evaluate a table of that modulus; at m = 256 (four test-vector slots a message on N = 1024:
    the bootstrap's own input rounding already decodes wrong) they are fresh encryptions at alpha_lv0, the noise level
    of a bootstrapped result, as in packing's noise table."""
    from conftest import oracle_keys

    op = getattr(O, name)
    osk, ock = oracle_keys(O, op)
    p = PARAM_SETS[name]
    sk = SecretKey(p, osk.key_lv0, osk.key_lv1)
    msgs = np.random.default_rng(m).integers(0, m, N)
    if source == "pbs":
        f = lambda x: (3 * x + 1) % m  # noqa: E731
        out = O.batch_bootstrap(ock, sk.encrypt_lwe_message(msgs, m, seed=9), testvec=O.lut_generate(f, m))
        msgs = f(msgs)
    else:
        out = sk.encrypt_lwe_message(msgs, m, seed=9)
    assert np.array_equal(sk.decrypt_lwe_message(out, m), msgs)
    pk = sk.packing_key(rng_key=10)
    packed = PK.pack_model(p, pk.mask_seed, pk.bodies, out)
    back = PK.unpack_model(p, ock.key_switching_key, packed, N)
    assert np.array_equal(sk.decrypt_lwe_message(back, m), msgs)


def test_unpack_entry_points_exported_with_their_prototypes():
    lib = _capi.lib()
    sz, vp, ci = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    want = {
        "batch_unpack_trlwe": [vp, vp, sz, vp, sz, vp],
        "batch_unpack_trlwe_dev": [vp, vp, sz, vp, sz, vp, vp],
        "pool_batch_unpack_trlwe": [vp, vp, sz, vp, sz, vp],
        "pool_batch_unpack_trlwe_dev": [vp, ci, vp, sz, vp, sz, vp, vp],
    }
    assert set(want) == set(ENTRY_POINTS)
    for fn, args in want.items():
        f = getattr(lib, "tfhe_hip_" + fn)  # AttributeError: not exported
        assert f.restype is ci and list(f.argtypes) == args, fn
    with open(os.path.join(ROOT, "include", "tfhe_hip.h")) as fh:
        header = fh.read()
    for fn in ENTRY_POINTS:
        assert "int tfhe_hip_" + fn + "(" in header, fn


def test_unpack_einval_without_a_device():
    lib = _capi.lib()
    for fn in ENTRY_POINTS:
        f = getattr(lib, "tfhe_hip_" + fn)
        args = [0 if t in (ctypes.c_size_t, ctypes.c_int) else None for t in f.argtypes]
        assert f(*args) == _capi.EINVAL, fn
        args = [5 if t is ctypes.c_size_t else 0 if t is ctypes.c_int else None for t in f.argtypes]
        assert f(*args) == _capi.EINVAL, fn


def build_cpp_unpack(outdir):
    """tests/cpp/test_unpack.cpp, built as test_many_lut_host.build_cpp_many_lut builds the many-LUT program."""
    exe = os.path.join(outdir, "test_unpack")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_unpack.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-L" + os.path.join(ROOT, "oracle"), "-ltfhe_oracle",
        "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-fopenmp", "-pthread"])
    return exe


def test_cpp_unpack_program_builds(O, tmp_path):
    """The C++ mirror's Engine::unpack program compiles and links against the header and both libraries (run on the GPU
    by tests/test_gpu_unpack.py)."""
    assert os.path.exists(build_cpp_unpack(str(tmp_path)))
