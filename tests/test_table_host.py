"""Encrypted-table key switch and the tree bootstrap on the host, no GPU: the integer model (packing.table_model)
against the direct definition of include/tfhe_hip.h and against the window over pack_model's sparse group, the key-free
closed form for trivial inputs, the exact phase at zero noise, Generator.generate_bivariate_tables, one composition of
the whole tree bootstrap on the CPU oracle, the new exports and their EINVAL cases that need no device, and the C++
program's build."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from rs_tfhe_amd import _capi, packing as PK
from rs_tfhe_amd.client import SecretKey
from rs_tfhe_amd.lut import Generator
from rs_tfhe_amd.params import N, SECURITY_80_BIT, SECURITY_128_BIT, SECURITY_UINT4, SECURITY_UINT8
from rs_tfhe_amd.seeded import negacyclic_binary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = [SECURITY_128_BIT, SECURITY_80_BIT, SECURITY_UINT4, SECURITY_UINT8]
NEW_EXPORTS = ("batch_pack_table", "batch_pack_table_dev", "batch_bootstrap_bivariate", "batch_bootstrap_bivariate_dev",
               "pool_batch_bootstrap_bivariate")
_KEYS = {}


def _key(p, alpha=None):
    if (p.name, alpha) not in _KEYS:
        sk = SecretKey.new(p, 3)
        pk = sk.packing_key(rng_key=4, alpha=alpha)
        _KEYS[(p.name, alpha)] = (sk, pk, PK.key_rows(p, pk.mask_seed, pk.bodies))
    return _KEYS[(p.name, alpha)]


def _words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def direct_table(p, rows, stage1, m):
    """The definition input by input, sharing no code with table_model: each input key-switched alone to a TRLWE row
    (exact int64), times X^(x W), summed, then out[y] = sum_{r < W} Q~[y + off - r] term by term."""
    k = rows.astype(np.int64)
    stage1 = np.asarray(stage1, np.uint32).reshape(m, -1, p.n + 1)
    count, W = stage1.shape[1], N // m
    off = W // 2
    out = np.zeros((count, 2, N), np.uint32)
    for c in range(count):
        Q = np.zeros((2, N), np.int64)
        for x in range(m):
            ct = stage1[x, c]
            ks = -(PK.digits(p, ct[:p.n]).reshape(-1).astype(np.int64) @ k)
            ks[N] += int(ct[p.n])
            j = x * W
            for h in range(2):
                poly = ks[h * N:(h + 1) * N]
                Q[h] += np.concatenate([-poly[N - j:], poly[:N - j]]) if j else poly  # X^j poly, negacyclic
        Q &= 0xFFFFFFFF
        acc = np.zeros((2, N), np.int64)
        for r in range(W):
            i = np.arange(N) + off - r  # in (-N, 2N)
            sign = np.where((i < 0) | (i >= N), -1, 1)
            acc += sign[None, :] * Q[:, i % N]
        out[c] = (acc & 0xFFFFFFFF).astype(np.uint32)
    return out


@pytest.mark.parametrize("p", SETS, ids=lambda p: p.name)
def test_table_model_equals_the_direct_definition(p):
    sk, pk, rows = _key(p)
    rng = np.random.default_rng(31)
    for m in (2, 4, 16, 64):
        for count in (1, 3):
            s1 = _words(rng, (m, count, p.n + 1))  # uniform words, not only valid ciphertexts
            got = PK.table_model(p, pk.mask_seed, pk.bodies, s1, m, rows=rows)
            assert got.shape == (count, 2, N) and got.dtype == np.uint32
            assert np.array_equal(got, direct_table(p, rows, s1, m)), (m, count)


@pytest.mark.parametrize("p", [SECURITY_128_BIT, SECURITY_UINT4], ids=lambda p: p.name)
def test_table_model_is_the_window_over_the_sparse_packed_group(p):
    """Q is what the packing key switch returns for a 1,024-input group that holds c_x at slot x W and zero
    ciphertexts elsewhere."""
    sk, pk, rows = _key(p)
    rng = np.random.default_rng(32)
    for m in (2, 16, 512):
        W = N // m
        s1 = _words(rng, (m, 2, p.n + 1))
        got = PK.table_model(p, pk.mask_seed, pk.bodies, s1, m, rows=rows)
        for c in range(2):
            group = np.zeros((N, p.n + 1), np.uint32)
            group[np.arange(m) * W] = s1[:, c]
            Q = PK.pack_model(p, pk.mask_seed, pk.bodies, group, rows=rows)
            assert np.array_equal(got[c], PK.window(Q[0], m)), (m, c)


@pytest.mark.parametrize("m", [2, 4, 16, 64, 512])
def test_trivial_inputs_give_the_generators_table(m):
    """a = 0, b = v_x: no key word takes part, the a row is zero and the b row is Generator._assemble(v) word for word."""
    p = SECURITY_UINT4
    sk, pk, rows = _key(p)
    v = _words(np.random.default_rng(33 + m), (m, 2))
    s1 = np.zeros((m, 2, p.n + 1), np.uint32)
    s1[:, :, p.n] = v
    got = PK.table_model(p, pk.mask_seed, pk.bodies, s1, m, rows=rows)
    for c in range(2):
        assert not got[c, 0].any()
        assert np.array_equal(got[c, 1], Generator(m)._assemble(v[:, c]).poly[1]), (m, c)


@pytest.mark.parametrize("p", [SECURITY_80_BIT, SECURITY_UINT4], ids=lambda p: p.name)
def test_phase_is_the_table_of_the_input_phases_at_zero_noise(p):
    """A zero-noise packing key and noise-free inputs whose mask words are multiples of 2^(32 - basebit t) (the key
    switch's rounding is then exact): the phase of the table under s1 is _assemble(phases), exactly."""
    sk, pk, rows = _key(p, alpha=0.0)
    rng = np.random.default_rng(34)
    bt = p.basebit * p.iks_t
    for m in (4, 32):
        v = _words(rng, (m, 2))
        s1 = _words(rng, (m, 2, p.n + 1)) & np.uint32((0xFFFFFFFF << (32 - bt)) & 0xFFFFFFFF)
        inner = (s1[..., :p.n].astype(np.uint64) * sk.key_lv0.astype(np.uint64)[None, None, :]).sum(axis=-1)
        s1[..., p.n] = ((inner + v) & 0xFFFFFFFF).astype(np.uint32)
        assert np.array_equal(sk.phase(s1.reshape(-1, p.n + 1)).reshape(m, 2), v)
        tab = PK.table_model(p, pk.mask_seed, pk.bodies, s1, m, rows=rows)
        phase = tab[:, 1] - negacyclic_binary(tab[:, 0], sk.key_lv1)
        for c in range(2):
            assert np.array_equal(phase[c], Generator(m)._assemble(v[:, c]).poly[1]), (m, c)


def test_generate_bivariate_tables():
    T = np.random.default_rng(35).integers(0, 8, (8, 8))
    f = lambda x, y: int(T[x, y])  # noqa: E731
    g = Generator(8)
    one = g.generate_bivariate_tables(f)
    assert one.shape == (8, 2, N) and one.dtype == np.uint32
    for x in range(8):
        assert np.array_equal(one[x], g.generate_lookup_table(lambda y, x=x: f(x, y)).poly)
    for k in (2, 4, 8):
        tabs = g.generate_bivariate_tables(f, n_luts=k)
        assert tabs.shape == (8 // k, 2, N)
        for j in range(8 // k):
            fs = [(lambda y, x=j * k + r: f(x, y)) for r in range(k)]
            assert np.array_equal(tabs[j], g.generate_many_lookup_table(fs).poly), (k, j)
    for k in (0, 3, 16):
        with pytest.raises(ValueError):
            g.generate_bivariate_tables(f, n_luts=k)
    with pytest.raises(ValueError):  # k > m
        Generator(2).generate_bivariate_tables(f, n_luts=4)
    for m in (1, 3, 12, 1024):
        with pytest.raises(ValueError):
            Generator(m).generate_bivariate_tables(f)
    with pytest.raises(ValueError):
        PK.table_model(SECURITY_UINT4, bytes(32), None, np.zeros((3, 1, SECURITY_UINT4.n + 1), np.uint32), 3)


def test_tree_bootstrap_composed_on_the_oracle_decodes(O, keys_uint4):
    """SECURITY_UINT4, m = 4, k = 4, 32 inputs, a random table: stage 1 with the many-LUT model, table_model, then the
    oracle's bootstrap with one test vector per ciphertext -- every output decodes to f(x, y).  No allowance: the worst
    phase error of this composition is 0.051 of the decoding half-interval."""
    from test_many_lut_host import many_model

    sk, ck = keys_uint4
    p = SECURITY_UINT4
    m, k, count = 4, 4, 32
    pk = PK.make_packing_key(p, sk.key_lv0, sk.key_lv1, rng=4)
    rng = np.random.default_rng(36)
    T = rng.integers(0, m, (m, m))
    f = lambda x, y: int(T[x, y])  # noqa: E731
    xs, ys = rng.integers(0, m, count), rng.integers(0, m, count)
    cx, cy = sk.encrypt_lwe_message(xs, m, 21), sk.encrypt_lwe_message(ys, m, 22)
    tabs = Generator(m).generate_bivariate_tables(f, n_luts=k)
    stage1 = np.concatenate([many_model(O, ck, cy, tabs[j], k) for j in range(m // k)])
    assert stage1.shape == (m, count, p.n + 1)
    tv = PK.table_model(p, pk.mask_seed, pk.bodies, stage1, m)
    out = O.batch_bootstrap(ck, cx, testvec=tv)
    want = np.array([f(int(x), int(y)) for x, y in zip(xs, ys)])
    assert np.array_equal(sk.decrypt_lwe_message(out, m), want)


def test_new_exports_and_einval_without_a_device():
    lib = _capi.lib()
    for fn in NEW_EXPORTS:
        assert "tfhe_hip_" + fn in _capi.SIGNATURES, fn
        f = getattr(lib, "tfhe_hip_" + fn)
        args = [0 if t in (ctypes.c_size_t, ctypes.c_int) else None for t in f.argtypes]
        assert f(*args) == _capi.EINVAL, fn  # a NULL handle


def build_cpp_bivariate(outdir):
    """tests/cpp/test_bivariate.cpp, built as tests/test_gpu_packing.py builds the packing program."""
    exe = os.path.join(outdir, "test_bivariate")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_bivariate.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-pthread"])
    return exe


def test_cpp_bivariate_program_builds(tmp_path):
    """The C++ bindings' tree-bootstrap program compiles and links against the header and the library (run on the GPU
    by tests/test_gpu_table.py)."""
    assert os.path.exists(build_cpp_bivariate(str(tmp_path)))
