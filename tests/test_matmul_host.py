"""Encrypted linear layers on the host, no GPU: the integer models of rs_tfhe_amd.linear against a chain of two-term
linear combinations and against packing.extract_rows, exact phase linearity under a client key, the shape checks of the
Python wrappers, the four entry points in the header, the ctypes table and the Rust binding, and the C++ mirror
program's build."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rs_tfhe_amd import _capi, linear as L, packing as PK
from rs_tfhe_amd.client import SecretKey
from rs_tfhe_amd.params import N, PARAM_SETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("batch_tlwe_matmul", "batch_tlwe_matmul_dev", "batch_trlwe_matmul", "batch_trlwe_matmul_dev")
EDGES = (0, 0x80000000, 0xFFFFFFFF, 0x7F7F7F7F, 0x80808080, 0x00800080, 0x7FFFFFFF)  # carries between balanced byte planes


def lincomb(ca, a, cb, b, cconst):
    """tfhe_hip_batch_tlwe_lincomb's definition (include/tfhe_hip.h): ca*a + cb*b on every word, + cconst on the body."""
    out = np.uint32(ca & 0xFFFFFFFF) * a + np.uint32(cb & 0xFFFFFFFF) * b
    out[..., -1] += np.uint32(cconst & 0xFFFFFFFF)
    return out


def weights(rng, rows, cols):
    """Random in [-128, 127]; the first rows all -128, all 127, all 0."""
    w = rng.integers(-128, 128, (rows, cols)).astype(np.int8)
    for r, v in zip(range(rows), (-128, 127, 0)):
        w[r] = v
    return w


def plant_edges(words):
    """EDGES at column 0 and in the last column of every group of [groups][rows][width] words."""
    k = min(len(EDGES), words.shape[1])
    words[:, :k, 0] = EDGES[:k]
    words[:, :k, -1] = EDGES[:k]
    return words


@pytest.mark.parametrize("name,rows,cols,groups", [("SECURITY_80_BIT", 5, 9, 2), ("SECURITY_128_BIT", 33, 31, 1)])
def test_matmul_model_is_a_chain_of_lincombs(name, rows, cols, groups):
    p = PARAM_SETS[name]
    rng = np.random.default_rng(1)
    w = weights(rng, rows, cols)
    bias = rng.integers(0, 1 << 32, rows, dtype=np.uint32)
    cts = plant_edges(rng.integers(0, 1 << 32, (groups, cols, p.n + 1), dtype=np.uint32))
    got = L.matmul_model(p, w, cts, bias)
    assert got.shape == (groups, rows, p.n + 1) and got.dtype == np.uint32
    for g in range(groups):
        for r in range(rows):
            acc = np.zeros(p.n + 1, np.uint32)
            for j in range(cols):  # acc = 1 * acc + w[r][j] * cts[g][j]; the bias rides on the last term
                acc = lincomb(1, acc, int(w[r, j]), cts[g, j], int(bias[r]) if j == cols - 1 else 0)
            assert np.array_equal(got[g, r], acc), (g, r)
    assert np.array_equal(L.matmul_model(p, w, cts[0], bias), got[:1])  # [cols][n+1] is one group
    nobias = L.matmul_model(p, w, cts)
    assert np.array_equal(nobias[..., :-1], got[..., :-1]) and np.array_equal(nobias[..., -1] + bias, got[..., -1])


def test_one_hot_packed_model_is_extract_rows_with_the_exact_negation():
    p = PARAM_SETS["SECURITY_128_BIT"]
    trlwe = np.random.default_rng(2).integers(0, 1 << 32, (2, 2, N), dtype=np.uint32)
    trlwe[:, 0, :7] = EDGES
    for cols, hot in ((1, (0,)), (N, (0, 1, 517, N - 1))):
        w = np.zeros((len(hot), cols), np.int8)
        w[np.arange(len(hot)), hot] = 1
        got = L.matmul_packed_model(p, w, trlwe)
        assert got.shape == (2, len(hot), N + 1)
        for g in range(2):
            ref = PK.extract_rows(trlwe, [g * N + j for j in hot])
            negated = np.arange(N)[None, :] > np.array(hot)[:, None]  # words i > j
            assert np.array_equal(got[g, :, :N], ref[:, :N] + negated.astype(np.uint32))  # each exactly one higher
            assert np.array_equal(got[g, :, N], ref[:, N])
    assert np.array_equal(L.extract_rows_exact(trlwe, [N + 5])[0, 6:N], np.uint32(0) - trlwe[1, 0, :5:-1])
    with pytest.raises(ValueError):
        L.extract_rows_exact(trlwe, [2 * N])


@pytest.mark.parametrize("name", ["SECURITY_128_BIT", "SECURITY_UINT4"])
def test_phase_linearity_is_exact(name):
    """phase(out) == sum_j w * phase(in) + bias word for word mod 2^32, dense and packed, under a client key."""
    p = PARAM_SETS[name]
    sk = SecretKey.new(p, 31)
    rng = np.random.default_rng(3)
    rows, cols, groups = 6, 40, 2
    w = weights(rng, rows, cols)
    wi = w.astype(np.int64)
    bias = rng.integers(0, 1 << 32, rows, dtype=np.uint32)
    cts = rng.integers(0, 1 << 32, (groups, cols, p.n + 1), dtype=np.uint32)
    out = L.matmul_model(p, w, cts, bias)
    ph_in = sk.phase(cts.reshape(-1, p.n + 1)).reshape(groups, cols).astype(np.int64)
    want = ((wi @ ph_in.T).T + bias.astype(np.int64)) & 0xFFFFFFFF
    assert np.array_equal(sk.phase(out.reshape(-1, p.n + 1)).reshape(groups, rows), want.astype(np.uint32))
    # packed: the lv1 rows are ciphertexts under key_lv1; their phases against packed_phase of the slots
    trlwe = rng.integers(0, 1 << 32, (groups, 2, N), dtype=np.uint32)
    lv1 = L.matmul_packed_model(p, w, trlwe, bias)
    s1 = np.asarray(sk.key_lv1, np.uint32)
    ph_out = lv1[..., N] - (lv1[..., :N] * s1).sum(axis=-1, dtype=np.uint32)
    slots = sk.packed_phase(trlwe, groups * N).reshape(groups, N)[:, :cols].astype(np.int64)
    want = ((wi @ slots.T).T + bias.astype(np.int64)) & 0xFFFFFFFF
    assert np.array_equal(ph_out, want.astype(np.uint32))
    # the reference's negation instead would be off by sum_i s1[i] * sum_{j<i} w[r][j]: the reason for the exact one
    ref_rows = PK.extract_rows(trlwe, np.arange(cols)).reshape(1, cols, N + 1)
    off = L.matmul_model(p, w, ref_rows, bias)[0]
    ph_off = off[:, N] - (off[:, :N] * s1).sum(axis=-1, dtype=np.uint32)
    prefix = np.concatenate([np.zeros((rows, 1), np.int64), np.cumsum(wi, axis=1)], axis=1)  # sum_{j<i} w[r][j], i <= cols
    prefix = np.concatenate([prefix, np.repeat(prefix[:, -1:], N - cols - 1, axis=1)], axis=1)[:, :N]
    drift = (prefix * s1.astype(np.int64)).sum(axis=1)
    assert np.array_equal(ph_off, ((want[0] + drift) & 0xFFFFFFFF).astype(np.uint32))


class _NoKey:
    """A cloud key that must never be used: the checks come before the library."""

    def __init__(self, params):
        self.params = params

    def __getattr__(self, name):
        raise AssertionError("the call reached the cloud key: " + name)


def test_wrappers_reject_bad_shapes_before_the_library(monkeypatch):
    from rs_tfhe_amd import bootstrap

    def no_engine(*a, **k):
        raise AssertionError("the call reached the library")

    monkeypatch.setattr(bootstrap, "keyed_engine", no_engine)
    p = PARAM_SETS["SECURITY_80_BIT"]
    ck = _NoKey(p)
    w = np.ones((3, 4), np.int8)
    cts = np.zeros((2, 4, p.n + 1), np.uint32)
    trlwe = np.zeros((2, 2, N), np.uint32)
    bad_dense = [
        (np.ones((3, 5), np.int8), cts, None),            # cols differ
        (w, cts[:, :, :-1], None),                        # width
        (w, cts.reshape(-1), None),                       # not [groups][cols][n+1]
        (np.ones(4, np.int8), cts, None),                 # w not a matrix
        (np.ones((0, 4), np.int8), cts, None),            # rows == 0
        (np.ones((3, 0), np.int8), cts[:, :0], None),     # cols == 0
        (np.full((3, 4), 128), cts, None),                # beyond int8
        (np.ones((3, 4), np.float32), cts, None),         # not integers
        (w, cts, np.zeros(2, np.uint32)),                 # bias is [rows]
        (np.ones((1, L.MAX_COLS + 1), np.int8), np.zeros((1, 1, p.n + 1), np.uint32), None),
    ]
    for bw, bc, bb in bad_dense:
        with pytest.raises(ValueError):
            L.matmul(bw, bc, ck, bias=bb)
        with pytest.raises(ValueError):
            L.matmul_model(p, bw, bc, bb)
    bad_packed = [
        (np.ones((3, N + 1), np.int8), trlwe, None),      # cols > N
        (w, trlwe[:, :1], None),                          # not [groups][2][N]
        (w, trlwe.reshape(-1), None),
        (np.ones((0, 4), np.int8), trlwe, None),
        (w, trlwe, np.zeros(4, np.uint32)),
    ]
    for bw, bt, bb in bad_packed:
        with pytest.raises(ValueError):
            L.matmul_packed(bw, bt, ck, bias=bb)
    with pytest.raises(ValueError):
        L.matmul_packed_model(p, np.ones((3, N + 1), np.int8), trlwe)


def test_engine_methods_reject_bad_shapes_before_the_library():
    from test_engine_calls_host import _T, _engine, _refuses

    e = _engine()
    W = e.params.n + 1
    w = np.ones((3, 4), np.int8)
    _refuses(e, e.batch_tlwe_matmul, w, np.zeros((2, 5, W), np.uint32))
    _refuses(e, e.batch_tlwe_matmul, w, np.zeros((2, 4, W), np.uint32), np.zeros(2, np.uint32))
    _refuses(e, e.batch_tlwe_matmul, np.full((3, 4), 300), np.zeros((2, 4, W), np.uint32))
    _refuses(e, e.batch_trlwe_matmul, np.ones((3, N + 1), np.int8), np.zeros((1, 2, N), np.uint32))
    _refuses(e, e.batch_trlwe_matmul, w, np.zeros((1, 3, N), np.uint32))
    dev = e.device
    tw, tin, tout = _T((3, 4), dev, itemsize=1), _T((2, 4, W), dev), _T((2, 3, W), dev)
    _refuses(e, e.batch_tlwe_matmul_dev, _T((3, 4), dev, itemsize=4), tin, tout)      # w is int8
    _refuses(e, e.batch_tlwe_matmul_dev, tw, _T((2, 5, W), dev), tout)
    _refuses(e, e.batch_tlwe_matmul_dev, tw, tin, _T((2, 4, W), dev))
    _refuses(e, e.batch_trlwe_matmul_dev, tw, _T((2, 2, N), dev), _T((2, 3, N + 1), dev))  # keyswitch: [..][n+1]
    _refuses(e, e.batch_trlwe_matmul_dev, tw, _T((2, 2, N), dev), _T((2, 3, W), dev), keyswitch=False)
    out = e.batch_tlwe_matmul(w, np.zeros((2, 4, W), np.uint32))  # a good call goes through, once
    assert out.shape == (2, 3, W)
    assert [c[0] for c in e._lib.calls] == ["tfhe_hip_batch_tlwe_matmul"]
    assert e._lib.calls[0][1][3:5] == (3, 4) and e._lib.calls[0][1][6] == 2


def test_entry_points_in_the_header_the_ctypes_table_and_the_rust_binding():
    sz, vp, ci = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    want = {
        "batch_tlwe_matmul": [vp, vp, vp, sz, sz, vp, sz, vp],
        "batch_tlwe_matmul_dev": [vp, vp, vp, sz, sz, vp, sz, vp, vp],
        "batch_trlwe_matmul": [vp, vp, vp, sz, sz, vp, sz, ci, vp],
        "batch_trlwe_matmul_dev": [vp, vp, vp, sz, sz, vp, sz, ci, vp, vp],
    }
    assert set(want) == set(ENTRY_POINTS)
    with open(os.path.join(ROOT, "include", "tfhe_hip.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "rust", "src", "bootstrap", "hip.rs")) as fh:
        rust = fh.read()
    ffi = "\n".join(re.findall(r'extern "C" \{(.*?)\n\}', rust, flags=re.S))
    for fn, args in want.items():
        res, argtypes = _capi.SIGNATURES["tfhe_hip_" + fn]
        assert res is ci and list(argtypes) == args, fn
        assert "int tfhe_hip_" + fn + "(" in header, fn
        assert "fn tfhe_hip_" + fn + "(" in ffi, fn
    assert "pub fn tlwe_matmul(" in rust and "pub fn trlwe_matmul(" in rust
    lib = _capi.lib()
    for fn in ENTRY_POINTS:
        f = getattr(lib, "tfhe_hip_" + fn)  # AttributeError: not exported
        assert f(*[0 if t in (sz, ci) else None for t in f.argtypes]) == _capi.EINVAL, fn  # NULL context


def build_cpp_matmul(outdir):
    """tests/cpp/test_matmul.cpp, built as test_unpack_host.build_cpp_unpack builds the unpacking program."""
    exe = os.path.join(outdir, "test_matmul")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_matmul.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-L" + os.path.join(ROOT, "oracle"), "-ltfhe_oracle",
        "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-fopenmp", "-pthread"])
    return exe


def test_cpp_matmul_program_builds(O, tmp_path):
    """The C++ mirror's linear::matmul / matmul_packed program compiles and links against the header and both libraries
    (run on the GPU by tests/test_gpu_matmul.py)."""
    assert os.path.exists(build_cpp_matmul(str(tmp_path)))
