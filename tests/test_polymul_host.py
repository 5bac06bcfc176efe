"""Plaintext polynomial products on packed ciphertexts, host side (no GPU): rs_tfhe_amd.linear.polymul_model against the
schoolbook double sum of the header's definition, monomial, the packed-convolution plan and its weights against a direct
integer convolution, phase exactness under a real key, and the argument checks of Engine.batch_trlwe_polymul[_dev] that
need no device."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from rs_tfhe_amd import engine as E
from rs_tfhe_amd import linear as L
from rs_tfhe_amd.params import N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = ((4, 16, 16, 3, 3, 1), (1, 32, 32, 5, 5, 1), (16, 8, 8, 3, 3, 1), (3, 18, 18, 1, 3, 1), (2, 20, 20, 3, 3, 2))


def schoolbook(w, trlwe, bias=None):
    """out[g][r][c][i] = sum_j sum_m w[r][j][m] * ext_{in[g][j][c]}[i - m] + (c == b ? bias[r][i] : 0), the sums as
    written in include/tfhe_hip.h: ext is laid out at index t + N, its lower half the exact wrapping negation."""
    w = np.asarray(w).astype(np.int64)
    rows, cols = w.shape[:2]
    groups = trlwe.shape[0]
    out = np.zeros((groups, rows, 2, N), np.uint32)
    for g in range(groups):
        for j in range(cols):
            for c in range(2):
                p = trlwe[g, j, c]
                ext = np.concatenate([np.uint32(0) - p, p])  # ext[t + N]
                for m in range(N):
                    col = w[:, j, m]
                    if not col.any():
                        continue
                    sl = ext[N - m:2 * N - m]  # ext[i - m], i = 0 .. N-1
                    out[g, :, c] += (col[:, None] & 0xFFFFFFFF).astype(np.uint32) * sl[None, :]
    if bias is not None:
        out[:, :, 1] += bias
    return out


def negacyclic_int(w, p):
    """w(X) * p(X) mod X^N + 1 for one int8 polynomial and one u32 polynomial, by the schoolbook sum."""
    return schoolbook(np.asarray(w).reshape(1, 1, N), np.stack([p, p])[None, None])[0, 0, 0]


def test_model_equals_the_schoolbook_double_sum():
    rng = np.random.default_rng(1)
    w = rng.integers(-128, 128, (2, 2, N)).astype(np.int8)
    w[0, 0, 0], w[0, 0, N - 1], w[1, 1, 0], w[1, 1, N - 1] = -128, 127, 127, -128
    trlwe = rng.integers(0, 1 << 32, (1, 2, 2, N), dtype=np.uint32)
    trlwe[0, :, :, 0] = [[0, 0x80000000], [0xFFFFFFFF, 0]]
    trlwe[0, :, :, N - 1] = [[0x80000000, 0xFFFFFFFF], [0, 0x80000000]]
    bias = rng.integers(0, 1 << 32, (2, N), dtype=np.uint32)
    got = L.polymul_model(w, trlwe, bias)
    assert got.shape == (1, 2, 2, N) and got.dtype == np.uint32
    assert np.array_equal(got, schoolbook(w, trlwe, bias))
    assert np.array_equal(L.polymul_model(w, trlwe), schoolbook(w, trlwe))
    assert np.array_equal(L.polymul_model(w, trlwe[0]), got - np.pad(bias[None, :, None], ((0, 0), (0, 0), (1, 0), (0, 0))))


def test_model_accepts_the_packers_layouts_and_refuses_the_rest():
    rng = np.random.default_rng(2)
    packed = rng.integers(0, 1 << 32, (3, 2, N), dtype=np.uint32)  # what pack / encrypt_packed_* return
    w = rng.integers(-128, 128, N).astype(np.int8)
    got = L.polymul_model(w, packed)
    assert got.shape == (3, 1, 2, N)
    assert np.array_equal(got[1, 0], L.polymul_model(w[None, None], packed[1])[0, 0])
    for bad_w in (np.zeros((1, 1, N - 1), np.int8), np.zeros((1, 65, N), np.int8), np.zeros((0, 1, N), np.int8),
                  np.full((1, 1, N), 128), np.zeros((1, 1, N), np.float32), np.zeros((2, N), np.int8)):
        with pytest.raises(ValueError):
            L.polymul_model(bad_w, packed)
    with pytest.raises(ValueError):
        L.polymul_model(np.zeros((1, 2, N), np.int8), packed[:1])  # [1][2][N] is not [cols = 2][2][N]
    with pytest.raises(ValueError):
        L.polymul_model(w, packed, bias=np.zeros((2, N), np.uint32))


def test_monomial():
    rng = np.random.default_rng(3)
    p = rng.integers(0, 1 << 32, (1, 2, N), dtype=np.uint32)
    for k in (0, 1, 17, N - 1):
        for sign in (1, -1):
            w = L.monomial(k, sign)
            assert w.shape == (N,) and w.dtype == np.int8 and w[k] == sign and np.count_nonzero(w) == 1
            rot = np.concatenate([np.uint32(0) - p[0, :, N - k:], p[0, :, :N - k]], axis=1)  # slot i -> i + k, wrapped negated
            assert np.array_equal(L.polymul_model(w, p)[0, 0], rot if sign > 0 else np.uint32(0) - rot)
    for bad in ((-1, 1), (N, 1), (0, 0), (0, 2), (1.5, 1)):
        with pytest.raises(ValueError):
            L.monomial(*bad)


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_packed_convolution_plan_equals_a_direct_convolution(geo):
    """Trivial ciphertexts (a = 0, b = random u32 words) and int8 filters over the full range: the b row of the product
    at the plan's slots is the direct integer convolution mod 2^32, exactly."""
    in_c, in_h, in_w, k_h, k_w, stride = geo
    rng = np.random.default_rng(sum(geo))
    plan = L.conv2d_packed_plan(in_c, in_h, in_w, k_h, k_w, stride)
    out_h, out_w = (in_h - k_h) // stride + 1, (in_w - k_w) // stride + 1
    assert (plan.out_h, plan.out_w) == (out_h, out_w) and plan.slots.shape == (out_h, out_w) and plan.slots.dtype == np.uint32
    assert plan.slots.max() < N and plan.slots.min() == plan.offset
    fmap = rng.integers(0, 1 << 32, (in_c, in_h, in_w), dtype=np.uint32)
    f = rng.integers(-128, 128, (3, k_h, k_w, in_c)).astype(np.int8)
    f[0], f[1] = -128, 127
    ct = np.zeros((1, 1, 2, N), np.uint32)
    ct[0, 0, 1] = plan.encode(fmap)
    assert np.array_equal(ct[0, 0, 1, :fmap.size].reshape(fmap.shape), fmap)  # index c H W + y W + x
    wp = L.conv2d_packed_weights(f, plan)
    assert wp.shape == (3, 1, N) and wp.dtype == np.int8
    prod = L.polymul_model(wp, ct)
    assert not prod[0, :, 0].any()
    want = np.zeros((3, out_h, out_w), np.uint32)
    f32 = (f.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    for ky in range(k_h):
        for kx in range(k_w):
            win = fmap[:, ky:ky + (out_h - 1) * stride + 1:stride, kx:kx + (out_w - 1) * stride + 1:stride]  # [c][oy][ox]
            want += (f32[:, ky, kx, :, None, None] * win[None]).sum(axis=1, dtype=np.uint32)
    assert np.array_equal(prod[0, :, 1][:, plan.slots], want)


def test_packed_convolution_plan_refuses_what_does_not_fit():
    L.conv2d_packed_plan(1, 32, 32, 3, 3)  # exactly N values
    for bad in ((1, 32, 33, 3, 3), (17, 8, 8, 3, 3), (0, 8, 8, 3, 3), (1, 8, 8, 9, 3), (1, 8, 8, 3, 0)):
        with pytest.raises(ValueError):
            L.conv2d_packed_plan(*bad)
    with pytest.raises(ValueError):
        L.conv2d_packed_plan(1, 8, 8, 3, 3, stride=0)
    plan = L.conv2d_packed_plan(2, 8, 8, 3, 3)
    with pytest.raises(ValueError):
        L.conv2d_packed_weights(np.zeros((1, 3, 3, 3), np.int8), plan)  # in_c differs
    with pytest.raises(ValueError):
        plan.encode(np.zeros((2, 8, 9)))


def test_phase_is_exact_under_a_real_key():
    """packed_phase(out) == w(X) * packed_phase(in) + bias(X), word for word: the phase is linear over Z[X] / (X^N + 1)."""
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    rng = np.random.default_rng(5)
    sk = SecretKey.new(p, 51)
    packed = sk.encrypt_packed_lwe_message(rng.integers(0, 16, 2 * N), 16, seed=52)  # [2][2][N]: cols = 2, one group
    w = np.zeros((2, 2, N), np.int8)
    w[0] = rng.integers(-128, 128, (2, N))
    w[1, 0], w[1, 1] = L.monomial(5), L.monomial(1000, -1)
    bias = rng.integers(0, 1 << 32, (2, N), dtype=np.uint32)
    out = L.polymul_model(w, packed[None], bias)
    ph_in = sk.packed_phase(packed, 2 * N).reshape(2, N)
    for r in range(2):
        want = negacyclic_int(w[r, 0], ph_in[0]) + negacyclic_int(w[r, 1], ph_in[1]) + bias[r]
        assert np.array_equal(sk.packed_phase(out[0, r], N), want), r


# ---- Engine.batch_trlwe_polymul[_dev]: what is refused before anything reaches the library ---------------------------------
P = types.SimpleNamespace(n=4, l=2, iks_t=2, base=4, alpha_lv0=1.5e-5, alpha_lv1=2.5e-8)
HANDLE = 0x5A5A0


class _Lib:
    """Records (symbol, arguments) of every call and returns 0 (TFHE_HIP_OK)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("tfhe_hip_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, tuple(x.value if isinstance(x, C._SimpleCData) else x for x in args)))
            return 0

        return fn


def _engine():
    e = E.Engine.__new__(E.Engine)
    e.params, e.device, e._lib, e._ctx = P, 3, _Lib(), C.c_void_p(HANDLE)
    e._owner, e._parent, e._views, e._key = None, None, [], None
    return e


def test_engine_forwards_the_host_form():
    e = _engine()
    w = np.ones((3, 2, N), np.int8)
    trlwe = np.zeros((4, 2, 2, N), np.uint32)
    bias = np.zeros((3, N), np.uint32)
    out = e.batch_trlwe_polymul(w, trlwe, bias)
    assert out.shape == (4, 3, 2, N) and out.dtype == np.uint32
    (name, args), = e._lib.calls
    assert name == "tfhe_hip_batch_trlwe_polymul"
    assert args[0] == HANDLE and args[1] == w.ctypes.data and args[2] == bias.ctypes.data
    assert args[3:5] == (3, 2) and args[5] == trlwe.ctypes.data and args[6] == 4 and args[7] == out.ctypes.data
    e._lib.calls.clear()
    assert e.batch_trlwe_polymul(L.monomial(3), np.zeros((5, 2, N), np.uint32)).shape == (5, 1, 2, N)  # [groups][2][N]
    (name, args), = e._lib.calls
    assert args[2] is None and args[3:5] == (1, 1) and args[6] == 5
    e._lib.calls.clear()
    assert e.batch_trlwe_polymul(w, trlwe[:0]).shape == (0, 3, 2, N)  # groups == 0 still reaches the library
    assert e._lib.calls[0][1][6] == 0


def test_engine_refuses_malformed_operands():
    e = _engine()
    w = np.ones((3, 2, N), np.int8)
    trlwe = np.zeros((4, 2, 2, N), np.uint32)
    for bad_w in (np.ones((3, 2, N - 1), np.int8), np.ones((3, 65, N), np.int8), np.ones((0, 2, N), np.int8),
                  np.full((3, 2, N), 128), np.full((3, 2, N), -129), np.ones((3, 2, N), np.float64), np.ones((3, N), np.int8)):
        with pytest.raises(ValueError):
            e.batch_trlwe_polymul(bad_w, trlwe)
    for bad_t in (np.zeros((4, 3, 2, N), np.uint32), np.zeros((4, 2, N), np.uint32), np.zeros((4, 2, 2, N - 1), np.uint32),
                  np.zeros((4, 2, 1, N), np.uint32)):
        with pytest.raises(ValueError):
            e.batch_trlwe_polymul(w, bad_t)
    for bad_b in (np.zeros(3, np.uint32), np.zeros((2, N), np.uint32), np.zeros((3, N + 1), np.uint32)):
        with pytest.raises(ValueError):
            e.batch_trlwe_polymul(w, trlwe, bad_b)
    with pytest.raises(ValueError):
        e.batch_trlwe_polymul_dev(None, None, None)
    assert e._lib.calls == []


def test_every_layer_declares_the_call_and_the_documents_name_it():
    from rs_tfhe_amd import _capi

    def text(*path):
        with open(os.path.join(ROOT, *path)) as fh:
            return fh.read()

    header, rust = text("include", "tfhe_hip.h"), text("rust", "src", "bootstrap", "hip.rs")
    for fn, nargs in (("batch_trlwe_polymul", 8), ("batch_trlwe_polymul_dev", 9)):
        assert "int tfhe_hip_" + fn + "(" in header and "fn tfhe_hip_" + fn + "(" in rust, fn
        assert len(_capi.SIGNATURES["tfhe_hip_" + fn][1]) == nargs
        f = getattr(_capi.lib(), "tfhe_hip_" + fn)  # AttributeError: not exported
        assert f(*[0 if t is C.c_size_t else None for t in f.argtypes]) == _capi.EINVAL, fn  # NULL context
    assert "pub fn trlwe_polymul(" in rust and "pub unsafe fn trlwe_polymul_dev(" in rust
    mirror = text("include", "rs_tfhe_hip.hpp")
    assert "inline std::vector<Torus> polymul(" in mirror and "inline std::vector<int8_t> monomial(" in mirror
    for doc, words in (("INTEGRATION.md", ("tfhe_hip_batch_trlwe_polymul", "linear::polymul", "HipEngine::trlwe_polymul")),
                       ("README.md", ("tfhe_hip_batch_trlwe_polymul", "polymul_bench.json")),
                       ("DESIGN.md", ("tfhe_hip_batch_trlwe_polymul", "MmNegacyclic", "polymul_bench.json"))):
        for word in words:
            assert word in text(doc), (doc, word)


def build_cpp_polymul(outdir):
    """tests/cpp/test_polymul.cpp, built as test_conv2d_host.build_cpp_conv2d builds the convolution's program (no oracle
    library: the program checks against its own loops)."""
    exe = os.path.join(outdir, "test_polymul")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_polymul.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-fopenmp", "-pthread"])
    return exe


def test_cpp_polymul_program_builds(tmp_path):
    """The C++ mirror's linear::polymul / monomial program compiles and links against the header and the library (run on
    the GPU by tests/test_gpu_polymul.py)."""
    assert os.path.exists(build_cpp_polymul(str(tmp_path)))
