"""Encrypted 2-D convolution on the host, no GPU: linear.conv2d_model against a direct six-loop evaluation of the header's
definition and against matmul_model at a 1 x 1 filter, the output-shape formula, every ValueError of the Python checks,
the argument checks of Engine.batch_tlwe_conv2d[_dev] on a stand-in library, the two entry points in the header, the
ctypes table, the struct and the Rust binding, and the C++ mirror program's build."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from rs_tfhe_amd import _capi, linear as L
from rs_tfhe_amd.params import PARAM_SETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("batch_tlwe_conv2d", "batch_tlwe_conv2d_dev")
FIELDS = ("in_h", "in_w", "in_c", "out_c", "k_h", "k_w", "stride_h", "stride_w", "pad_h", "pad_w")


def direct(w, cts, bias, stride, padding):
    """The header's definition, one loop per index: out[g][oy][ox][oc] = sum_{ky,kx,ic} w * in (zero outside) + bias."""
    out_c, k_h, k_w, in_c = w.shape
    groups, in_h, in_w, _, width = cts.shape
    (sh, sw), (ph, pw) = stride, padding
    out_h, out_w = (in_h + 2 * ph - k_h) // sh + 1, (in_w + 2 * pw - k_w) // sw + 1
    out = np.zeros((groups, out_h, out_w, out_c, width), np.uint32)
    for g in range(groups):
        for oy in range(out_h):
            for ox in range(out_w):
                for oc in range(out_c):
                    acc = np.zeros(width, np.uint32)
                    for ky in range(k_h):
                        for kx in range(k_w):
                            iy, ix = oy * sh + ky - ph, ox * sw + kx - pw
                            if not (0 <= iy < in_h and 0 <= ix < in_w):
                                continue
                            for ic in range(in_c):
                                acc += np.uint32(int(w[oc, ky, kx, ic]) & 0xFFFFFFFF) * cts[g, iy, ix, ic]
                    if bias is not None:
                        acc[-1:] += bias[oc:oc + 1]
                    out[g, oy, ox, oc] = acc
    return out


def test_model_is_the_six_loop_definition():
    p = PARAM_SETS["SECURITY_80_BIT"]
    rng = np.random.default_rng(1)
    w = rng.integers(-128, 128, (2, 2, 3, 3)).astype(np.int8)
    w[0, 0, 0], w[1, 1, 2] = (-128, 127, 0), (127, -128, -1)
    bias = rng.integers(0, 1 << 32, 2, dtype=np.uint32)
    cts = rng.integers(0, 1 << 32, (2, 4, 5, 3, p.n + 1), dtype=np.uint32)
    cts[:, 0, 0, 0, :3] = (0xFFFFFFFF, 0x80000000, 0x80808080)
    got = L.conv2d_model(p, w, cts, bias, stride=(2, 1), padding=(1, 0))
    assert got.shape == (2, 3, 3, 2, p.n + 1) and got.dtype == np.uint32
    assert np.array_equal(got, direct(w, cts, bias, (2, 1), (1, 0)))
    assert np.array_equal(L.conv2d_model(p, w, cts[0], bias, (2, 1), (1, 0)), got[:1])  # four axes: one group
    nobias = L.conv2d_model(p, w, cts, None, (2, 1), (1, 0))
    assert np.array_equal(nobias[..., :-1], got[..., :-1])
    assert np.array_equal(nobias[..., -1] + bias[None, None, None, :], got[..., -1])
    # an int stands for both axes
    assert np.array_equal(L.conv2d_model(p, w, cts, bias, 2, 1), direct(w, cts, bias, (2, 2), (1, 1)))


def test_one_by_one_filter_is_the_dense_form():
    p = PARAM_SETS["SECURITY_128_BIT"]
    rng = np.random.default_rng(2)
    w = rng.integers(-128, 128, (5, 1, 1, 7)).astype(np.int8)
    bias = rng.integers(0, 1 << 32, 5, dtype=np.uint32)
    cts = rng.integers(0, 1 << 32, (2, 3, 4, 7, p.n + 1), dtype=np.uint32)
    got = L.conv2d_model(p, w, cts, bias)
    want = L.matmul_model(p, w.reshape(5, 7), cts.reshape(2 * 3 * 4, 7, p.n + 1), bias)
    assert np.array_equal(got, want.reshape(2, 3, 4, 5, p.n + 1))


def test_output_shape_formula():
    assert L.conv2d_out_shape(5, 5, 3, 3, 1, 1) == (5, 5)
    assert L.conv2d_out_shape(7, 8, 3, 3, (2, 3), 0) == (3, 2)
    assert L.conv2d_out_shape(2, 2, 3, 3, 1, 2) == (4, 4)  # pad = k - 1
    assert L.conv2d_out_shape(1, 9, 1, 4, 1, 0) == (1, 6)  # one-dimensional
    assert L.conv2d_out_shape(4, 5, 2, 3, (2, 1), (1, 0)) == (3, 3)
    assert L.conv2d_out_shape(3, 3, 3, 3, 5, 0) == (1, 1)  # a stride past the map
    for in_h in range(1, 7):
        for k in range(1, 4):
            for s in range(1, 4):
                for pad in range(0, 3):
                    if k > in_h + 2 * pad:
                        with pytest.raises(ValueError):
                            L.conv2d_out_shape(in_h, in_h, k, k, s, pad)
                        continue
                    # the positions oy with oy * s + k <= in_h + 2 pad
                    want = len([oy for oy in range(in_h + 2 * pad) if oy * s + k <= in_h + 2 * pad])
                    assert L.conv2d_out_shape(in_h, 9, k, 1, s, pad) == (want, (9 + 2 * pad - 1) // s + 1)
    p = PARAM_SETS["SECURITY_80_BIT"]
    out = L.conv2d_model(p, np.ones((2, 3, 2, 1), np.int8), np.zeros((1, 7, 8, 1, p.n + 1), np.uint32), None, (2, 3), (0, 1))
    assert out.shape == (1,) + L.conv2d_out_shape(7, 8, 3, 2, (2, 3), (0, 1)) + (2, p.n + 1)


class _NoKey:
    """A cloud key that must never be used: the checks come before the library."""

    def __init__(self, params):
        self.params = params

    def __getattr__(self, name):
        raise AssertionError("the call reached the cloud key: " + name)


def test_python_checks_raise_before_the_library(monkeypatch):
    from rs_tfhe_amd import bootstrap

    def no_engine(*a, **k):
        raise AssertionError("the call reached the library")

    monkeypatch.setattr(bootstrap, "keyed_engine", no_engine)
    p = PARAM_SETS["SECURITY_80_BIT"]
    ck = _NoKey(p)
    w = np.ones((2, 3, 3, 4), np.int8)
    cts = np.zeros((2, 5, 5, 4, p.n + 1), np.uint32)
    bad = [
        (np.ones((2, 3, 3, 5), np.int8), cts, None, 1, 0),          # in_c differs
        (w, cts[..., :-1], None, 1, 0),                            # width
        (w, cts.reshape(-1), None, 1, 0),                          # not a feature map
        (w, cts.reshape(2, 25, 4, p.n + 1)[:, :, None, None], None, 1, 0),  # six axes
        (np.ones((2, 9, 4), np.int8), cts, None, 1, 0),            # w not [out_c][k_h][k_w][in_c]
        (np.ones((0, 3, 3, 4), np.int8), cts, None, 1, 0),         # out_c == 0
        (np.ones((2, 0, 3, 4), np.int8), cts, None, 1, 0),         # k_h == 0
        (np.ones((2, 3, 3, 0), np.int8), cts[:, :, :, :0], None, 1, 0),  # in_c == 0
        (np.full((2, 3, 3, 4), 128), cts, None, 1, 0),             # beyond int8
        (np.ones((2, 3, 3, 4), np.float32), cts, None, 1, 0),      # not integers
        (w, cts, np.zeros(3, np.uint32), 1, 0),                    # bias is [out_c]
        (w, cts, None, 0, 0),                                      # stride 0
        (w, cts, None, (1, 0), 0),
        (w, cts, None, (1, 1, 1), 0),                              # not a pair
        (w, cts, None, 1.5, 0),
        (w, cts, None, 1, -1),                                     # negative padding
        (w, cts, None, 1, (0, -1)),
        (np.ones((2, 6, 3, 4), np.int8), cts, None, 1, 0),         # filter taller than the map
        (np.ones((2, 3, 8, 4), np.int8), cts, None, 1, (5, 1)),    # wider than the padded map
        (np.ones((1, 129, 128, 4), np.int8), np.zeros((1, 129, 128, 4, 1), np.uint32), None, 1, 0),  # K = 66,048 > 65,536
    ]
    for bw, bc, bb, st, pad in bad:
        with pytest.raises(ValueError):
            L.conv2d(bw, bc, ck, bias=bb, stride=st, padding=pad)
        with pytest.raises(ValueError):
            L.conv2d_model(p, bw, bc, bb, st, pad)
    for args in ((0, 5, 1, 1), (5, 5, 0, 1), (5, 5, 6, 1), (5, 5, 1, 6)):
        with pytest.raises(ValueError):
            L.conv2d_out_shape(*args)
    with pytest.raises(ValueError):
        L.conv2d_out_shape(5, 5, 3, 3, stride=0)
    with pytest.raises(ValueError):
        L.conv2d_out_shape(5, 5, 3, 3, padding=-1)


def test_engine_methods_reject_bad_arguments_before_the_library():
    from test_engine_calls_host import _T, _engine, _refuses

    e = _engine()
    W = e.params.n + 1
    w = np.ones((2, 3, 3, 4), np.int8)
    cts = np.zeros((2, 5, 6, 4, W), np.uint32)
    _refuses(e, e.batch_tlwe_conv2d, np.ones((2, 3, 3, 5), np.int8), cts)                   # in_c differs
    _refuses(e, e.batch_tlwe_conv2d, np.ones((2, 9, 4), np.int8), cts)                      # w has four axes
    _refuses(e, e.batch_tlwe_conv2d, np.full((2, 3, 3, 4), 300), cts)                       # beyond int8
    _refuses(e, e.batch_tlwe_conv2d, w, cts[..., :-1])                                      # width
    _refuses(e, e.batch_tlwe_conv2d, w, cts.reshape(2, 30, 4, W)[:, :, None, None])         # six axes
    _refuses(e, e.batch_tlwe_conv2d, w, cts, np.zeros(3, np.uint32))                        # bias is [out_c]
    _refuses(e, e.batch_tlwe_conv2d, w, cts, None, 0)                                       # stride
    _refuses(e, e.batch_tlwe_conv2d, w, cts, None, 1, -1)                                   # padding
    _refuses(e, e.batch_tlwe_conv2d, w, cts, None, (1, 2, 3))
    _refuses(e, e.batch_tlwe_conv2d, np.ones((2, 6, 3, 4), np.int8), cts)                   # filter taller than the map
    _refuses(e, e.batch_tlwe_conv2d, np.ones((1, 129, 128, 4), np.int8), np.zeros((1, 129, 128, 4, W), np.uint32))  # K
    dev = e.device
    tw, tin = _T((2, 3, 3, 4), dev, itemsize=1), _T((2, 5, 6, 4, W), dev)
    tout = _T((2, 2, 4, 2, W), dev)  # stride (2, 1), padding (0, 1): 2 x 6 -> (5 - 3) / 2 + 1 = 2, (6 + 2 - 3) / 1 + 1 = 6
    _refuses(e, e.batch_tlwe_conv2d_dev, _T((2, 3, 3, 4), dev, itemsize=4), tin, tout)      # w is int8
    _refuses(e, e.batch_tlwe_conv2d_dev, _T((2, 3, 3, 4), dev + 1, itemsize=1), tin, tout)  # another GPU
    _refuses(e, e.batch_tlwe_conv2d_dev, tw, _T((5, 6, 4, W), dev), tout)                   # the device form takes five axes
    _refuses(e, e.batch_tlwe_conv2d_dev, tw, _T((2, 5, 6, 5, W), dev), tout)
    _refuses(e, e.batch_tlwe_conv2d_dev, tw, tin, tout, stride=(2, 1), padding=(0, 1))      # out is [2][2][6][2][W]
    _refuses(e, e.batch_tlwe_conv2d_dev, tw, tin, _T((2, 2, 6, 2, W), dev), bias=_T((3,), dev), stride=(2, 1), padding=(0, 1))
    # good calls go through once each, with the shape the header defines
    seen = []
    e._lib.hooks["tfhe_hip_batch_tlwe_conv2d"] = lambda args: seen.append(tuple(getattr(args[1].contents, f) for f in FIELDS))
    out = e.batch_tlwe_conv2d(w, cts, np.zeros(2, np.uint32), stride=(2, 1), padding=(0, 1))
    assert out.shape == (2, 2, 6, 2, W) and out.dtype == np.uint32
    assert [c[0] for c in e._lib.calls] == ["tfhe_hip_batch_tlwe_conv2d"]
    assert seen == [(5, 6, 4, 2, 3, 3, 2, 1, 0, 1)]
    assert e._lib.calls[0][1][5] == 2  # groups
    assert e.batch_tlwe_conv2d(w, cts[0], padding=1).shape == (1, 5, 6, 2, W)  # four axes: one group
    assert e.batch_tlwe_conv2d(w, cts[:0]).shape == (0, 3, 4, 2, W)  # the empty batch
    e._lib.calls.clear()
    e._lib.hooks["tfhe_hip_batch_tlwe_conv2d_dev"] = lambda args: seen.append(tuple(getattr(args[1].contents, f) for f in FIELDS))
    e.batch_tlwe_conv2d_dev(tw, tin, _T((2, 2, 6, 2, W), dev), bias=_T((2,), dev), stride=(2, 1), padding=(0, 1),
                            stream=_stream(dev))
    assert [c[0] for c in e._lib.calls] == ["tfhe_hip_batch_tlwe_conv2d_dev"]
    assert seen[-1] == (5, 6, 4, 2, 3, 3, 2, 1, 0, 1)
    args = e._lib.calls[0][1]
    assert args[2] == tw.data_ptr() and args[4] == tin.data_ptr() and args[5] == 2 and args[7] == 0x777


def _stream(dev):
    from test_engine_calls_host import _S

    return _S(dev)


def test_entry_points_in_the_header_the_ctypes_table_and_the_rust_binding():
    sz, vp, ci = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
    sp = ctypes.POINTER(_capi.Conv2dShape)
    want = {
        "batch_tlwe_conv2d": [vp, sp, vp, vp, vp, sz, vp],
        "batch_tlwe_conv2d_dev": [vp, sp, vp, vp, vp, sz, vp, vp],
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
    assert "pub fn tlwe_conv2d(" in rust and "pub unsafe fn tlwe_conv2d_dev(" in rust
    # the struct: ten u32 fields in the header's order, in ctypes and in the Rust binding
    m = re.search(r"typedef struct tfhe_hip_conv2d_shape \{(.*?)\} tfhe_hip_conv2d_shape;", header, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("uint32_t "), decl
            names += [x.strip() for x in decl[len("uint32_t "):].split(",")]
    assert tuple(names) == FIELDS
    assert tuple(f for f, _ in _capi.Conv2dShape._fields_) == FIELDS
    assert all(t is ctypes.c_uint32 for _, t in _capi.Conv2dShape._fields_) and ctypes.sizeof(_capi.Conv2dShape) == 40
    m = re.search(r"pub struct TfheHipConv2dShape \{(.*?)\n\}", rust, flags=re.S)
    assert tuple(re.findall(r"pub (\w+): u32", m.group(1))) == FIELDS
    lib = _capi.lib()
    for fn in ENTRY_POINTS:
        f = getattr(lib, "tfhe_hip_" + fn)  # AttributeError: not exported
        assert f(*[0 if t is sz else None for t in f.argtypes]) == _capi.EINVAL, fn  # NULL context


def test_the_documents_name_the_call():
    for doc, words in (("INTEGRATION.md", ("tfhe_hip_batch_tlwe_conv2d", "linear::conv2d", "HipEngine::tlwe_conv2d")),
                       ("README.md", ("tfhe_hip_batch_tlwe_conv2d", "conv2d_bench.json")),
                       ("DESIGN.md", ("tfhe_hip_batch_tlwe_conv2d", "MmConv", "conv2d_bench.json"))):
        with open(os.path.join(ROOT, doc)) as fh:
            text = fh.read()
        for word in words:
            assert word in text, (doc, word)


def build_cpp_conv2d(outdir):
    """tests/cpp/test_conv2d.cpp, built as test_matmul_host.build_cpp_matmul builds the linear layers' program (no
    oracle library: the program checks against its own loops)."""
    exe = os.path.join(outdir, "test_conv2d")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_conv2d.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-fopenmp", "-pthread"])
    return exe


def test_cpp_conv2d_program_builds(tmp_path):
    """The C++ mirror's linear::conv2d program compiles and links against the header and the library (run on the GPU by
    tests/test_gpu_conv2d.py)."""
    assert os.path.exists(build_cpp_conv2d(str(tmp_path)))
