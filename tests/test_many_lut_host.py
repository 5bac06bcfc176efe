"""Many-LUT programmable bootstrap, host side: the packed test vector (Generator.generate_many_lookup_table), the
pre-rounding model the GPU kernels are held to (run on the CPU oracle), the circuit scheduler's many-LUT groups
(compiled without a device) and argument checking."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest


def _gen(m):
    from rs_tfhe_amd.lut import Generator

    return Generator(m)


def _unrotate(poly, m):
    """generate_lookup_table's rotation undone: raw[pos] for every table position (negation of the wrapped tail
    reverted)."""
    from rs_tfhe_amd.lut import div_round

    size = poly.shape[-1]
    off = div_round(size, 2 * m)
    rot = poly[1].astype(np.int64)
    rot[size - off:] = (-rot[size - off:]) % (1 << 32)
    raw = np.empty(size, np.int64)
    raw[(np.arange(size) + off) % size] = rot
    return raw


@pytest.mark.parametrize("m,k", [(8, 2), (4, 4), (2, 8), (16, 2), (4, 2)])
def test_packing_box_and_residue(m, k):
    """Position r of message x's box holds encode(f_(r mod k)(x))."""
    fs = [(lambda j: (lambda x: (3 * x + j) % m))(j) for j in range(k)]
    g = _gen(m)
    poly = g.generate_many_lookup_table(fs).poly
    assert not poly[0].any()
    raw = _unrotate(poly, m)
    box = raw.size // m
    for x in range(m):
        for r in range(box):
            assert raw[x * box + r] == g.encoder.encode(fs[r % k](x)), (x, r)


@pytest.mark.parametrize("m", [2, 3, 8, 16, 32])
def test_one_function_is_generate_lookup_table(m):
    g = _gen(m)
    f = lambda x: (x * x + 1) % m  # noqa: E731
    assert np.array_equal(g.generate_many_lookup_table([f]).poly, g.generate_lookup_table(f).poly)


def test_bad_k_or_m_raises():
    g = _gen(8)
    with pytest.raises(ValueError):
        g.generate_many_lookup_table([lambda x: x] * 3)
    with pytest.raises(ValueError):
        g.generate_many_lookup_table([])
    with pytest.raises(ValueError):
        g.generate_many_lookup_table([lambda x: x] * 16)
    with pytest.raises(ValueError):  # N / (2m) = 1 is not a multiple of 2
        _gen(512).generate_many_lookup_table([lambda x: x] * 2)
    with pytest.raises(ValueError):  # N / (2m) = 4 is not a multiple of 8
        _gen(128).generate_many_lookup_table([lambda x: x] * 8)
    with pytest.raises(ValueError):  # boxes not of equal size
        _gen(3).generate_many_lookup_table([lambda x: x] * 2)


def many_model(O, ck, prepared, tv, k, keyswitch=True):
    """The many-LUT bootstrap on the CPU oracle: every word rounded to a multiple of 2^(21+d) first, then the
    ordinary blind rotation, sample_extract_index(., j) and the key switch -> [k][count][n+1]."""
    d = k.bit_length() - 1
    w = np.asarray(prepared, np.uint64)
    wr = ((((w + (1 << (20 + d))) >> (21 + d)) << (21 + d)) & 0xFFFFFFFF).astype(np.uint32)
    tr = O.batch_blind_rotate(ck, wr, testvec=tv)
    out = []
    for j in range(k):
        if keyswitch:
            out.append(O.batch_identity_key_switching(ck, np.stack([O.sample_extract_index(t, j) for t in tr])))
        else:
            out.append(np.stack([O.sample_extract_index_2(t, j, ck.params.n) for t in tr]))
    return np.stack(out)


def test_prerounding_model_decrypts_on_oracle(O, keys_uint4):
    """64 SECURITY_UINT4 inputs, m = 8, k = 2: every output of the model decrypts to f_j(x)."""
    sk, ck = keys_uint4
    m, fs = 8, [lambda x: (x + 3) % 8, lambda x: (x * 5) % 8]
    rng = np.random.default_rng(11)
    xs = rng.integers(0, m, 64)
    cts = sk.encrypt_lwe_message(xs, m, 77)
    tv = _gen(m).generate_many_lookup_table(fs).poly
    out = many_model(O, ck, cts, tv, 2)
    for j, f in enumerate(fs):
        assert np.array_equal(sk.decrypt_lwe_message(out[j], m), np.array([f(int(x)) for x in xs])), j


def test_lut_add_u8_digits_schedule():
    """The base-4 digit adder: 4 bootstrap levels, one LUT launch per level, 4 LUT nodes, 8 output wires in the
    function-major slots of their launch; the single-LUT form has twice the LUT nodes."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd.circuit import lut_add_u8_digits

    c = R.Circuit(8)
    sums, carries = lut_add_u8_digits(c, list(range(4)), list(range(4, 8)))
    d = c.describe()
    assert len(d) == 5
    for lv in d[1:]:
        assert lv["lut_launches"] == 1 and lv["lut_nodes"] == 1 and lv["gate_launches"] == 0
    assert sum(lv["lut_nodes"] for lv in d) == 4
    outs = sums + carries
    assert len(set(outs)) == 8
    for i in range(4):
        lv = d[i + 1]
        s, cy = c.wire_slot(sums[i]), c.wire_slot(carries[i])
        assert cy == s + 1 and lv["begin"] <= s and cy < lv["end"]
        assert c.operand_slots(sums[i]) == c.operand_slots(carries[i])
    c1 = R.Circuit(8)
    lut_add_u8_digits(c1, list(range(4)), list(range(4, 8)), n_luts=1)
    d1 = c1.describe()
    assert sum(lv["lut_nodes"] for lv in d1) == 8 and sum(lv["lut_launches"] for lv in d1) == 8


def test_many_group_slots_function_major():
    """Two many-LUT nodes of one (lut, coefficients, k) share one launch; function j of node q sits at base + j*2 + q."""
    import rs_tfhe_amd as R

    c = R.Circuit(2)
    lut = c.lut(_gen(4).generate_many_lookup_table([lambda x: x] * 4).poly)
    w0 = c.pbs_many(1, 0, 0, None, 0, lut, 4)
    w1 = c.pbs_many(1, 1, 0, None, 0, lut, 4)
    d = c.describe()
    assert len(d) == 2 and d[1]["lut_launches"] == 1 and d[1]["lut_nodes"] == 2
    base = d[1]["begin"]
    for j in range(4):
        assert c.wire_slot(w0[j]) == base + 2 * j and c.wire_slot(w1[j]) == base + 2 * j + 1
    assert d[1]["end"] == base + 8 and c.slots == 2 + 8


def test_add_pbs_many_einval():
    from rs_tfhe_amd import _capi

    lib = _capi.lib()
    h = C.c_void_p()
    assert lib.tfhe_hip_circuit_create(2, C.byref(h)) == _capi.OK
    try:
        tv = np.zeros(2 * 1024, np.uint32)
        lid = C.c_uint32()
        assert lib.tfhe_hip_circuit_add_lut(h, tv.ctypes.data_as(C.c_void_p), C.byref(lid)) == _capi.OK
        ws = (C.c_uint32 * 8)()
        EINVAL = _capi.EINVAL
        for k in (0, 3, 5, 16, -1):
            assert lib.tfhe_hip_circuit_add_pbs_many(h, 1, 0, 0, 0, 0, 0, k, ws) == EINVAL
        assert lib.tfhe_hip_circuit_add_pbs_many(h, 1, 5, 0, 0, 0, 0, 2, ws) == EINVAL  # no wire 5
        assert lib.tfhe_hip_circuit_add_pbs_many(h, 1, 0, 1, 9, 0, 0, 2, ws) == EINVAL  # no wire 9 (cb != 0)
        assert lib.tfhe_hip_circuit_add_pbs_many(h, 1, 0, 0, 0, 0, 1, 2, ws) == EINVAL  # no lut 1
        assert lib.tfhe_hip_circuit_add_pbs_many(h, 1, 0, 0, 0, 0, 0, 2, None) == EINVAL
        assert lib.tfhe_hip_circuit_add_pbs_many(h, 1, 0, 0, 9, 0, 0, 2, ws) == _capi.OK  # b ignored when cb == 0
        assert list(ws[:2]) == [2, 3]
        assert lib.tfhe_hip_circuit_compile(h) == _capi.OK
        assert lib.tfhe_hip_circuit_add_pbs_many(h, 1, 0, 0, 0, 0, 0, 2, ws) == EINVAL  # compiled
    finally:
        lib.tfhe_hip_circuit_destroy(h)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_cpp_many_lut(outdir):
    """tests/cpp/test_many_lut.cpp, built as test_circuit_host.build_cpp_circuit builds the circuit program."""
    exe = os.path.join(outdir, "test_many_lut")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_many_lut.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-L" + os.path.join(ROOT, "oracle"), "-ltfhe_oracle",
        "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-fopenmp", "-pthread"])
    return exe


def test_cpp_many_lut_program_builds(O, tmp_path):
    """The C++ bindings' many-LUT program compiles and links against the header and both libraries (run on the GPU
    by tests/test_gpu_many_lut.py)."""
    assert os.path.exists(build_cpp_many_lut(str(tmp_path)))


def test_many_entry_points_exported():
    from rs_tfhe_amd import _capi

    lib = _capi.lib()
    for name in ("tfhe_hip_batch_lincomb_bootstrap_many", "tfhe_hip_batch_lincomb_bootstrap_many_dev",
                 "tfhe_hip_pool_batch_lincomb_bootstrap_many", "tfhe_hip_pool_batch_lincomb_bootstrap_many_dev",
                 "tfhe_hip_circuit_add_pbs_many"):
        assert hasattr(lib, name), name
