"""The native circuit scheduler's host side (tfhe_hip_circuit_*): construction, levelisation, slot assignment and the
launch plan, all without a device; argument checking; the C++ binding's circuit test program builds against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _adder(bits):
    import rs_tfhe_amd as R

    c = R.Circuit(2 * bits + 1)
    s, carry = c.add(list(range(bits)), list(range(bits, 2 * bits)), 2 * bits)
    return c, s, carry


def test_add16_schedule():
    """examples/add_two_numbers.rs, 16 bits: 80 gates in 33 levels, one gate launch per level and nothing else, every
    level's outputs one contiguous slot range, every operand in an earlier level's range."""
    c, s, carry = _adder(16)
    d = c.describe()
    assert len(c.gates) == 80 and len(d) == 34
    assert d[0]["begin"] == 0 and d[0]["end"] == 33
    for lv in d[1:]:
        assert lv["gate_launches"] == 1 and lv["lincomb_launches"] == 0 and lv["nks_launches"] == 0 and lv["lut_launches"] == 0
    assert sum(lv["gate_nodes"] for lv in d) == 80 and c.slots == 33 + 80
    for prev, lv in zip(d, d[1:]):
        assert lv["begin"] == prev["end"] and lv["end"] - lv["begin"] == lv["gate_nodes"]
    for g in c.gates:
        lv = d[g.level]
        assert lv["begin"] <= c.wire_slot(g.out) < lv["end"]
        ops = c.operand_slots(g.out)
        assert len(ops) == 2 and all(o < lv["begin"] for o in ops)
        assert ops == [c.wire_slot(g.a), c.wire_slot(g.b)]


def test_mux_and_gate_level_schedule():
    """A configs[4]-shaped level, M mux + X xor over inputs: one launch without key switch (2M), one gate launch (M + X)."""
    import rs_tfhe_amd as R

    M, X = 5, 3
    c = R.Circuit(3 * M + 2 * X)
    for k in range(M):
        c.mux(3 * k, 3 * k + 1, 3 * k + 2)
    for k in range(X):
        c.xor(3 * M + 2 * k, 3 * M + 2 * k + 1)
    d = c.describe()
    assert len(d) == 2
    assert (d[1]["nks_launches"], d[1]["nks_nodes"], d[1]["gate_launches"], d[1]["gate_nodes"]) == (1, 2 * M, 1, M + X)
    assert d[1]["lincomb_launches"] == 0 and d[1]["lut_launches"] == 0
    assert d[1]["end"] - d[1]["begin"] == 3 * M + X
    assert c.operand_slots(3 * M + 2 * X) == [0, 1, 2]


def _nibble_adder():
    import rs_tfhe_amd as R

    gen = R.lut.Generator(32)
    c = R.Circuit(4)  # a_low, a_high, b_low, b_high
    mod16 = c.lut(gen.generate_lookup_table(lambda x: x % 16).poly)
    cry = c.lut(gen.generate_lookup_table(lambda x: 1 if x >= 16 else 0).poly)
    sum_low = c.pbs(1, 0, 1, 2, 0, mod16)
    carry = c.pbs(1, 0, 1, 2, 0, cry)
    high = c.lincomb([(1, 1), (1, 3)])
    sum_high = c.pbs(1, high, 1, carry, 0, mod16)
    return c, (sum_low, sum_high, carry), high


def test_nibble_adder_schedule():
    """examples/lut_add_two_numbers.rs as pbs / lincomb nodes: three blind-rotation launches, one lincomb launch (the
    three-wire high sum is materialised), the two-wire low sum folded into its bootstraps."""
    c, (sl, sh, cr), high = _nibble_adder()
    d = c.describe()
    assert len(d) == 3
    assert sum(lv["lut_launches"] + lv["gate_launches"] + lv["nks_launches"] for lv in d) == 3
    assert sum(lv["lincomb_launches"] for lv in d) == 1
    assert d[1]["lut_launches"] == 2 and d[1]["lincomb_launches"] == 0
    assert d[2]["lincomb_launches"] == 1 and d[2]["lincomb_nodes"] == 1 and d[2]["lut_launches"] == 1
    assert c.wire_slot(high) == R_NO_SLOT()
    assert c.operand_slots(sl) == [0, 2]


def R_NO_SLOT():
    from rs_tfhe_amd import _capi

    return _capi.NO_SLOT


def test_folding_rules():
    """A gate whose operand is a linear node over <= 2 wires folds it (no lincomb launch; a non-gate coefficient set is a
    launch of its own); over more wires the linear node is materialised at the consuming level."""
    import rs_tfhe_amd as R

    c = R.Circuit(3)
    na = c.not_(0)
    g1 = c.and_(na, 1)       # -a + b - 1/8 == and_ny(a, b): still the gate launch
    g2 = c.xor(na, 1)        # -a + 2b + 1/4: a folded launch of its own
    s3 = c.lincomb([(1, 0), (1, 1), (1, 2)])
    g3 = c.or_(s3, 2)        # four-term expansion: s3 materialised
    k = c.constant(False)
    g4 = c.and_(k, 0)        # one source wire: folded
    d = c.describe()
    assert len(d) == 2
    assert d[1]["gate_launches"] == 1 and d[1]["gate_nodes"] == 2  # g1 (as and_ny), g3 (over the materialised s3)
    assert d[1]["lincomb_launches"] == 1 and d[1]["lincomb_nodes"] == 1
    assert d[1]["lut_launches"] == 2 and d[1]["lut_nodes"] == 2  # g2 and g4: folded, coefficients of no gate code
    assert c.operand_slots(g1) == [0, 1]
    assert c.wire_slot(na) == R_NO_SLOT() and c.wire_slot(k) == R_NO_SLOT()
    ops3 = c.operand_slots(g3)
    assert ops3[0] >= d[1]["begin"] and ops3[1] == 2
    for w in (g1, g2, g3, g4):
        assert d[1]["begin"] <= c.wire_slot(w) < d[1]["end"]


def _lib():
    from rs_tfhe_amd import _capi

    return _capi.lib(), _capi


def test_invalid_arguments():
    lib, capi = _lib()
    h = C.c_void_p()
    assert lib.tfhe_hip_circuit_create(0, C.byref(h)) == capi.EINVAL
    assert lib.tfhe_hip_circuit_create(2, None) == capi.EINVAL
    assert lib.tfhe_hip_circuit_create(2, C.byref(h)) == capi.OK
    w = C.c_uint32()
    try:
        assert lib.tfhe_hip_circuit_add_gate(h, 11, 0, 1, C.byref(w)) == capi.EINVAL  # above COPY
        assert lib.tfhe_hip_circuit_add_gate(h, -1, 0, 1, C.byref(w)) == capi.EINVAL
        assert lib.tfhe_hip_circuit_add_gate(h, 0, 0, 2, C.byref(w)) == capi.EINVAL   # wire 2 does not exist yet
        assert lib.tfhe_hip_circuit_add_mux(h, 0, 1, 7, C.byref(w)) == capi.EINVAL
        assert lib.tfhe_hip_circuit_add_not(h, 9, C.byref(w)) == capi.EINVAL
        bad = np.array([5], np.uint32)
        one = np.array([1], np.uint32)
        assert lib.tfhe_hip_circuit_add_lincomb(h, one.ctypes.data_as(C.c_void_p), bad.ctypes.data_as(C.c_void_p), 1, 0,
                                                C.byref(w)) == capi.EINVAL
        assert lib.tfhe_hip_circuit_add_pbs(h, 1, 0, 1, 1, 0, 0, C.byref(w)) == capi.EINVAL  # no lut 0
        tv = np.zeros(2 * 1024, np.uint32)
        lid = C.c_uint32()
        assert lib.tfhe_hip_circuit_add_lut(h, tv.ctypes.data_as(C.c_void_p), C.byref(lid)) == capi.OK
        assert lib.tfhe_hip_circuit_add_pbs(h, 1, 0, 1, 1, 0, lid.value + 1, C.byref(w)) == capi.EINVAL
        assert lib.tfhe_hip_circuit_add_pbs(h, 1, 0, 1, 1, 0, lid.value, C.byref(w)) == capi.OK
        assert lib.tfhe_hip_circuit_add_gate(h, 10, w.value, w.value, C.byref(w)) == capi.OK  # COPY is the last code
        assert lib.tfhe_hip_circuit_compile(h) == capi.OK
        assert lib.tfhe_hip_circuit_add_gate(h, 0, 0, 1, C.byref(w)) == capi.EINVAL  # after compile
        assert lib.tfhe_hip_circuit_add_lut(h, tv.ctypes.data_as(C.c_void_p), C.byref(lid)) == capi.EINVAL
        slot = C.c_uint32()
        assert lib.tfhe_hip_circuit_wire_slot(h, 99, C.byref(slot)) == capi.EINVAL
        # NULL handles
        assert lib.tfhe_hip_circuit_compile(None) == capi.EINVAL
        assert lib.tfhe_hip_circuit_add_gate(None, 0, 0, 1, C.byref(w)) == capi.EINVAL
        assert lib.tfhe_hip_circuit_run(None, h, None, 1, None, 0, None) == capi.EINVAL
        assert lib.tfhe_hip_circuit_run_pool(None, h, None, 1, None, 0, None) == capi.EINVAL
        assert lib.tfhe_hip_circuit_run_pool_dev(None, 0, h, None, None, 1, None) == capi.EINVAL
    finally:
        lib.tfhe_hip_circuit_destroy(h)


def test_python_api_kept_and_extended():
    import rs_tfhe_amd as R

    c = R.Circuit(3)
    for name in ("gate", "nand", "and_", "or_", "xor", "xnor", "nor", "and_ny", "and_yn", "or_ny", "or_yn", "mux_naive",
                 "full_adder", "add", "levels", "run", "run_dev", "run_reference", "_run_dev_torch", "mux", "pbs", "lut",
                 "lincomb", "not_", "constant"):
        assert callable(getattr(c, name)), name
    m = c.mux(0, 1, 2)
    assert c.n_wires == 4 and c.describe()[1]["nks_nodes"] == 2
    with pytest.raises(ValueError):
        c.xor(0, 17)
    # run_reference evaluates linear nodes in numpy with wrapping arithmetic
    k = c.lincomb([(3, 0), (0xFFFFFFFF, 1)], 5)
    inputs = np.array([[[1, 2]], [[4, 0xFFFFFFFF]], [[0, 0]]], np.uint32)
    ref = c.run_reference(None, inputs, mux_fn=lambda a, b, cc: a)
    assert ref[k].tolist() == [[(3 * 1 - 4) & 0xFFFFFFFF, (3 * 2 - 0xFFFFFFFF + 5) & 0xFFFFFFFF]]
    assert m == 3


def test_cpp_circuit_program_builds(tmp_path):
    """tests/cpp/test_circuit.cpp against include/rs_tfhe_hip.hpp / tfhe_hip.h (the test_mirror rule's flags)."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    if not os.path.exists(os.path.join(ROOT, "oracle", "libtfhe_oracle.so")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "libtfhe_oracle.so"])
    exe = build_cpp_circuit(str(tmp_path))
    assert os.path.exists(exe)


def build_cpp_circuit(outdir):
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(outdir, "test_circuit")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(cpp, "test_circuit.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-L" + os.path.join(ROOT, "oracle"), "-ltfhe_oracle",
        "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-fopenmp", "-pthread"])
    return exe
