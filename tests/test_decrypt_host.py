"""Decryption on the GPU (include/tfhe_hip.h, "decryption"), the parts a CPU can check: the header and the library's
exports, the MESSAGE / BOOL decode of csrc/decrypt_decode.hpp compiled for the host against rs-tfhe_amd/client.py's
expressions at every decode boundary, that program once under AddressSanitizer + UBSan, the new numpy path of
SecretKey.phase_lv1, the C++ mirror program's build, and the `device=None` paths of the six SecretKey methods against
their expressions restated here.

The planted phases and the numpy decodes are shared with tests/test_gpu_decrypt.py (boundary_phases, numpy_message)."""
import os
import re
import subprocess

import numpy as np
import pytest

from rs_tfhe_amd import params as P
from rs_tfhe_amd.client import SecretKey, torus_to_f64
from rs_tfhe_amd.params import N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("tfhe_hip_batch_decrypt", "tfhe_hip_batch_decrypt_dev", "tfhe_hip_batch_decrypt_trlwe",
             "tfhe_hip_batch_decrypt_trlwe_dev")
MODULI = (2, 3, 4, 5, 10, 16, 255, 65536)
PHASE, BOOL, MESSAGE = 0, 1, 2


def threshold_phases(m: int, ks) -> list:
    """round((2k + 1) 2^32 / (4m)) + {-1, 0, +1}: where the decode steps from message k to k + 1 (the value before the
    truncation crosses an integer there)"""
    return [(((2 * k + 1) << 32) + 2 * m) // (4 * m) + d for k in ks for d in (-1, 0, 1)]


def boundary_phases(m: int) -> np.ndarray:
    """round(k 2^32 / (2m)) + {-1, 0, +1} (the encodings of the messages) for every k <= 2m when m <= 16 and for 64
    spread k otherwise, the decode's steps between them (threshold_phases) for the same k, plus 0, 2^31 - 1, 2^31 and
    2^32 - 1; u32 (values at or past 2^32 wrap)."""
    ks = range(2 * m + 1) if m <= 16 else sorted({(j * 2 * m) // 63 for j in range(64)})
    vals = [((k << 32) + m) // (2 * m) + d for k in ks for d in (-1, 0, 1)]  # round-half-up of k 2^32 / (2m), exactly
    vals += threshold_phases(m, ks)
    vals += [0, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
    return np.array([v % (1 << 32) for v in vals], np.uint64).astype(np.uint32)


def numpy_message(phase: np.ndarray, m: int) -> np.ndarray:
    """SecretKey.decrypt_lwe_message's expression on given phases (client.py:  the definition)"""
    scale = 1.0 / (2.0 * m)
    return (torus_to_f64(phase) / scale + 0.5).astype(np.int64) % m


def test_header_declares_decryption():
    hdr = open(os.path.join(ROOT, "include", "tfhe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for fn in FUNCTIONS:
        assert re.search(r"\bint\s+" + fn + r"\s*\(", code), fn
    assert re.search(r"enum\s*\{\s*TFHE_HIP_DECRYPT_PHASE\s*=\s*0\s*,\s*TFHE_HIP_DECRYPT_BOOL\s*=\s*1\s*,\s*"
                     r"TFHE_HIP_DECRYPT_MESSAGE\s*=\s*2\s*\}", code)
    assert "/* ---- decryption" in hdr
    from rs_tfhe_amd import _capi

    assert _capi.DECRYPT_MODES == {"phase": PHASE, "bool": BOOL, "message": MESSAGE}
    for fn in FUNCTIONS:
        assert fn in _capi.SIGNATURES


def test_library_exports_decryption():
    so = os.path.join(ROOT, "rs-tfhe_amd", "libtfhe_hip.so")
    assert os.path.exists(so), "build first: python __graft_entry__.py"
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert not [fn for fn in FUNCTIONS if fn not in exported]


def build_decode_program(outdir, sanitize=False):
    """tests/cpp/test_decrypt_decode.cpp: host code only, the flags that matter for the decode as the library has them
    (-ffp-contract=fast, no fast-math)"""
    exe = os.path.join(outdir, "test_decrypt_decode" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O3"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-ffp-contract=fast"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "test_decrypt_decode.cpp")])
    return exe


def _planted():
    """(mode, modulus, phase) lines and the words client.py's expressions give them"""
    lines, want = [], []
    for m in MODULI:
        ph = boundary_phases(m)
        lines += [(MESSAGE, m, int(v)) for v in ph]
        want += [int(v) for v in numpy_message(ph, m)]
        if m == 2:
            lines += [(BOOL, 0, int(v)) for v in ph] + [(PHASE, 0, int(v)) for v in ph]
            want += [int(v) for v in (ph.view(np.int32) >= 0)] + [int(v) for v in ph]
    return lines, want


def _run_decode(exe):
    lines, want = _planted()
    text = "".join(f"{a} {b} {c}\n" for a, b, c in lines)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = [int(v) for v in r.stdout.split()]
    return lines, want, got, r.stderr


def test_decode_equals_client_expressions(tmp_path):
    lines, want, got, _ = _run_decode(build_decode_program(str(tmp_path)))
    assert len(lines) == sum(len(boundary_phases(m)) for m in MODULI) + 2 * len(boundary_phases(2)) == len(got) == len(want)
    bad = [(ln, w, g) for ln, w, g in zip(lines, want, got) if w != g]
    assert not bad, bad[:10]
    # the plant reaches what it is for: every message value of every modulus up to 16, and both sides of a boundary
    for m in (2, 3, 4, 5, 10, 16):
        ph = boundary_phases(m)
        dec = numpy_message(ph, m)
        assert set(dec.tolist()) == set(range(m))
        th = numpy_message(np.array(threshold_phases(m, range(2 * m - 1)), np.uint64).astype(np.uint32), m).reshape(-1, 3)
        assert (th[:, 0] != th[:, 2]).all(), "a step of the decode lies inside every planted triple"


def test_decode_program_under_sanitizers(tmp_path):
    """the same program with AddressSanitizer and UBSan (host code, its own main, no preload), once"""
    lines, want, got, err = _run_decode(build_decode_program(str(tmp_path), sanitize=True))
    assert got == want
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-4000:]


def test_phase_lv1_numpy_path():
    sk = SecretKey.new(P.SECURITY_128_BIT, 31)
    rows = np.random.default_rng(32).integers(0, 1 << 32, (37, N + 1), dtype=np.uint64).astype(np.uint32)
    want = np.empty(37, np.uint32)
    for r in range(37):  # b - a . s, one row at a time in Python integers
        want[r] = (int(rows[r, N]) - sum(int(a) for a, s in zip(rows[r, :N], sk.key_lv1) if s)) % (1 << 32)
    got = sk.phase_lv1(rows)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert np.array_equal(sk.phase_lv1(rows.reshape(-1)), want)


def build_cpp_decrypt(outdir):
    """tests/cpp/test_decrypt.cpp, built as test_sym_encrypt_host.build_cpp_sym_encrypt builds its program."""
    exe = os.path.join(outdir, "test_decrypt")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_decrypt.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-fopenmp", "-pthread"])
    return exe


def test_cpp_decrypt_program_builds(tmp_path):
    """the C++ mirror's decrypt_batch / phase_batch / packed pair compile and link against the library"""
    assert os.path.exists(build_cpp_decrypt(str(tmp_path)))


@pytest.mark.parametrize("pname", ["SECURITY_128_BIT", "SECURITY_UINT7"])
def test_device_none_paths_are_the_numpy_expressions(pname):
    """Without device= the six methods return what their numpy expressions, restated here, return: same words, same
    dtypes (bool for booleans, int64 for messages, uint32 for phases)."""
    from rs_tfhe_amd.seeded import negacyclic_binary

    p = P.PARAM_SETS[pname]
    sk = SecretKey.new(p, 77)
    bits = np.random.default_rng(5).integers(0, 2, 64).astype(bool)
    cts = sk.encrypt_bool(bits, seed=6)
    inner = (cts[:, :-1] * sk.key_lv0[None, :]).sum(axis=1, dtype=np.uint32)
    phase = cts[:, -1] - inner
    got = sk.phase(cts)
    assert got.dtype == np.uint32 and np.array_equal(got, phase)
    got = sk.decrypt_bool(cts)
    assert got.dtype == np.bool_ and np.array_equal(got, phase.view(np.int32) >= 0) and np.array_equal(got, bits)
    for m in (2, 3, 10, 16):
        msgs = np.arange(64) % m
        c = sk.encrypt_lwe_message(msgs, m, seed=7)
        ph = c[:, -1] - (c[:, :-1] * sk.key_lv0[None, :]).sum(axis=1, dtype=np.uint32)
        got = sk.decrypt_lwe_message(c, m)
        assert got.dtype == np.int64 and np.array_equal(got, numpy_message(ph, m)) and np.array_equal(got, msgs)
    count = N + 3
    pbits = np.random.default_rng(8).integers(0, 2, count).astype(bool)
    packed = sk.encrypt_packed_bool(pbits, seed=9)
    pphase = (packed[:, 1] - negacyclic_binary(packed[:, 0], sk.key_lv1)).reshape(-1)[:count]
    got = sk.packed_phase(packed, count)
    assert got.dtype == np.uint32 and np.array_equal(got, pphase)
    got = sk.decrypt_packed_bool(packed, count)
    assert got.dtype == np.bool_ and np.array_equal(got, pphase.view(np.int32) >= 0) and np.array_equal(got, pbits)
    pm = sk.encrypt_packed_lwe_message(np.arange(count) % 10, 10, seed=10)
    pph = (pm[:, 1] - negacyclic_binary(pm[:, 0], sk.key_lv1)).reshape(-1)[:count]
    got = sk.decrypt_packed_lwe_message(pm, count, 10)
    assert got.dtype == np.int64 and np.array_equal(got, numpy_message(pph, 10)) and np.array_equal(got, np.arange(count) % 10)
    with pytest.raises(ValueError):
        sk.packed_phase(packed, 2 * N + 1)
