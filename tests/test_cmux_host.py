"""The packed CMUX on the CPU (include/tfhe_hip.h, "packed CMUX"): the numpy model of tests/cmux_model.py held to the
oracle -- its digits to oracle.decomposition and its product to oracle.external_product_exact in both digit modes, its
CMUX with the reference's digits to the f64 FFT path oracle.cmux --, its output noise to the formula the header states,
the CPU form of SecretKey.encrypt_trgsw to the model word for word, and four planted slips to the word comparison that
must catch them.  No GPU.

Every test prints its figures (`CMUX {json}` lines; run with -s) before it asserts."""
import json
import os
import re

import numpy as np
import pytest

import cmux_model as CM
import trlwe_switch_model as TM
from oracle import oracle as O
from rs_tfhe_amd import seeded as SD
from rs_tfhe_amd.params import N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = bytes((29 * i + 5) & 0xFF for i in range(32))  # a fixed generator key
ALPHA = 2.0e-8  # alpha_lv1 of SECURITY_128_BIT
ORACLE_SHAPES = ((6, 3), (7, 4), (4, 4), (1, 1))  # t <= ORC_MAX_L = 4


def _say(**kv):
    print("CMUX " + json.dumps(kv, default=float))


def _secret(seed):
    return np.random.default_rng(seed).integers(0, 2, N).astype(np.uint32)


def _words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def edge_words(basebit, t):
    """0xFFFFFFFF, 0x7FFFFFFF, 0x80000000 and, around rounding boundaries, the half step below, the boundary and its
    neighbours"""
    bt = basebit * t
    w = [0, 1, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 0x80000001]
    if bt < 32:
        half = 1 << (31 - bt)
        for q in (1, (1 << bt) // 2, (1 << bt) - 1, (1 << bt) // 2 - 1):
            base = (q << (32 - bt)) & 0xFFFFFFFF
            w += [(base - half - 1) & 0xFFFFFFFF, (base - half) & 0xFFFFFFFF, (base - 1) & 0xFFFFFFFF, base, (base + half - 1) & 0xFFFFFFFF]
    return np.array(w, np.uint32)


@pytest.fixture(scope="module")
def keys128():
    """SECURITY_128_BIT keys of the oracle with the time-domain rows of the bootstrapping key: made once, never written"""
    sk, ck = O.keygen(O.SECURITY_128_BIT, 11, with_time_domain=True)
    return sk, ck


def _oracle_offset(basebit, t, reference):
    return (O.gen_decomposition_offset(t, basebit) + CM.rounding(basebit, t, reference)) & 0xFFFFFFFF


# ---- the model against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reference", [False, True])
@pytest.mark.parametrize("basebit,t", ORACLE_SHAPES)
def test_digits_and_product_equal_the_oracle(keys128, basebit, t, reference):
    """oracle.decomposition / external_product_exact with offset = gen_decomposition_offset(t, beta) + rnd, on rows of
    the time-domain bootstrapping key and on the model's own TRGSW"""
    sk, ck = keys128
    rng = np.random.default_rng(100 * basebit + t + reference)
    x = _words(rng, (2, N))
    e = edge_words(basebit, t)
    x[:, :len(e)] = e
    off = _oracle_offset(basebit, t, reference)
    assert O.gen_decomposition_offset(t, basebit) == CM.offset(basebit, t)
    d = CM.digits(x, basebit, t, reference)  # [2][N][t]
    want_d = O.decomposition(x, t, basebit, off).view(np.int32)  # [2t][N]
    got_d = d.transpose(0, 2, 1).reshape(2 * t, N).astype(np.int32)
    assert np.array_equal(got_d, want_d)
    assert d.min() >= -(1 << (basebit - 1)) and d.max() < (1 << (basebit - 1))
    own, _, _ = CM.encrypt_trgsw(sk.key_lv1, np.eye(1, N, 0, dtype=np.int64), basebit, t, ALPHA, K)
    for name, rows in (("bsk", ck.bootstrapping_key_time.reshape(-1, 2, N)[5:5 + 2 * t]), ("own", own[0])):
        got = CM.external_product(rows, basebit, t, x[None], reference)[0]
        want = O.external_product_exact(np.ascontiguousarray(rows), x, t, basebit, off)
        slow = CM.external_product_int64(rows, basebit, t, x, reference)
        _say(case="oracle_exact", rows=name, basebit=basebit, t=t, reference=reference, equal=bool(np.array_equal(got, want)))
        assert np.array_equal(got, want), name
        assert np.array_equal(slow, want), name


@pytest.mark.parametrize("basebit,t", CM.SHAPES + ((3, 10), (7, 1)))
def test_rounding_digits_are_the_switchs(basebit, t):
    """the header calls the default digits the TRLWE key switch's: the formula without a carry chain gives the same"""
    w = np.concatenate([edge_words(basebit, t), _words(np.random.default_rng(basebit + 10 * t), 4096)])
    assert np.array_equal(CM.digits(w, basebit, t), TM.digits(w, basebit, t))
    if basebit * t < 32:
        assert not np.array_equal(CM.digits(w, basebit, t, True), CM.digits(w, basebit, t))


def test_cmux_with_reference_digits_equals_the_fft_oracle(keys128):
    """(beta, t) = (bgbit, l) = (6, 3) and TFHE_HIP_CMUX_REFERENCE_DIGITS: oracle.cmux, the reference's f64 FFT path,
    under rows of the bootstrapping key.  DESIGN section 7: at bgbit = 6 the FFT product equals the exact one, so the
    words are equal; the worst difference is recorded."""
    sk, ck = keys128
    P = O.SECURITY_128_BIT
    rng = np.random.default_rng(7)
    worst = 0
    for i in (0, 1, 350, 699):
        d0, d1 = sk_trlwe(sk, rng), sk_trlwe(sk, rng)
        got = CM.cmux(ck.bootstrapping_key_time[i], P.bgbit, P.l, d0[None], d1[None], reference=True)[0]
        want = O.cmux(d0, d1, ck.bootstrapping_key[i], P.l, P.bgbit, ck.decomposition_offset)
        worst = max(worst, int(np.abs((got - want).view(np.int32)).max()))
    _say(case="oracle_fft", worst_difference_lsb=worst)
    assert worst == 0


def sk_trlwe(sk, rng):
    """a TRLWE of a random boolean-encoded message under the oracle's ring key, noise alpha_lv1"""
    a = _words(rng, N)
    msg = np.where(rng.integers(0, 2, N) == 1, 0x20000000, 0xE0000000).astype(np.uint32)
    e = np.round(rng.normal(0.0, ALPHA, N) * 2.0 ** 32).astype(np.int64).astype(np.uint32)
    with np.errstate(over="ignore"):
        return np.stack([a, O.negacyclic_schoolbook(a, sk.key_lv1) + msg + e])


# ---- the noise ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", [0, 1])
def test_output_noise_obeys_the_formula(mu):
    """(6, 3) at alpha_lv1: the error of out against d_mu at coefficient 0 of 8 x 256 independent ciphertexts (one
    coefficient a ciphertext: under a 0/1 key those of one ciphertext are correlated), eight selectors.  Its mean
    square agrees with 2t N (B^2 / 12) alpha^2 + mu (1 + |s|_1) 2^(-2 beta t) / 12 within 5 standard errors, the
    standard error of a variance over n Gaussian samples being v sqrt(2 / n)."""
    basebit, t, sels, per = 6, 3, 8, 256
    s = _secret(40)
    rng = np.random.default_rng(41 + mu)
    m = np.zeros((sels, N), np.int64)
    m[:, 0] = mu
    rows, _, _ = CM.encrypt_trgsw(s, m, basebit, t, ALPHA, K, first_index=1000 * mu)
    errs = []
    for r in rows:
        d0, d1 = _words(rng, (per, 2, N)), _words(rng, (per, 2, N))
        out = CM.cmux(r, basebit, t, d0, d1)
        with np.errstate(over="ignore"):
            errs.append((CM.phase(out, s) - CM.phase(d1 if mu else d0, s))[:, 0].view(np.int32) / 2.0 ** 32)
    e = np.concatenate(errs)
    want = CM.cmux_variance(basebit, t, ALPHA, mu, ones=float(s.sum()))
    got, se = float((e * e).mean()), want * np.sqrt(2.0 / len(e))
    _say(case="noise", mu=mu, samples=len(e), measured=got, formula=want, standard_errors=abs(got - want) / se, mean=float(e.mean()))
    assert abs(got - want) <= 5 * se
    assert abs(e.mean()) <= 5 * np.sqrt(want / len(e))


# ---- TRGSW encryption ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basebit,t", [(6, 3), (1, 32), (7, 4)])
def test_cpu_encryption_equals_the_model_and_has_the_stated_phases(basebit, t):
    """SecretKey.encrypt_trgsw(device=None, rng_key=K) equals the model word for word (both take the f64 sampler); rows
    t + i have phase g_i mu + e and rows i phase -g_i mu (*) s + e, exactly so at alpha = 0"""
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    sk = SecretKey.new(p, 50)
    rng = np.random.default_rng(51)
    mu = np.zeros((3, N), np.int64)
    mu[0, 0] = 1
    mu[1, 5] = -1  # a monomial
    mu[2] = rng.integers(-3, 4, N)  # dense and small
    first = (1 << 32) - 4  # the row indices cross a carry of the low nonce word
    g = CM.gadget(basebit, t).astype(np.int64)
    for alpha in (0.0, ALPHA):
        got = sk.encrypt_trgsw(mu, basebit, t, alpha=alpha, rng_key=K, first_index=first)
        want, _, seed = CM.encrypt_trgsw(sk.key_lv1, mu, basebit, t, alpha, K, first)
        assert len(got) == 3 and all((s.basebit, s.t) == (basebit, t) for s in got)
        rows = np.stack([s.rows for s in got])
        assert rows.shape == (3, 2 * t, 2, N) and np.array_equal(rows, want)
        ph = CM.phase(rows, sk.key_lv1).reshape(3, 2, t, N)
        with np.errstate(over="ignore"):
            mu_s = SD.negacyclic_binary((mu & 0xFFFFFFFF).astype(np.uint32), sk.key_lv1).astype(np.int64)
            want_b = ((g[None, :, None] * mu[:, None, :]) & 0xFFFFFFFF).astype(np.uint32)
            want_a = ((-g[None, :, None] * mu_s[:, None, :]) & 0xFFFFFFFF).astype(np.uint32)
            err_a = (ph[:, 0] - want_a).view(np.int32) / 2.0 ** 32
            err_b = (ph[:, 1] - want_b).view(np.int32) / 2.0 ** 32
        _say(case="trgsw_phases", basebit=basebit, t=t, alpha=alpha, worst_a=float(np.abs(err_a).max()), worst_b=float(np.abs(err_b).max()))
        assert np.abs(err_a).max() <= 7 * alpha and np.abs(err_b).max() <= 7 * alpha
    assert seed == CM.mask_seed(K)
    one = sk.encrypt_trgsw_bool(True, basebit, t, alpha=0.0, rng_key=K, first_index=first)
    assert np.array_equal(one.rows, want_rows_of(sk, basebit, t, first))


def want_rows_of(sk, basebit, t, first):
    m = np.zeros((1, N), np.int64)
    m[0, 0] = 1
    return CM.encrypt_trgsw(sk.key_lv1, m, basebit, t, 0.0, K, first)[0][0]


def test_a_noiseless_selector_selects_exactly():
    """alpha = 0 and beta t = 32: nothing is rounded, so out has exactly the phase of d_mu, and a monomial selector
    rotates the slots"""
    basebit, t = 4, 8
    s = _secret(60)
    rng = np.random.default_rng(61)
    d0, d1 = _words(rng, (2, 2, N)), _words(rng, (2, 2, N))
    m = np.zeros((3, N), np.int64)
    m[1, 0] = 1
    m[2, 5] = 1
    rows, _, _ = CM.encrypt_trgsw(s, m, basebit, t, 0.0, K)
    assert np.array_equal(CM.phase(CM.cmux(rows[0], basebit, t, d0, d1), s), CM.phase(d0, s))
    assert np.array_equal(CM.phase(CM.cmux(rows[1], basebit, t, d0, d1), s), CM.phase(d1, s))
    ph = CM.phase(d1, s)
    with np.errstate(over="ignore"):
        rot = np.concatenate([np.uint32(0) - ph[:, N - 5:], ph[:, :N - 5]], axis=1)
    assert np.array_equal(CM.phase(CM.cmux(rows[2], basebit, t, None, d1), s), rot)


# ---- planted slips --------------------------------------------------------------------------------------------------------------
def test_planted_slips_are_caught_by_the_word_comparison():
    basebit, t = 6, 3
    s = _secret(70)
    rng = np.random.default_rng(71)
    m = np.zeros((1, N), np.int64)
    m[0, 0] = 1
    good, _, _ = CM.encrypt_trgsw(s, m, basebit, t, ALPHA, K)
    for alter in CM.ALTERS_ENCRYPT:
        bad, _, _ = CM.encrypt_trgsw(s, m, basebit, t, ALPHA, K, alter=alter)
        differ = int((bad != good).sum())
        _say(case="slip", alter=alter, words_differing=differ)
        assert differ > 0, alter
    d0, d1 = _words(rng, (2, 2, N)), _words(rng, (2, 2, N))
    want = CM.cmux(good[0], basebit, t, d0, d1)
    for alter in CM.ALTERS_CMUX:
        bad = CM.cmux(good[0], basebit, t, d0, d1, alter=alter)
        differ = int((bad != want).sum())
        _say(case="slip", alter=alter, words_differing=differ)
        assert differ > 0, alter
    # and what each slip does to the result: the swapped gadget and the reversed difference select the other input
    sw, _, _ = CM.encrypt_trgsw(s, m, basebit, t, ALPHA, K, alter="swap_ab")
    with np.errstate(over="ignore"):
        e_good = (CM.phase(want, s) - CM.phase(d1, s)).view(np.int32) / 2.0 ** 32
        e_swap = (CM.phase(CM.cmux(sw[0], basebit, t, d0, d1), s) - CM.phase(d1, s)).view(np.int32) / 2.0 ** 32
    assert np.abs(e_good).max() < 1e-3 < 0.2 < e_swap.std()


# ---- the mirrors -----------------------------------------------------------------------------------------------------------------
def test_the_constants_mirror_the_headers():
    from rs_tfhe_amd import engine as E
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd import seeded as S

    text = open(os.path.join(ROOT, "rs-tfhe_amd", "csrc", "keygen.hpp")).read()
    m = re.search(r"kStreamTrgswSeed = (\d+)u;", text)
    assert m and int(m.group(1)) == CM.SEED_STREAM == PK.TRGSW_SEED_STREAM
    for name, want, tag in (("kSeedDomainTrgswMask", CM.DOMAIN_MASK, b"EGL"), ("kSeedDomainTrgswNoise", CM.DOMAIN_NOISE, b"EGN")):
        m = re.search(name + r" = 0x([0-9A-Fa-f]+)u;", text)
        assert m and int(m.group(1), 16) == want == int.from_bytes(tag, "big"), name
    assert S.DOMAINS_TRGSW == (CM.DOMAIN_MASK, CM.DOMAIN_NOISE)
    head = open(os.path.join(ROOT, "include", "tfhe_hip.h")).read()
    m = re.search(r"enum \{ TFHE_HIP_CMUX_REFERENCE_DIGITS = (\d+) \};", head)
    assert m and int(m.group(1)) == CM.REFERENCE_DIGITS == E.CMUX_REFERENCE_DIGITS
    sw = open(os.path.join(ROOT, "rs-tfhe_amd", "csrc", "trlwe_switch.hpp")).read()
    cm = open(os.path.join(ROOT, "rs-tfhe_amd", "csrc", "cmux.hpp")).read()
    assert "constexpr size_t kCmuxChunk = kTsChunk;" in cm
    assert int(re.search(r"constexpr size_t kTsChunk = (\d+);", sw).group(1)) == CM.CHUNK == PK.CMUX_CHUNK


def test_the_selector_class_checks_its_shape():
    from rs_tfhe_amd.packing import Trgsw

    assert Trgsw(6, 3, np.zeros((6, 2, N), np.uint32)).rows.shape == (6, 2, N)
    for bad in ((0, 3), (8, 4), (6, 0), (1, 33), (4, 9), (7, 5)):
        with pytest.raises(ValueError):
            Trgsw(*bad, np.zeros((2 * max(bad[1], 1), 2, N), np.uint32))
    with pytest.raises(ValueError):
        Trgsw(6, 3, np.zeros((5, 2, N), np.uint32))


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------------
def build_cpp_cmux(outdir):
    """tests/cpp/test_cmux.cpp, built as test_trlwe_switch_host.build_cpp_trlwe_switch builds the switch's program"""
    import subprocess

    exe = os.path.join(outdir, "test_cmux")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_cmux.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-fopenmp", "-pthread"])
    return exe


def test_cpp_cmux_program_builds(tmp_path):
    """The C++ mirror's Trgsw / packing::cmux program compiles and links against the header and the library (run on the
    GPU by tests/test_gpu_cmux.py)."""
    assert os.path.exists(build_cpp_cmux(str(tmp_path)))
