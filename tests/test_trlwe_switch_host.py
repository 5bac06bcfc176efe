"""The TRLWE key switch on the CPU (include/tfhe_hip.h, "TRLWE key switch"): the numpy model of
tests/trlwe_switch_model.py held to the section's identities -- the digits recompose, the automorphisms compose, the
phase of a switched ciphertext is psi_k of the input's, its error obeys the two-term variance the header states, the
partial trace is exact on a noiseless key -- and the Python mirror of kTsChunk to the header it mirrors.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import trlwe_switch_model as TM
from rs_tfhe_amd.params import N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = bytes((53 * i + 7) & 0xFF for i in range(32))  # a fixed generator key
ALPHA = 2.0e-8  # alpha_lv1 of the 128-bit and 80-bit sets


def _say(**kv):
    print("TRLWESWITCH " + json.dumps(kv, default=float))


def _secret(seed):
    return np.random.default_rng(seed).integers(0, 2, N).astype(np.uint32)


def _edge_words(basebit, t):
    """0xFFFFFFFF and 0x7FFFFFFF (the rounding carry runs to the top and is dropped), and around every rounding boundary
    the half step below it, the boundary and the word above"""
    bt = basebit * t
    w = [0, 1, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 0x80000001]
    if bt < 32:
        half = 1 << (31 - bt)
        for q in (1, 2, (1 << bt) // 2, (1 << bt) - 1, (1 << bt) // 2 - 1):
            base = (q << (32 - bt)) & 0xFFFFFFFF
            w += [(base - half - 1) & 0xFFFFFFFF, (base - half) & 0xFFFFFFFF, (base - 1) & 0xFFFFFFFF, base, (base + half - 1) & 0xFFFFFFFF]
    return np.array(w, np.uint32)


# ---- model identities ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basebit,t", TM.SHAPES + ((3, 10), (5, 6), (7, 1), (1, 1)))
def test_digits_recompose_to_the_rounded_word(basebit, t):
    """sum_l d_l g_l = a_bar 2^(32 - beta t) mod 2^32, d_l in [-B/2, B/2), on random words and the edge words"""
    rng = np.random.default_rng(basebit * 100 + t)
    w = np.concatenate([_edge_words(basebit, t), rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32)])
    d = TM.digits(w, basebit, t).astype(np.int64)
    B = 1 << basebit
    assert d.min() >= -B // 2 and d.max() < B // 2
    g = TM.gadget(basebit, t).astype(np.int64)
    got = (d * g[None, :]).sum(axis=1) & 0xFFFFFFFF
    want = (TM.a_bar(w, basebit, t).astype(np.int64) << (32 - basebit * t)) & 0xFFFFFFFF
    assert np.array_equal(got, want)
    if basebit * t == 32:
        assert np.array_equal(want.astype(np.uint32), w)  # nothing is rounded


def test_automorphisms_compose():
    """psi_k psi_k' = psi_(k k' mod 2N), psi_1 the identity, psi_(2N-1) the reversal with the stated signs"""
    rng = np.random.default_rng(3)
    p = rng.integers(0, 1 << 32, (3, N), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(TM.psi(p, 1), p)
    for k in TM.KS + (5, 1023, 1027):
        for k2 in TM.KS + (7, 2045):
            assert np.array_equal(TM.psi(TM.psi(p, k2), k), TM.psi(p, (k * k2) % (2 * N))), (k, k2)
    rev = TM.psi(p, 2 * N - 1)
    assert np.array_equal(rev[:, 0], p[:, 0])
    assert np.array_equal(rev[:, 1:], (np.uint32(0) - p[:, 1:])[:, ::-1])  # X^j -> X^(-j) = -X^(N - j)
    alt = TM.psi(p, N + 1)  # X -> -X
    assert np.array_equal(alt[:, ::2], p[:, ::2]) and np.array_equal(alt[:, 1::2], np.uint32(0) - p[:, 1::2])


def test_the_fast_products_equal_the_int64_sums():
    """Switcher's float64 matmuls over 16-bit halves against switch_int64, term by term, on one ciphertext with the
    edge words planted; (7, 4) and an all -B/2 digit row reach the largest sums"""
    rng = np.random.default_rng(5)
    for (basebit, t), k in (((4, 6), 3), ((7, 4), 2047)):
        rows = rng.integers(0, 1 << 32, (t, 2, N), dtype=np.uint64).astype(np.uint32)
        rows[:, :, :4] = (0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0)
        ct = rng.integers(0, 1 << 32, (2, N), dtype=np.uint64).astype(np.uint32)
        e = _edge_words(basebit, t)
        ct[0, :len(e)] = e
        ct[0, 512:] = 0x80000000  # every digit of the top position -B/2
        assert np.array_equal(TM.switch(rows, k, basebit, t, ct[None])[0], TM.switch_int64(rows, k, basebit, t, ct))


# ---- phase and noise ---------------------------------------------------------------------------------------------------
def _errors(k, basebit, t, alpha, distinct, cts=2, seed=0):
    """phase(switch(ct)) - psi_k(phase(ct)) as float torus fractions [cts][N], and the ones of the source key"""
    s_from = _secret(100 + seed)
    s_to = _secret(200 + seed) if distinct else s_from
    key = TM.make_key(s_from, s_to, k, basebit, t, K, alpha)
    rng = np.random.default_rng(1000 * k + seed)
    ct = rng.integers(0, 1 << 32, (cts, 2, N), dtype=np.uint64).astype(np.uint32)
    out = TM.switch(TM.key_rows(key.mask_seed, k, t, key.bodies), k, basebit, t, ct)
    with np.errstate(over="ignore"):
        err = TM.phase(out, s_to) - TM.psi(TM.phase(ct, s_from), k)
    return err.view(np.int32) / 2.0 ** 32, int(s_from.sum())


@pytest.mark.parametrize("basebit,t,alpha", [(4, 6, ALPHA), (4, 6, 0.0), (7, 3, ALPHA)])
def test_phase_is_psi_k_of_the_input_phase_within_the_stated_noise(basebit, t, alpha):
    """For k in {1, 3, 513, 1025, 2047} (two different keys at k = 1, one key otherwise) every coefficient of the output's
    phase equals psi_k of the input's within 8 standard deviations of the header's two-term variance
    (N/2) 2^(-2 beta t) / 12 + N t (B^2 / 12) alpha^2: the error is a sum of >= 512 independent bounded terms, Gaussian
    to the accuracy that matters, P(|z| > 8) = 1.2e-15 a sample, 1e-11 over the 10,240 samples here.
    Where the key noise is the larger term (alpha = 2e-8: by 350x at (4, 6), 170x at (7, 3)) the formula is held to the
    sample variance by DESIGN 11.3's rule for a standard deviation: |std / formula - 1| <= 5 SE, SE = 1 / sqrt(2 M) =
    0.70 % at M = 10,240.  The samples count as independent there: the terms digit x noise have zero-mean digits, so two
    coefficients of one ciphertext are uncorrelated.  What the formula leaves out is well inside the bound: the digits'
    variance is (B^2 - 1) / 12 (-0.2 % of the std at B = 16) and f64_to_torus truncates toward zero (-0.6 % at
    alpha = 2e-8).  The rounding term has its own test below: under a 0 / 1 key its coefficients are correlated."""
    errs = [_errors(k, basebit, t, alpha, distinct=(k == 1))[0].reshape(-1) for k in TM.KS]
    err = np.concatenate(errs)
    M = len(err)
    sigma = np.sqrt(TM.switch_variance(basebit, t, alpha))
    ratio = float(err.std() / sigma)
    _say(case="noise", basebit=basebit, t=t, alpha=alpha, M=M, sigma=sigma, sample_std=float(err.std()), ratio=ratio,
         worst_in_sigma=float(np.abs(err).max() / sigma), se=1 / np.sqrt(2 * M))
    assert M == 10240
    assert np.abs(err).max() <= 8 * sigma
    if alpha > 0:
        assert TM.key_noise_variance(basebit, t, alpha) > 100 * TM.rounding_variance(basebit, t)
        assert abs(ratio - 1) <= 5 / np.sqrt(2 * M)
        assert abs(err.mean()) <= 5 * sigma / np.sqrt(M)


def test_the_rounding_term_of_the_variance():
    """alpha = 0 leaves the rounding error (a' - a'_rounded) (*) psi_k(s_from) alone: `ones` terms uniform over one step
    2^(-beta t), variance ones 2^(-2 beta t) / 12 a coefficient.  A 0 / 1 key is not zero-mean, so the coefficients of
    ONE ciphertext share a common component (the mean over a ciphertext's coefficients is 0.4 of their std) and are not
    independent samples.  Coefficient 0 of 2,048 independent ciphertexts per k is: M = 10,240 over the five k, the same
    5 SE rule, with the key's own count of ones in the formula (the header's N/2 is its expectation).  (beta, t) = (4, 2)
    keeps the products small; the step is then 2^-8 and 8 sigma = 0.21 of the torus: no wrap."""
    basebit, t = 4, 2
    err = []
    for k in TM.KS:
        e, ones = _errors(k, basebit, t, 0.0, distinct=(k == 1), cts=2048)
        err.append(e[:, 0])
    err = np.concatenate(err)
    M = len(err)
    sigma = np.sqrt(TM.rounding_variance(basebit, t, ones))
    ratio = float(err.std() / sigma)
    _say(case="rounding", basebit=basebit, t=t, M=M, ones=ones, sigma=sigma, sample_std=float(err.std()), ratio=ratio)
    assert M == 10240 and np.abs(err).max() <= 8 * sigma < 0.25
    assert abs(ratio - 1) <= 5 / np.sqrt(2 * M)
    assert abs(TM.rounding_variance(basebit, t) / TM.rounding_variance(basebit, t, ones) - 1) < 0.1  # N/2 is the expectation


def test_a_wrong_key_does_not_decrypt():
    """the checker's own check: under another target key the error is uniform on the torus"""
    e = _errors(3, 4, 6, ALPHA, distinct=False)[0]
    s_from = _secret(100)
    key = TM.make_key(s_from, s_from, 3, 4, 6, K, ALPHA)
    ct = np.random.default_rng(9).integers(0, 1 << 32, (1, 2, N), dtype=np.uint64).astype(np.uint32)
    out = TM.switch(TM.key_rows(key.mask_seed, 3, 6, key.bodies), 3, 4, 6, ct)
    with np.errstate(over="ignore"):
        bad = (TM.phase(out, _secret(300)) - TM.psi(TM.phase(ct, s_from), 3)).view(np.int32) / 2.0 ** 32
    assert np.abs(e).max() < 1e-4 < 0.2 < bad.std()


def test_one_generator_key_shares_no_noise_between_ks():
    """nonce row 64 k + l: the noise rows of different k under one K are all different, and the seed does not depend on k"""
    rows = np.concatenate([TM.key_noise(K, k, 6, ALPHA).words for k in TM.KS])
    assert len(np.unique(rows, axis=0)) == len(rows)
    masks = np.concatenate([TM.key_masks(TM.mask_seed(K), k, 6) for k in TM.KS])
    assert len(np.unique(masks, axis=0)) == len(masks)
    assert TM.nonce_rows(3, 64)[-1] < TM.nonce_rows(5, 64)[0]  # l < 64 never reaches the next odd k's rows


# ---- the trace ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [3, 10])
def test_trace_identity_on_a_noiseless_key(steps):
    """alpha = 0 and (beta, t) = (4, 8): beta t = 32 rounds nothing, so every switch is exact and after `steps` steps the
    phase holds 2^steps times the input's at the multiples of 2^steps and exactly zero elsewhere."""
    basebit, t = 4, 8
    s = _secret(7)
    seed = TM.mask_seed(K)
    rng = np.random.default_rng(70 + steps)
    ct = rng.integers(0, 1 << 32, (2, 2, N), dtype=np.uint64).astype(np.uint32)
    cur = ct.copy()
    with np.errstate(over="ignore"):
        for k in TM.trace_keys(steps):
            bodies = TM.bodies_from(seed, s, s, k, basebit, t, np.zeros((t, N), np.uint32))
            sw = TM.Switcher(TM.key_rows(seed, k, t, bodies), k, basebit, t)
            cur = TM.trace([sw], cur)
        want = np.zeros((2, N), np.uint32)
        keep = np.arange(0, N, 1 << steps)
        want[:, keep] = TM.phase(ct, s)[:, keep] * np.uint32(1 << steps)
    assert np.array_equal(TM.phase(cur, s), want)
    from rs_tfhe_amd import packing as PK

    assert PK.trace_ks(steps) == TM.trace_keys(steps) and PK.trace_ks(10)[-1] == 3


# ---- the mirrors ---------------------------------------------------------------------------------------------------------
def test_the_chunk_constant_mirrors_the_header():
    from rs_tfhe_amd import packing as PK

    text = open(os.path.join(ROOT, "rs-tfhe_amd", "csrc", "trlwe_switch.hpp")).read()
    m = re.search(r"constexpr size_t kTsChunk = (\d+);", text)
    assert m and int(m.group(1)) == PK.TRLWE_SWITCH_CHUNK
    state = open(os.path.join(ROOT, "rs-tfhe_amd", "csrc", "internal.hpp")).read()  # KeyState
    m = re.search(r"kMaxTrlweSwitchKeys = (\d+);", state)
    assert m and int(m.group(1)) == PK.TRLWE_SWITCH_MAX_KEYS


def test_the_stream_table_rows_are_the_models():
    """keygen.hpp's three new rows and the domain word are what the model draws from"""
    text = open(os.path.join(ROOT, "rs-tfhe_amd", "csrc", "keygen.hpp")).read()
    for name, want in (("kStreamTksMask", TM.MASK_STREAM), ("kStreamTksNoise", TM.NOISE_STREAM), ("kStreamTksSeed", TM.SEED_STREAM)):
        m = re.search(name + r" = (\d+)u;", text)
        assert m and int(m.group(1)) == want, name
    m = re.search(r"kSeedDomainTks = 0x([0-9A-Fa-f]+)u;", text)
    assert m and int(m.group(1), 16) == TM.DOMAIN == int.from_bytes(b"TKS", "big")


def test_the_key_class_checks_its_shape():
    from rs_tfhe_amd.packing import TrlweSwitchKey

    ok = TrlweSwitchKey(3, 4, 6, bytes(32), np.zeros((6, N), np.uint32))
    assert ok.nbytes == 6 * N * 4 + 32
    for bad in ((2, 4, 6), (2049, 4, 6), (0, 4, 6), (3, 8, 4), (3, 0, 4), (3, 4, 9), (3, 1, 33), (3, 4, 0)):
        with pytest.raises(ValueError):
            TrlweSwitchKey(*bad, bytes(32), np.zeros((max(bad[2], 1), N), np.uint32))
    with pytest.raises(ValueError):
        TrlweSwitchKey(3, 4, 6, bytes(31), np.zeros((6, N), np.uint32))
    with pytest.raises(ValueError):
        TrlweSwitchKey(3, 4, 6, bytes(32), np.zeros((5, N), np.uint32))


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------
def build_cpp_trlwe_switch(outdir):
    """tests/cpp/test_trlwe_switch.cpp, built as test_polymul_host.build_cpp_polymul builds the product's program"""
    import subprocess

    exe = os.path.join(outdir, "test_trlwe_switch")
    subprocess.check_call([
        "g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
        os.path.join(ROOT, "tests", "cpp", "test_trlwe_switch.cpp"),
        "-L" + os.path.join(ROOT, "rs-tfhe_amd"), "-ltfhe_hip", "-Wl,-rpath," + os.path.join(ROOT, "rs-tfhe_amd"),
        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-fopenmp", "-pthread"])
    return exe


def test_cpp_trlwe_switch_program_builds(tmp_path):
    """The C++ mirror's TrlweSwitchKey program compiles and links against the header and the library (run on the GPU by
    tests/test_gpu_trlwe_switch.py)."""
    assert os.path.exists(build_cpp_trlwe_switch(str(tmp_path)))
