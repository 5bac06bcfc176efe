"""The packed CMUX on the GPU (csrc/cmux.hpp behind tfhe_hip_batch_trlwe_cmux and tfhe_hip_batch_encrypt_trgsw) held to the
numpy model of tests/cmux_model.py: the CMUX and the external product word for word (np.array_equal, no tolerance) in
both digit modes over the decompositions and batch sizes at which the kernels take another path, the host and _dev
forms, generated selectors under DESIGN 11.2's borderline rule, selection, lookup and slot rotation end to end, the
error codes, and the C++ mirror.

Every test prints its figures (`CMUX {json}` lines; run with -s) before it asserts."""
import json
import subprocess

import numpy as np
import pytest

import cmux_model as CM
import keygen_model as KM
from rs_tfhe_amd.params import N
from test_cmux_host import edge_words

pytestmark = pytest.mark.gpu

K = bytes((43 * i + 17) & 0xFF for i in range(32))  # a fixed generator key
ALPHA = 2.0e-8
COUNTS = (1, 3, 63, 64, 65)  # one row, a few, the 64-row tile less one, full, and one into the next


def _say(**kv):
    print("CMUX " + json.dumps(kv, default=float))


def _secret(seed):
    return np.random.default_rng(seed).integers(0, 2, N).astype(np.uint32)


def _words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def _inputs(seed, count, basebit, t):
    """(d0, d1) [count][2][N] random words; in the first and last ciphertext the edge words are planted as the
    DIFFERENCE at both ends of both rows -- against d0 = 0, against a d0 that makes the subtraction wrap, and as d1
    itself"""
    rng = np.random.default_rng(seed)
    d0, d1 = _words(rng, (count, 2, N)), _words(rng, (count, 2, N))
    e = edge_words(basebit, t)
    n = len(e)
    with np.errstate(over="ignore"):
        for c in (0, count - 1):
            d0[c, :, :n] = 0
            d1[c, :, :n] = e  # x = e
            d0[c, :, n:2 * n] = np.uint32(0xFFFFFFFF)
            d1[c, :, n:2 * n] = e + np.uint32(0xFFFFFFFF)  # x = e through a wrapping difference
            d1[c, :, -n:] = e
            d0[c, :, -n:] = e[::-1]  # pairs of edge words
    return d0, d1


def _selector_rows(seed, t):
    """random rows (the product is defined for any) with the plane-byte extremes planted"""
    rows = _words(np.random.default_rng(seed), (2 * t, 2, N))
    rows[:, :, :4] = (0xFFFFFFFF, 0x80000000, 0x7F7F7F80, 0)
    return rows


@pytest.fixture(scope="module")
def engine():
    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    e = R.Engine(p, 0)  # no cloud key: the CMUX needs none
    yield e
    e.close()


# ---- words -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reference", [False, True])
@pytest.mark.parametrize("basebit,t", CM.SHAPES)
def test_cmux_equals_the_model(engine, basebit, t, reference):
    """every count of COUNTS on prefixes of one batch of 65 (the model runs once); (1, 32) fills all 64 columns"""
    rows = _selector_rows(200 + basebit, t)
    d0, d1 = _inputs(300 + 10 * basebit + reference, max(COUNTS), basebit, t)
    want = CM.cmux(rows, basebit, t, d0, d1, reference)
    for count in COUNTS:  # (the edge words sit in ciphertext 0, which every prefix holds, and in the last of the 65)
        got = engine.batch_trlwe_cmux(rows, basebit, t, d0[:count], d1[:count], reference_digits=reference)
        equal = bool(np.array_equal(got, want[:count]))
        _say(case="words", basebit=basebit, t=t, reference=reference, count=count, equal=equal)
        assert got.shape == (count, 2, N) and got.dtype == np.uint32
        assert equal, count
    if basebit * t < 32:  # the two modes give different words: neither comparison passes on the other's code
        assert not np.array_equal(want[:1], CM.cmux(rows, basebit, t, d0[:1], d1[:1], not reference))


def test_a_batch_that_crosses_a_chunk(engine):
    """kCmuxChunk + 1 ciphertexts at (7, 1): the last one takes a second pass through the digit scratch"""
    basebit, t = 7, 1
    rows = _selector_rows(5, t)
    d0, d1 = _inputs(77, CM.CHUNK + 1, basebit, t)
    want = CM.cmux(rows, basebit, t, d0, d1)
    got = engine.batch_trlwe_cmux(rows, basebit, t, d0, d1)
    assert np.array_equal(got[-1], want[-1]) and np.array_equal(got[CM.CHUNK - 1], want[CM.CHUNK - 1])
    assert np.array_equal(got, want)


def test_all_digits_at_minus_half_the_base(engine):
    """(7, 4): the difference whose digits are all -B/2 = -64 in every coefficient of both halves, against selector rows
    of 0x7F7F7F80 (four plane bytes of -128): every byte-plane accumulator reaches 8192 x 64 x 128 = 2^26 at coefficient
    N - 1, where no term is negated -- the accumulator's extreme for this shape"""
    basebit, t = 7, 4
    word = np.uint32((0 - CM.offset(basebit, t) - CM.rounding(basebit, t)) & 0xFFFFFFFF)
    assert (CM.digits(word, basebit, t) == -64).all()
    rows = np.full((2 * t, 2, N), 0x7F7F7F80, np.uint32)
    d0 = _words(np.random.default_rng(8), (2, 2, N))
    with np.errstate(over="ignore"):
        d1 = d0 + word
    want = CM.cmux(rows, basebit, t, d0, d1)
    got = engine.batch_trlwe_cmux(rows, basebit, t, d0, d1)
    assert np.array_equal(got, want)
    assert np.array_equal(engine.batch_trlwe_cmux(rows, basebit, t, None, d1 - d0), CM.cmux(rows, basebit, t, None, d1 - d0))


# ---- forms --------------------------------------------------------------------------------------------------------------------
def test_external_product_is_the_call_without_d0(engine):
    basebit, t = 4, 6
    rows = _selector_rows(11, t)
    _, d = _inputs(12, 5, basebit, t)
    want = CM.external_product(rows, basebit, t, d)
    assert np.array_equal(engine.batch_trlwe_cmux(rows, basebit, t, None, d), want)
    assert np.array_equal(want, CM.cmux(rows, basebit, t, np.zeros_like(d), d))


def test_host_and_dev_forms_agree_on_a_callers_stream(engine):
    import torch

    basebit, t = 6, 3
    rows = _selector_rows(21, t)
    d0, d1 = _inputs(22, 67, basebit, t)
    host = engine.batch_trlwe_cmux(rows, basebit, t, d0, d1)
    dev = lambda a: torch.from_numpy(a.view(np.int32)).to("cuda:0")  # noqa: E731
    ts, t0, t1 = dev(rows), dev(d0), dev(d1)
    out = torch.full(t1.shape, -1, dtype=torch.int32, device="cuda:0")
    side = torch.cuda.Stream(device=0)
    side.wait_stream(torch.cuda.current_stream(0))
    res = engine.batch_trlwe_cmux(ts, basebit, t, t0, t1, out=out, stream=side)
    side.synchronize()
    assert res is out and np.array_equal(out.cpu().numpy().view(np.uint32), host)
    fresh = engine.batch_trlwe_cmux(ts, basebit, t, None, t1)  # a new tensor, torch's current stream, no d0
    torch.cuda.synchronize()
    assert np.array_equal(fresh.cpu().numpy().view(np.uint32), CM.external_product(rows, basebit, t, d1))
    assert np.array_equal(host, CM.cmux(rows, basebit, t, d0, d1))
    assert engine._lib.tfhe_hip_key_is_loaded(engine._ctx) == 0  # all of it on a context with no cloud key


# ---- selector encryption ---------------------------------------------------------------------------------------------------------
def _messages(count, seed):
    """+1, -1 X^7 and a dense small polynomial, in turn"""
    mu = np.zeros((count, N), np.int32)
    for m in range(count):
        if m % 3 == 0:
            mu[m, 0] = 1
        elif m % 3 == 1:
            mu[m, 7] = -1
        else:
            mu[m] = np.random.default_rng(seed + m).integers(-3, 4, N)
    return mu


@pytest.mark.parametrize("basebit,t,count,key", [(6, 3, 1, "random"), (6, 3, 3, "ones"), (1, 32, 1, "zeros"), (1, 32, 3, "random")])
def test_generated_selectors_equal_the_model(engine, basebit, t, count, key):
    """Every word of k_encrypt_trgsw under the fixed K, the row indices crossing a carry of the low nonce word: equal at
    alpha = 0; at alpha_lv1 a word may differ from the model by +-1 LSB only where the long-double sampler marks its
    noise sample borderline (KM.compare_words, at most 16 words)."""
    s = {"random": _secret(31), "ones": np.ones(N, np.uint32), "zeros": np.zeros(N, np.uint32)}[key]
    mu = _messages(count, 32)
    first = (1 << 32) - t - 1
    for alpha in (0.0, ALPHA):
        got, seed = engine.batch_encrypt_trgsw(s, mu, basebit, t, alpha=alpha, rng_key=K, first_index=first, return_seed=True)
        want, border, want_seed = CM.encrypt_trgsw(s, mu, basebit, t, alpha, K, first)
        differ = int((got != want).sum())
        _say(case="selectors", basebit=basebit, t=t, count=count, key=key, alpha=alpha, words=int(want.size),
             words_differing=differ, borderline=int(border.sum()), seed_equal=seed == want_seed)
        assert seed == want_seed == CM.mask_seed(K)
        assert got.shape == want.shape == (count, 2 * t, 2, N)
        if alpha == 0.0:
            assert np.array_equal(got, want)
        mism, _ = KM.compare_words(got, want, border, f"TRGSW ({basebit}, {t}) count {count} key {key} alpha {alpha}")
        assert mism <= KM.MAX_MISMATCHES


def test_selector_dev_form_equals_the_host_form(engine):
    import torch

    s, mu = _secret(33), _messages(2, 34)
    host = engine.batch_encrypt_trgsw(s, mu, 6, 3, alpha=ALPHA, rng_key=K, first_index=9)
    out = torch.full((2, 6, 2, N), -1, dtype=torch.int32, device="cuda:0")
    seed = engine.batch_encrypt_trgsw_dev(s, torch.from_numpy(mu).to("cuda:0"), 6, 3, out, alpha=ALPHA, rng_key=K, first_index=9)
    assert seed == CM.mask_seed(K)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), host)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_cmux_selects_between_two_packed_ciphertexts():
    """SECURITY_128_BIT: two packed ciphertexts of m = 16 messages, a selector of 0 and one of 1 made on the GPU, and the
    CMUX decrypts to the chosen one in all 1,024 slots"""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    m = 16
    sk = SecretKey.new(p, 41)
    msgs = np.random.default_rng(42).integers(0, m, (2, N))
    d0, d1 = (sk.encrypt_packed_lwe_message(msgs[i], m, seed=43 + i) for i in range(2))
    sels = sk.encrypt_trgsw_bool([0, 1], device=0)
    e = R.Engine(p, 0)
    try:
        for bit, sel in enumerate(sels):
            out = PK.cmux(sel, d0, d1, e)
            got = sk.decrypt_packed_lwe_message(out, N, m)
            _say(case="select", bit=bit, wrong=int((got != msgs[bit]).sum()))
            assert out.shape == (1, 2, N) and np.array_equal(got, msgs[bit])
    finally:
        e.close()


def test_lookup_returns_every_entry_within_the_noise_bound():
    """packing.lookup over 8 packed ciphertexts of m = 16 messages under three encrypted index bits: entry k for every
    k < 8, and every slot's phase error inside 8 sigma, sigma^2 = alpha^2 (the fresh encryption) + 3 times the CMUX's
    variance at mu = 1 of DESIGN section 9 (the larger of the two cases)"""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    m, d, basebit, t = 16, 3, 6, 3
    sk = SecretKey.new(p, 51)
    msgs = np.random.default_rng(52).integers(0, m, (1 << d, N))
    table = np.concatenate([sk.encrypt_packed_lwe_message(msgs[k], m, seed=60 + k) for k in range(1 << d)])
    sigma = CM.lookup_sigma(basebit, t, p.alpha_lv1, p.alpha_lv1, d)
    assert 8 * sigma < 1 / (4.0 * m)
    e = R.Engine(p, 0)
    try:
        for k in range(1 << d):
            sels = sk.encrypt_trgsw_bool([(k >> i) & 1 for i in range(d)], basebit, t, device=0)  # least significant first
            out = PK.lookup(sels, table, e)
            err = (sk.packed_phase(out, N).view(np.int32) / 2.0 ** 32) - msgs[k] / (2.0 * m)
            err -= np.round(err)
            got = sk.decrypt_packed_lwe_message(out, N, m)
            _say(case="lookup", k=k, wrong=int((got != msgs[k]).sum()), sigma=sigma, worst_in_sigma=float(np.abs(err).max() / sigma))
            assert out.shape == (2, N) and np.array_equal(got, msgs[k])
            assert np.abs(err).max() <= 8 * sigma
    finally:
        e.close()


def test_external_product_by_a_monomial_rotates_the_slots():
    """mu = X^5: the external product moves slot i to i + 5 with the sign of X^N = -1, as the plaintext product with
    linear.monomial(5) does"""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import linear as L
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    sk = SecretKey.new(p, 61)
    bits = np.random.default_rng(62).integers(0, 2, N).astype(bool)
    packed = sk.encrypt_packed_bool(bits, seed=63)
    mu = np.zeros(N, np.int32)
    mu[5] = 1
    sel = sk.encrypt_trgsw(mu, device=0)
    e = R.Engine(p, 0)
    try:
        got = sk.decrypt_packed_bool(PK.external_product(sel, packed, e), N)
        plain = sk.decrypt_packed_bool(e.batch_trlwe_polymul(L.monomial(5), packed)[:, 0], N)
    finally:
        e.close()
    assert np.array_equal(got, np.concatenate([~bits[N - 5:], bits[:N - 5]]))
    assert np.array_equal(got, plain)


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_error_codes_and_a_refused_call_writes_nothing(engine):
    from rs_tfhe_amd import _capi

    C = _capi.C
    lib = _capi.lib()
    ctx = engine._ctx
    rows = _selector_rows(71, 3)
    d0, d1 = _inputs(72, 3, 6, 3)
    out = np.full_like(d1, 0xAAAAAAAA)
    vp = C.c_void_p
    sp, p0, p1, op = (a.ctypes.data_as(vp) for a in (rows, d0, d1, out))
    host, devf = lib.tfhe_hip_batch_trlwe_cmux, lib.tfhe_hip_batch_trlwe_cmux_dev
    untouched = lambda: bool((out == 0xAAAAAAAA).all())  # noqa: E731
    assert host(None, sp, 6, 3, 0, p0, p1, 3, op) == _capi.EINVAL and devf(None, sp, 6, 3, 0, p0, p1, 3, op, None) == _capi.EINVAL
    for bad in ((None, p0, p1, op), (sp, p0, None, op), (sp, p0, p1, None)):
        s_, a_, b_, o_ = bad
        assert host(ctx, s_, 6, 3, 0, a_, b_, 3, o_) == _capi.EINVAL and devf(ctx, s_, 6, 3, 0, a_, b_, 3, o_, None) == _capi.EINVAL
    for b, t in ((0, 3), (8, 4), (6, 0), (1, 33), (4, 9), (7, 5), (-1, 3), (6, -1)):
        assert host(ctx, sp, b, t, 0, p0, p1, 3, op) == _capi.EINVAL and untouched(), (b, t)
        assert devf(ctx, sp, b, t, 0, p0, p1, 3, op, None) == _capi.EINVAL, (b, t)
        assert host(ctx, sp, b, t, 0, p0, p1, 0, op) == _capi.EINVAL, (b, t)  # the shape is checked ahead of the empty batch
    for flags in (2, 4, 3, -1):
        assert host(ctx, sp, 6, 3, flags, p0, p1, 3, op) == _capi.EINVAL and untouched(), flags
    assert host(ctx, sp, 6, 3, 0, p0, p1, 1 << 31, op) == _capi.EINVAL and untouched()
    assert host(ctx, sp, 6, 3, 0, p0, p1, 0, op) == _capi.OK and host(ctx, None, 6, 3, 0, None, None, 0, None) == _capi.OK and untouched()
    assert devf(ctx, None, 6, 3, 1, None, None, 0, None, None) == _capi.OK
    with pytest.raises(_capi.TfheHipError) as err:
        engine.batch_trlwe_cmux(rows, 8, 3, d0, d1)
    assert err.value.code == _capi.EINVAL
    assert host(ctx, sp, 6, 3, 0, p0, p1, 3, op) == _capi.OK and np.array_equal(out, CM.cmux(rows, 6, 3, d0, d1))
    # the encryption
    enc, encd = lib.tfhe_hip_batch_encrypt_trgsw, lib.tfhe_hip_batch_encrypt_trgsw_dev
    s, mu = _secret(73), _messages(1, 74)
    sel = np.full((1, 6, 2, N), 0xAAAAAAAA, np.uint32)
    kp, mp, ep = (a.ctypes.data_as(vp) for a in (s, mu, sel))
    rk, seed = (C.c_uint8 * 32).from_buffer_copy(K), (C.c_uint8 * 32)()
    al = C.c_double(ALPHA)
    clean = lambda: bool((sel == 0xAAAAAAAA).all())  # noqa: E731
    assert enc(None, kp, mp, 1, 6, 3, al, rk, 0, seed, ep) == _capi.EINVAL and encd(None, kp, mp, 1, 6, 3, al, rk, 0, seed, ep) == _capi.EINVAL
    for args in ((None, mp, 1, 6, 3, al, rk, 0, seed, ep), (kp, None, 1, 6, 3, al, rk, 0, seed, ep), (kp, mp, 1, 6, 3, al, rk, 0, seed, None),
                 (kp, mp, 1, 0, 3, al, rk, 0, seed, ep), (kp, mp, 1, 6, 33, al, rk, 0, seed, ep), (kp, mp, 1, 7, 5, al, rk, 0, seed, ep),
                 (kp, mp, 1, 6, 3, C.c_double(-1.0), rk, 0, seed, ep), (kp, mp, 1, 6, 3, C.c_double(float("nan")), rk, 0, seed, ep),
                 (kp, mp, 1, 6, 3, al, rk, (1 << 64) - 3, seed, ep), (kp, mp, (1 << 31) // 6 + 1, 6, 3, al, rk, 0, seed, ep)):
        assert enc(ctx, *args) == _capi.EINVAL and clean(), args[2:5]
        assert encd(ctx, *args) == _capi.EINVAL, args[2:5]
    two = s.copy()
    two[9] = 2
    assert enc(ctx, two.ctypes.data_as(vp), mp, 1, 6, 3, al, rk, 0, seed, ep) == _capi.EINVAL and clean()  # not binary
    assert enc(ctx, kp, None, 0, 6, 3, al, rk, 0, seed, None) == _capi.OK and clean()
    assert enc(ctx, kp, mp, 1, 6, 3, al, rk, 0, None, ep) == _capi.OK and not clean()  # mask_seed_out may be NULL
    assert np.array_equal(sel, engine.batch_encrypt_trgsw(s, mu, 6, 3, alpha=ALPHA, rng_key=K))
    t = _capi.CmuxTimes()
    assert lib.tfhe_hip_get_cmux_times(ctx, None) == _capi.EINVAL and lib.tfhe_hip_get_cmux_times(None, C.byref(t)) == _capi.EINVAL
    assert lib.tfhe_hip_get_cmux_times(ctx, C.byref(t)) == _capi.OK and t.passes == 0  # profiling is off


def test_times_count_the_passes():
    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    e = R.Engine(p, 0)
    try:
        e.set_profiling(True)
        rows = _selector_rows(81, 3)
        d0, d1 = _inputs(82, 3, 6, 3)
        e.batch_trlwe_cmux(rows, 6, 3, d0, d1)
        e.batch_trlwe_cmux(rows, 6, 3, None, d1)
        tm = e.cmux_times()
        _say(case="times", **tm)
        assert tm["passes"] == 2 and tm["digits_ms"] > 0 and tm["contraction_ms"] > 0 and tm["addend_ms"] > 0
        assert e.cmux_times()["passes"] == 0
    finally:
        e.close()


# ---- C++ ------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_cmux():
    """tests/cpp/test_cmux.cpp: Trgsw::encrypt_bool and packing::cmux select both ways in every slot, the external
    product keeps the message, the refused shapes throw."""
    import tempfile

    from test_cmux_host import build_cpp_cmux

    with tempfile.TemporaryDirectory() as d:
        exe = build_cpp_cmux(d)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test_cmux ok" in r.stdout
