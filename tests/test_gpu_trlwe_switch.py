"""The TRLWE key switch on the GPU (csrc/trlwe_switch.hpp behind tfhe_hip_batch_trlwe_keyswitch and its key calls) held to
the numpy model of tests/trlwe_switch_model.py: generated key bodies under DESIGN 11.2's borderline rule, the switch word
for word (np.array_equal, no tolerance) over the decompositions, automorphisms and batch sizes at which the kernels take
another path, the host and _dev forms, packed re-encryption, the trace and the slot reversal end to end, the error codes
and the handle's sixteen entries, and the C++ mirror.

Every test prints its figures (`TRLWESWITCH {json}` lines; run with -s) before it asserts."""
import json
import subprocess

import numpy as np
import pytest

import keygen_model as KM
import trlwe_switch_model as TM
from rs_tfhe_amd.params import N

pytestmark = pytest.mark.gpu

K = bytes((53 * i + 7) & 0xFF for i in range(32))  # a fixed generator key
ALPHA = 2.0e-8


def _say(**kv):
    print("TRLWESWITCH " + json.dumps(kv, default=float))


def _secret(seed):
    return np.random.default_rng(seed).integers(0, 2, N).astype(np.uint32)


def _words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def _edge_words(basebit, t):
    """0xFFFFFFFF and 0x7FFFFFFF (the rounding carry runs to the top, where the last carry is dropped) and, at every
    rounding boundary picked, the half step below it, the boundary and its neighbours"""
    bt = basebit * t
    w = [0, 1, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 0x80000001]
    if bt < 32:
        half = 1 << (31 - bt)
        for q in (1, (1 << bt) // 2, (1 << bt) - 1, (1 << bt) // 2 - 1):
            base = (q << (32 - bt)) & 0xFFFFFFFF
            w += [(base - half - 1) & 0xFFFFFFFF, (base - half) & 0xFFFFFFFF, (base - 1) & 0xFFFFFFFF, base, (base + half - 1) & 0xFFFFFFFF]
    return np.array(w, np.uint32)


def _inputs(seed, count, basebit, t):
    """[count][2][N] random words with the edge words planted at both ends of both rows of the first and last ciphertext"""
    ct = _words(np.random.default_rng(seed), (count, 2, N))
    e = _edge_words(basebit, t)
    for c in (0, count - 1):
        ct[c, :, :len(e)] = e
        ct[c, :, -len(e):] = e
    return ct


@pytest.fixture(scope="module")
def engine():
    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    e = R.Engine(p, 0)  # no cloud key: the switch needs none
    yield e
    e.close()


def _load_random_key(engine, k, basebit, t, seed):
    """a key of random bodies under a fixed seed (the switch is defined for any rows): (TrlweSwitchKey, model rows)"""
    from rs_tfhe_amd.packing import TrlweSwitchKey

    S = bytes((11 * i + seed) & 0xFF for i in range(32))
    bodies = _words(np.random.default_rng(1000 + seed), (t, N))
    bodies[:, :4] = (0xFFFFFFFF, 0x80000000, 0x7F7F7F80, 0)
    key = TrlweSwitchKey(k, basebit, t, S, bodies)
    engine.load_trlwe_switch_key(key)
    return key, TM.key_rows(S, k, t, bodies)


# ---- key bodies ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,basebit,t,alpha,distinct", [(1, 4, 6, ALPHA, True), (2047, 7, 4, ALPHA, False),
                                                         (513, 1, 32, KM.ALPHA_BSK_UINT, False), (3, 2, 16, 0.5, True)])
def test_generated_bodies_equal_the_model(engine, k, basebit, t, alpha, distinct):
    """The mask seed and every body word of k_gen_trlwe_switch_key under the fixed K: a word may differ from the model by
    +-1 LSB only where the long-double sampler marks its noise sample borderline (KM.compare_words, at most 16 words).
    At alpha = 2.2e-16 the noise truncates to zero in any arithmetic: plain equality."""
    s_from, s_to = _secret(21), (_secret(22) if distinct else _secret(21))
    got = engine.gen_trlwe_switch_key(s_from, s_to, k, basebit, t, rng_key=K, alpha=alpha)
    assert engine.trlwe_switch_key_is_loaded(k)
    engine.drop_trlwe_switch_key(k)
    m = TM.make_key(s_from, s_to, k, basebit, t, K, alpha)
    differ = int((got.bodies != m.bodies).sum())
    _say(case="bodies", k=k, basebit=basebit, t=t, alpha=alpha, words=int(m.bodies.size), words_differing=differ,
         borderline=int(m.border.sum()), seed_equal=got.mask_seed == m.mask_seed)
    assert got.mask_seed == m.mask_seed == TM.mask_seed(K)
    assert (got.k, got.basebit, got.t) == (k, basebit, t) and got.bodies.shape == m.bodies.shape
    if alpha == KM.ALPHA_BSK_UINT:
        assert np.array_equal(got.bodies, m.bodies)
    mism, _ = KM.compare_words(got.bodies, m.bodies, m.border, f"switching key k={k} ({basebit}, {t}) alpha {alpha}")
    assert mism <= KM.MAX_MISMATCHES


def test_load_reproduces_the_generating_handle():
    """switch on the generating handle, on a handle that loaded (S, bodies), on one generated with bodies = NULL, and in
    the model over (S, bodies): the same words"""
    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    s_from, s_to = _secret(31), _secret(32)
    ct = _inputs(33, 5, 4, 6)
    gen, other, quiet = R.Engine(p, 0), R.Engine(p, 0), R.Engine(p, 0)
    try:
        key = gen.gen_trlwe_switch_key(s_from, s_to, 3, 4, 6, rng_key=K, alpha=ALPHA)
        on_gen = gen.batch_trlwe_keyswitch(3, ct)
        other.load_trlwe_switch_key(key)
        on_other = other.batch_trlwe_keyswitch(3, ct)
        assert quiet.gen_trlwe_switch_key(s_from, s_to, 3, 4, 6, rng_key=K, alpha=ALPHA, download=False) is None
        on_quiet = quiet.batch_trlwe_keyswitch(3, ct)
        want = TM.switch(TM.key_rows(key.mask_seed, 3, 6, key.bodies), 3, 4, 6, ct)
        _say(case="handle", generating_equals_model=bool(np.array_equal(on_gen, want)),
             loaded_equals_model=bool(np.array_equal(on_other, want)), no_download_equals_model=bool(np.array_equal(on_quiet, want)))
        assert np.array_equal(on_gen, want), "the generating handle switches under another key than (S, bodies)"
        assert np.array_equal(on_other, want)
        assert np.array_equal(on_quiet, want), "bodies = NULL left another key on the handle"
    finally:
        for e in (gen, other, quiet):
            e.close()


# ---- the switch ------------------------------------------------------------------------------------------------------------
SWITCH_CASES = ([(3, b, t, 65) for b, t in TM.SHAPES]  # every decomposition; 65: a second 64-row block and the row tail
                + [(k, 4, 6, 3) for k in TM.KS if k != 3]  # every automorphism
                + [(1025, 4, 6, 1), (2047, 7, 3, 65), (1, 1, 32, 3)])


@pytest.mark.parametrize("k,basebit,t,count", SWITCH_CASES)
def test_switch_equals_the_model(engine, k, basebit, t, count):
    key, rows = _load_random_key(engine, k, basebit, t, seed=k % 97 + t)
    ct = _inputs(100 * k + count, count, basebit, t)
    want = TM.switch(rows, k, basebit, t, ct)
    got = engine.batch_trlwe_keyswitch(k, ct)
    engine.drop_trlwe_switch_key(k)
    assert got.shape == (count, 2, N) and got.dtype == np.uint32
    assert np.array_equal(got, want)


def test_a_batch_that_crosses_a_chunk(engine):
    """kTsChunk + 1 ciphertexts: the last one takes a second pass through the digit scratch and lands behind the first
    pass's output"""
    from rs_tfhe_amd.packing import TRLWE_SWITCH_CHUNK

    k, basebit, t = 1025, 7, 3
    key, rows = _load_random_key(engine, k, basebit, t, seed=5)
    ct = _inputs(77, TRLWE_SWITCH_CHUNK + 1, basebit, t)
    want = TM.switch(rows, k, basebit, t, ct)
    got = engine.batch_trlwe_keyswitch(k, ct)
    engine.drop_trlwe_switch_key(k)
    assert np.array_equal(got[-1], want[-1]) and np.array_equal(got[TRLWE_SWITCH_CHUNK - 1], want[TRLWE_SWITCH_CHUNK - 1])
    assert np.array_equal(got, want)


def test_all_digits_at_plus_half_the_base(engine):
    """beta = 7, t = 4: the word whose digits are all -B/2 = -64 (0x3F 0x3F 0x3F 0x40 in base 128 after the carries,
    shifted past the four bits that are rounded away) in every coefficient makes every NEGATED digit +64, the one value
    outside [-B/2, B/2) the int8 planes carry, and with bodies of 0x7F7F7F80 (four plane bytes of -128) every
    byte-plane accumulator of the b half reaches 4096 x 64 x 128 = 2^25 at coefficient N - 1, where no term is negated."""
    from rs_tfhe_amd.packing import TrlweSwitchKey

    basebit, t, k = 7, 4, 1
    word = np.uint32(((63 << 21) | (63 << 14) | (63 << 7) | 64) << 4)
    assert (TM.digits(word, basebit, t) == -64).all()
    S = bytes(range(32))
    key = TrlweSwitchKey(k, basebit, t, S, np.full((t, N), 0x7F7F7F80, np.uint32))
    engine.load_trlwe_switch_key(key)
    ct = _words(np.random.default_rng(8), (2, 2, N))
    ct[:, 0] = word
    want = TM.switch(TM.key_rows(S, k, t, key.bodies), k, basebit, t, ct)
    got = engine.batch_trlwe_keyswitch(k, ct)
    engine.drop_trlwe_switch_key(k)
    assert np.array_equal(got, want)


def test_host_and_dev_forms_agree_on_a_callers_stream(engine):
    import torch

    k, basebit, t = 513, 4, 6
    key, rows = _load_random_key(engine, k, basebit, t, seed=9)
    ct = _inputs(55, 67, basebit, t)
    host = engine.batch_trlwe_keyswitch(k, ct)
    tin = torch.from_numpy(ct.view(np.int32)).to("cuda:0")
    out = torch.full(tin.shape, -1, dtype=torch.int32, device="cuda:0")
    side = torch.cuda.Stream(device=0)
    side.wait_stream(torch.cuda.current_stream(0))
    res = engine.batch_trlwe_keyswitch(k, tin, out=out, stream=side)
    side.synchronize()
    assert res is out and np.array_equal(out.cpu().numpy().view(np.uint32), host)
    fresh = engine.batch_trlwe_keyswitch(k, tin)  # a new tensor, torch's current stream
    torch.cuda.synchronize()
    assert np.array_equal(fresh.cpu().numpy().view(np.uint32), host)
    engine.drop_trlwe_switch_key(k)
    assert np.array_equal(host, TM.switch(rows, k, basebit, t, ct))


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("set_name", ["SECURITY_128_BIT", "SECURITY_UINT4"])
def test_packed_reencryption_end_to_end(set_name):
    """encrypt_packed_bool under Alice, PackedReencryptionKey.reencrypt, decrypt under Bob: every bit, two ciphertexts"""
    import rs_tfhe_amd as R
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.proxy_reenc import PackedReencryptionKey

    p = getattr(R.params, set_name)
    alice, bob = SecretKey.new(p, 41), SecretKey.new(p, 42)
    bits = np.random.default_rng(43).integers(0, 2, 2 * N).astype(bool)
    packed = alice.encrypt_packed_bool(bits, seed=44)
    with PackedReencryptionKey.new_symmetric(alice, bob) as rk:
        assert (rk.key.k, rk.key.basebit, rk.key.t) == (1, 4, 6) and rk.key.nbytes == 6 * N * 4 + 32
        out = rk.reencrypt(packed)
        one = rk.reencrypt(packed[0])
    assert out.shape == packed.shape and one.shape == (2, N) and np.array_equal(one, out[0])
    got = bob.decrypt_packed_bool(out, 2 * N)
    _say(case="reencrypt", set=set_name, wrong=int((got != bits).sum()), key_bytes=rk.key.nbytes)
    assert np.array_equal(got, bits)
    assert (alice.decrypt_packed_bool(out, 2 * N) == bits).mean() < 0.75  # Alice's key no longer reads it


def test_inner_product_then_trace_end_to_end():
    """SECURITY_UINT4, m = 16.  x_j in {0..3}, j < 8, encrypted at x_j / (2 m 2^10) -- the trace's caller encodes at
    message / 2^steps -- times W(X) = w_0 - sum_{j >= 1} w_j X^(N - j) puts sum_j w_j x_j in coefficient 0 and partial
    sums in the others; trace(10) multiplies coefficient 0 by 1,024 and clears the rest.  Bound on a cleared slot: the
    surviving coefficient's noise is 2^10 sqrt(V_in + V_switch / 3) (each step doubles what it keeps and adds one
    switch), a cleared one's is smaller (it only collects the switches after it was cleared); V_in = sum w^2 alpha^2 and
    V_switch the header's two-term variance.  8 sigma of that is asserted on all 1,023 cleared slots."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import SECURITY_UINT4 as p

    m, steps, basebit, t = 16, 10, 4, 6
    x = np.array([3, 1, 0, 2, 3, 3, 1, 2])
    w = np.array([1, 1, 0, 1, 1, 0, 1, 1])
    want = int((w * x).sum())
    assert want == 12 < m
    sk = SecretKey.new(p, 51)
    plain = np.zeros(N)
    plain[:8] = x / (2.0 * m * (1 << steps))
    plain[8:] = np.random.default_rng(52).integers(0, 4, N - 8) / (2.0 * m * (1 << steps))  # what the trace must clear
    packed = sk.encrypt_packed_f64(plain, seed=53)
    W = np.zeros(N, np.int8)
    W[0] = w[0]
    W[N - np.arange(1, 8)] = -w[1:]
    e = R.Engine(p, 0)
    try:
        keys = PK.gen_trace_keys(e, sk, steps, basebit, t)
        assert [k.k for k in keys] == PK.trace_ks(steps) and all(e.trlwe_switch_key_is_loaded(k.k) for k in keys)
        prod = e.batch_trlwe_polymul(W, packed)[:, 0]  # [1][2][N]
        pre = sk.packed_phase(prod, N).view(np.int32) / 2.0 ** 32
        assert np.abs(pre[1:]).max() > 1e-4  # the by-products are there before the trace
        out = PK.trace(prod, steps, e)
    finally:
        e.close()
    ph = sk.packed_phase(out, N).view(np.int32) / 2.0 ** 32
    sigma = (1 << steps) * np.sqrt(float((w * w).sum()) * p.alpha_lv1 ** 2 + TM.switch_variance(basebit, t, p.alpha_lv1) / 3)
    got = int(sk.decrypt_packed_lwe_message(out, 1, m)[0])
    _say(case="trace", got=got, want=want, sigma=sigma, worst_cleared_in_sigma=float(np.abs(ph[1:]).max() / sigma),
         slot0_error_in_sigma=float(abs(ph[0] - want / (2.0 * m)) / sigma))
    assert got == want
    assert abs(ph[0] - want / (2.0 * m)) <= 8 * sigma < 1 / (4.0 * m)
    assert np.abs(ph[1:]).max() <= 8 * sigma


def test_automorphism_2047_reverses_the_slots():
    """psi_(2N-1): slot j moves to N - j with the sign flipped, slot 0 stays"""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    sk = SecretKey.new(p, 61)
    bits = np.random.default_rng(62).integers(0, 2, N).astype(bool)
    packed = sk.encrypt_packed_bool(bits, seed=63)
    e = R.Engine(p, 0)
    try:
        e.gen_trlwe_switch_key(sk.key_lv1, sk.key_lv1, 2 * N - 1, download=False)
        got = sk.decrypt_packed_bool(PK.automorphism(packed, 2 * N - 1, e), N)
    finally:
        e.close()
    want = np.concatenate([bits[:1], ~bits[1:][::-1]])
    assert np.array_equal(got, want)


# ---- errors and the handle's entries ---------------------------------------------------------------------------------------
def test_error_codes_and_the_sixteen_entries():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi
    from rs_tfhe_amd.packing import TRLWE_SWITCH_MAX_KEYS, TrlweSwitchKey
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    C = _capi.C
    lib = _capi.lib()
    eng = R.Engine(p, 0)
    try:
        ctx = eng._ctx
        s1, s2 = _secret(71), _secret(72)
        ct = _inputs(73, 3, 4, 6)
        out = np.full_like(ct, 0xAAAAAAAA)
        vp = C.c_void_p
        ip, op, k1, k2 = (a.ctypes.data_as(vp) for a in (ct, out, s1, s2))
        seed, rk = (C.c_uint8 * 32)(), (C.c_uint8 * 32).from_buffer_copy(K)
        bodies = np.zeros((6, N), np.uint32)
        bp = bodies.ctypes.data_as(vp)
        host, devf = lib.tfhe_hip_batch_trlwe_keyswitch, lib.tfhe_hip_batch_trlwe_keyswitch_dev
        gen, load = lib.tfhe_hip_gen_trlwe_switch_key, lib.tfhe_hip_load_trlwe_switch_key
        # no key yet
        assert host(ctx, 3, ip, 3, op) == _capi.ENOKEY and devf(ctx, 3, ip, 3, op, None) == _capi.ENOKEY
        assert host(ctx, 3, None, 0, None) == _capi.ENOKEY and lib.tfhe_hip_drop_trlwe_switch_key(ctx, 3) == _capi.ENOKEY
        assert lib.tfhe_hip_trlwe_switch_key_is_loaded(ctx, 3) == 0 and lib.tfhe_hip_trlwe_switch_key_is_loaded(None, 3) == 0
        assert host(None, 3, ip, 3, op) == _capi.EINVAL and devf(None, 3, ip, 3, op, None) == _capi.EINVAL
        words = C.c_size_t()
        assert lib.tfhe_hip_trlwe_switch_key_words(6, C.byref(words)) == _capi.OK and words.value == 6 * N
        for bad_t in (0, 65, -1):
            assert lib.tfhe_hip_trlwe_switch_key_words(bad_t, C.byref(words)) == _capi.EINVAL
        assert lib.tfhe_hip_trlwe_switch_key_words(6, None) == _capi.EINVAL
        # a key for k = 3, then every refusal leaves it answering
        assert gen(ctx, k1, k2, 3, 4, 6, C.c_double(ALPHA), rk, seed, bp) == _capi.OK
        key = TrlweSwitchKey(3, 4, 6, bytes(seed), bodies)
        want = TM.switch(TM.key_rows(key.mask_seed, 3, 6, key.bodies), 3, 4, 6, ct)

        def answering():
            return lib.tfhe_hip_trlwe_switch_key_is_loaded(ctx, 3) == 1 and np.array_equal(eng.batch_trlwe_keyswitch(3, ct), want)

        assert answering()
        bad_shapes = ((2, 4, 6), (0, 4, 6), (-3, 4, 6), (2 * N, 4, 6), (2 * N + 1, 4, 6),  # k even / out of range
                      (3, 0, 6), (3, 8, 4), (3, 4, 0), (3, 1, 65), (3, 4, 9), (3, 7, 5))  # beta, t, beta t > 32
        for k, b, t in bad_shapes:
            assert gen(ctx, k1, k2, k, b, t, C.c_double(ALPHA), rk, seed, None) == _capi.EINVAL, (k, b, t)
            assert load(ctx, k, b, t, seed, bp) == _capi.EINVAL, (k, b, t)
            assert answering(), (k, b, t)
        for alpha in (-1.0, float("nan")):
            assert gen(ctx, k1, k2, 3, 4, 6, C.c_double(alpha), rk, seed, None) == _capi.EINVAL and answering()
        for args in ((None, k2, 3, 4, 6, C.c_double(ALPHA), rk, seed, None), (k1, None, 3, 4, 6, C.c_double(ALPHA), rk, seed, None),
                     (k1, k2, 3, 4, 6, C.c_double(ALPHA), rk, None, None)):
            assert gen(ctx, *args) == _capi.EINVAL and answering()
        assert load(ctx, 3, 4, 6, None, bp) == _capi.EINVAL and load(ctx, 3, 4, 6, seed, None) == _capi.EINVAL and answering()
        assert gen(None, k1, k2, 3, 4, 6, C.c_double(ALPHA), rk, seed, None) == _capi.EINVAL
        assert load(None, 3, 4, 6, seed, bp) == _capi.EINVAL and lib.tfhe_hip_drop_trlwe_switch_key(None, 3) == _capi.EINVAL
        # the switch's own refusals; count == 0 writes nothing
        for bad in ((None, 3, op), (ip, 3, None)):
            assert host(ctx, 3, *bad) == _capi.EINVAL and devf(ctx, 3, *bad, None) == _capi.EINVAL
        assert host(ctx, 3, None, 0, None) == _capi.OK and devf(ctx, 3, None, 0, None, None) == _capi.OK
        assert host(ctx, 3, ip, 0, op) == _capi.OK and (out == 0xAAAAAAAA).all()
        assert host(ctx, 5, ip, 3, op) == _capi.ENOKEY  # another k
        # generating a cloud key leaves the entry in place
        sk = KM.secret_key(p)
        eng.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=5)
        assert eng._lib.tfhe_hip_key_is_loaded(ctx) == 1 and answering()
        # fifteen more keys fit, the seventeenth is refused, the sixteen still answer; replacing one of them is no new key
        small = TrlweSwitchKey(5, 7, 1, bytes(seed), np.zeros((1, N), np.uint32))
        others = [5 + 2 * i for i in range(TRLWE_SWITCH_MAX_KEYS - 1)]
        for k in others:
            small.k = k
            eng.load_trlwe_switch_key(small)
        assert all(eng.trlwe_switch_key_is_loaded(k) for k in [3] + others)
        assert load(ctx, 101, 7, 1, seed, bp) == _capi.EINVAL
        assert gen(ctx, k1, k2, 101, 7, 1, C.c_double(ALPHA), rk, seed, None) == _capi.EINVAL
        assert not eng.trlwe_switch_key_is_loaded(101) and answering()
        small.k = others[0]
        eng.load_trlwe_switch_key(small)  # an entry that exists: replaced in place
        # drop, then switch: ENOKEY; the freed entry takes the key refused before
        eng.drop_trlwe_switch_key(3)
        assert not eng.trlwe_switch_key_is_loaded(3) and host(ctx, 3, ip, 3, op) == _capi.ENOKEY
        with pytest.raises(_capi.TfheHipError) as err:
            eng.batch_trlwe_keyswitch(3, ct)
        assert err.value.code == _capi.ENOKEY
        assert load(ctx, 101, 7, 1, seed, bp) == _capi.OK and eng.trlwe_switch_key_is_loaded(101)
        # a key view has entries of its own
        view = eng.new_key_view()
        try:
            assert not view.trlwe_switch_key_is_loaded(101)
            view.load_trlwe_switch_key(key)
            assert np.array_equal(view.batch_trlwe_keyswitch(3, ct), want) and not eng.trlwe_switch_key_is_loaded(3)
        finally:
            view.close()
    finally:
        eng.close()


# ---- C++ -------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_trlwe_switch():
    """tests/cpp/test_trlwe_switch.cpp: TrlweSwitchKey::generate / load / switch_batch -- packed re-encryption decoded under
    the target key, the loaded copy against the generated key, the slot reversal, the refused shapes."""
    import tempfile

    from test_trlwe_switch_host import build_cpp_trlwe_switch

    with tempfile.TemporaryDirectory() as d:
        exe = build_cpp_trlwe_switch(d)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test_trlwe_switch ok" in r.stdout
