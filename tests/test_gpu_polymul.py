"""Plaintext polynomial products on packed ciphertexts on the GPU: tfhe_hip_batch_trlwe_polymul equals
rs_tfhe_amd.linear.polymul_model word for word (np.array_equal, no tolerance) -- monomials at every boundary of the
kernel's walk, dense weights with a row tail and a second row block, the accumulator bound at cols = 64 --, agrees with
the packed matmul on the same memory, the _dev form gives the host form's bits on a side stream, the error codes, the
packed convolution and a slot rotation end to end, and the C++ mirror."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1024
EDGES = (0, 0x80000000, 0xFFFFFFFF, 0x7F7F7F7F, 0x80808080, 0x00800080, 0x7FFFFFFF)  # carries between balanced byte planes
MONOMIAL_K = (0, 1, 15, 16, 17, 31, 32, 127, 128, 129, 1023)  # around a 16-row fetch, a K-step of 32, a column block of 128


def distinct_words(rng, shape):
    """All different u32 words, none of them one of the planted values."""
    n = int(np.prod(shape))
    v = rng.permutation(n).astype(np.uint32) * np.uint32(2654435761) + np.uint32(12345)  # an odd multiplier: a bijection
    assert len(np.unique(v)) == n and not np.isin(v, (0, 0x80000000, 0xFFFFFFFF)).any()
    return v.reshape(shape)


def dev(a):
    import torch

    return torch.from_numpy(a.view(np.int8 if a.dtype == np.int8 else np.int32)).to("cuda:0")


@pytest.fixture(scope="module")
def engine():
    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    e = R.Engine(p, 0)  # no key: the product needs none
    yield e
    e.close()


def test_monomials_rotate_with_the_negacyclic_sign(engine):
    """rows = cols = groups = 1, w = +-X^k.  The a row and the b row hold different, all distinct words, so a wrap that
    read the other component's tail (an index that ran below the polynomial instead of being masked into it) shows: the
    test first checks that such a reader's result differs from the definition's.  Two inputs, so that 0, 0x80000000 and
    0xFFFFFFFF each stand at coefficient 0 and at coefficient N - 1 and both rows carry them at both ends."""
    from rs_tfhe_amd import linear as L

    rng = np.random.default_rng(11)
    for plant in (((0, 0, 0), (0, N - 1, 0x80000000), (1, 0, 0xFFFFFFFF)),
                  ((0, 0, 0x80000000), (0, N - 1, 0xFFFFFFFF), (1, N - 1, 0))):
        ct = distinct_words(rng, (1, 1, 2, N))
        for c, i, v in plant:
            ct[0, 0, c, i] = v
        assert len(np.unique(ct)) == 2 * N
        for k in MONOMIAL_K:
            for sign in (1, -1):
                w = L.monomial(k, sign)
                want = L.polymul_model(w, ct)
                if k:  # what a reader of the other component's tail would return
                    wrong = want.copy()
                    wrong[0, 0, 0, :k], wrong[0, 0, 1, :k] = want[0, 0, 1, :k], want[0, 0, 0, :k]
                    assert not np.array_equal(wrong[0, 0, 0], want[0, 0, 0]) and not np.array_equal(wrong[0, 0, 1], want[0, 0, 1])
                got = engine.batch_trlwe_polymul(w, ct)
                assert got.shape == (1, 1, 2, N) and got.dtype == np.uint32
                assert np.array_equal(got, want), (k, sign)


def dense_case(seed, rows=65, cols=3, groups=3):
    rng = np.random.default_rng(seed)
    w = rng.integers(-128, 128, (rows, cols, N)).astype(np.int8)
    w[0], w[1], w[2] = -128, 127, 0
    trlwe = rng.integers(0, 1 << 32, (groups, cols, 2, N), dtype=np.uint32)
    trlwe[..., :len(EDGES)] = EDGES
    trlwe[..., -len(EDGES):] = EDGES
    bias = rng.integers(0, 1 << 32, (rows, N), dtype=np.uint32)
    return w, trlwe, bias


def test_dense_weights_row_tail_second_row_block_and_bias(engine):
    """rows = 65 (a second row block of one row), cols = 3 (K crosses polynomial boundaries), groups = 3, weights over the
    full int8 range, a bias polynomial: the b rows carry it, the a rows equal the model computed WITHOUT bias.  The
    _dev form runs on a side stream with w at an odd address and gives the same bits."""
    import torch
    from rs_tfhe_amd import linear as L

    w, trlwe, bias = dense_case(21)
    want, plain = L.polymul_model(w, trlwe, bias), L.polymul_model(w, trlwe)
    assert not np.array_equal(want[:, :, 1], plain[:, :, 1])
    got = engine.batch_trlwe_polymul(w, trlwe, bias)
    assert np.array_equal(got[:, :, 0], plain[:, :, 0])
    assert np.array_equal(got, want)
    assert np.array_equal(engine.batch_trlwe_polymul(w, trlwe), plain)  # bias NULL

    side = torch.cuda.Stream(device=0)
    flat = torch.zeros(w.size + 16, dtype=torch.int8, device="cuda:0")
    tw = flat[1:1 + w.size].view(w.shape)  # one byte past an aligned address
    tw.copy_(dev(w))
    assert tw.data_ptr() % 2 == 1 and tw.is_contiguous()
    tb, tin = dev(bias), dev(trlwe)
    out = torch.full(want.shape, -1, dtype=torch.int32, device="cuda:0")
    side.wait_stream(torch.cuda.current_stream(0))
    engine.batch_trlwe_polymul_dev(tw, tin, out, bias=tb, stream=side)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    out.fill_(-1)
    engine.batch_trlwe_polymul_dev(dev(w), tin, out)  # aligned w, bias None, torch's current stream
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), plain)


@pytest.mark.parametrize("case", ["bound", "carries"])
def test_accumulator_bound_at_64_polynomials(engine, case):
    """rows = 1, cols = 64 (K = 65,536), all weights -128.  bound: every word 0x7F7F7F80, whose four balanced plane
    bytes are all -128: at coefficient N - 1 no term is negated and every plane accumulates 65,536 * 2^14 = 2^30, the
    bound the header states.  carries: random words with the values that carry between the planes planted."""
    from rs_tfhe_amd import linear as L

    cols = 64
    w = np.full((1, cols, N), -128, np.int8)
    if case == "bound":
        trlwe = np.full((1, cols, 2, N), 0x7F7F7F80, np.uint32)
        assert (((trlwe[0, 0, 0, :1] + np.uint32(0x80808080)) ^ np.uint32(0x80808080)) == 0x80808080).all()  # planes: -128 x 4
    else:
        rng = np.random.default_rng(31)
        trlwe = rng.integers(0, 1 << 32, (1, cols, 2, N), dtype=np.uint32)
        trlwe[..., :len(EDGES)] = EDGES
        trlwe[..., -len(EDGES):] = EDGES
        trlwe[0, ::2, :, 100:200] = 0x80808080
    bias = np.full((1, N), 0xDEADBEEF, np.uint32)
    assert np.array_equal(engine.batch_trlwe_polymul(w, trlwe, bias), L.polymul_model(w, trlwe, bias))


def test_slot_n_minus_1_of_the_product_is_the_packed_matmul(engine):
    """cols = 1, rows = 1: coefficient N - 1 of w(X) * ct(X) is sum_j w[N - 1 - j] * slot j, so the exact lv1 extraction
    of slot N - 1 of the product equals batch_trlwe_matmul(keyswitch=False) with the N weights reversed, on the same
    ciphertext: the new loader against the one already trusted."""
    from rs_tfhe_amd import linear as L

    rng = np.random.default_rng(41)
    w = rng.integers(-128, 128, N).astype(np.int8)
    ct = rng.integers(0, 1 << 32, (2, 2, N), dtype=np.uint32)  # two groups
    ct[:, :, :len(EDGES)] = EDGES
    ct[:, :, -len(EDGES):] = EDGES
    prod = engine.batch_trlwe_polymul(w, ct)  # [2][1][2][N]
    rows = L.extract_rows_exact(prod[:, 0], [N - 1, 2 * N - 1])
    mm = engine.batch_trlwe_matmul(w[::-1].reshape(1, N), ct, keyswitch=False)  # [2][1][N+1]
    assert np.array_equal(rows, mm[:, 0])


def test_error_codes_and_the_empty_batch(engine):
    from rs_tfhe_amd import _capi

    lib = _capi.lib()
    vp = _capi.C.c_void_p
    w = np.ones((3, 2, N), np.int8)
    trlwe = np.zeros((2, 2, 2, N), np.uint32)
    out = np.full((2, 3, 2, N), 0xAAAAAAAA, np.uint32)
    wp, tp, op = (a.ctypes.data_as(vp) for a in (w, trlwe, out))
    host, devf = lib.tfhe_hip_batch_trlwe_polymul, lib.tfhe_hip_batch_trlwe_polymul_dev
    ctx = engine._ctx
    for bad in ((None, None, 3, 2, tp, 2, op), (wp, None, 3, 2, None, 2, op), (wp, None, 3, 2, tp, 2, None),  # NULL w, trlwe, out
                (wp, None, 0, 2, tp, 2, op), (wp, None, 3, 0, tp, 2, op), (wp, None, 3, 65, tp, 2, op),       # rows, cols
                (wp, None, 1 << 16, 2, tp, 1 << 15, op), (wp, None, 1 << 31, 2, tp, 1, op)):                   # rows * groups
        assert host(ctx, *bad) == _capi.EINVAL, bad
        assert devf(ctx, *bad, None) == _capi.EINVAL, bad
    assert host(None, wp, None, 3, 2, tp, 2, op) == _capi.EINVAL
    assert devf(None, wp, None, 3, 2, tp, 2, op, None) == _capi.EINVAL
    assert host(ctx, None, None, 3, 2, None, 0, None) == _capi.OK  # groups == 0 writes nothing
    assert devf(ctx, None, None, 3, 2, None, 0, None, None) == _capi.OK
    assert host(ctx, wp, None, 3, 2, tp, 0, op) == _capi.OK and (out == 0xAAAAAAAA).all()
    assert engine.batch_trlwe_polymul(w, trlwe[:0]).shape == (0, 3, 2, N)
    assert not engine.batch_trlwe_polymul(w, trlwe).any()  # the handle still works: zeros in, zeros out
    assert host(ctx, wp, None, 3, 64, tp, 0, op) == _capi.OK  # cols = 64 is in range


def test_packed_convolution_end_to_end():
    """y = min(conv(x) + b, 3) on SECURITY_UINT4, m = 16, as test_gpu_conv2d.test_one_convolutional_layer_end_to_end
    demands of the LWE route: a 1 x 6 x 6 map of messages in {0, 1, 2} packed by the client into ONE ciphertext, one
    2 x 2 filter with weights in {0, 1}, bias 1: every sum is at most 3 * 2 + 1 = 7 < 16.  The server multiplies by the
    plan's polynomial, unpacks the plan's 25 slots and bootstraps.  The packed input's noise (alpha_lv1) grows by at
    most sqrt(3), then by the key switch's, against a decoding margin of 1/64; with this weight range and modulus the
    CPU route (polymul_model, packing.unpack_model, the oracle's bootstrap) decoded every output before the GPU saw
    the case.  All 25 outputs are asserted."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import linear as L
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.lut import Generator
    from rs_tfhe_amd.params import SECURITY_UINT4 as p

    m, b = 16, 1
    img = np.array([[[0, 1, 2, 0, 0, 1], [0, 0, 1, 0, 2, 0], [0, 0, 0, 1, 0, 0], [1, 2, 2, 2, 0, 1], [0, 0, 1, 0, 0, 0],
                     [2, 0, 0, 1, 1, 2]]])
    k = np.array([[1, 0], [1, 1]])
    pre = np.array([[(img[0, oy:oy + 2, ox:ox + 2] * k).sum() + b for ox in range(5)] for oy in range(5)])
    assert pre.min() < 3 < pre.max() <= m - 1
    want = np.minimum(pre, 3).reshape(-1)
    plan = L.conv2d_packed_plan(1, 6, 6, 2, 2)
    assert plan.slots.shape == (5, 5)
    wp = L.conv2d_packed_weights(k.reshape(1, 2, 2, 1).astype(np.int8), plan)
    bias = np.zeros((1, N), np.uint32)
    bias[0, plan.slots.reshape(-1)] = np.uint32(b) << np.uint32(32 - 5)  # b / (2 m) on the torus, m = 16
    tv = Generator(m).generate_lookup_table(lambda v: min(v, 3)).poly
    sk = SecretKey.new(p, 91)
    e = R.Engine(p, 0)
    try:
        e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=92)
        packed = sk.encrypt_packed_lwe_message(plan.encode(img), m, seed=93)  # [1][2][N]: 8 KiB for the whole map
        prod = e.batch_trlwe_polymul(wp, packed, bias)
        assert np.array_equal(prod, L.polymul_model(wp, packed, bias))
        assert np.array_equal(sk.decrypt_packed_lwe_message(prod[0, 0], N, m)[plan.slots.reshape(-1)], pre.reshape(-1))
        lin = e.unpack(prod[:, 0], slots=plan.slots)
        assert np.array_equal(sk.decrypt_lwe_message(lin, m), pre.reshape(-1))  # (pre < m: no wrap)
        out = e.batch_bootstrap(lin, tv)
        assert np.array_equal(sk.decrypt_lwe_message(out, m), want)
    finally:
        e.close()


def test_slot_rotation_end_to_end(engine):
    """encrypt_packed_bool, times X^k, decrypt_packed_bool: bit i moves to slot i + k, and the bits that pass N come back
    at the bottom inverted (X^N = -1 negates +-1/8)."""
    from rs_tfhe_amd import linear as L
    from rs_tfhe_amd.client import SecretKey

    rng = np.random.default_rng(61)
    sk = SecretKey.new(engine.params, 62)
    bits = rng.integers(0, 2, N).astype(bool)
    packed = sk.encrypt_packed_bool(bits, seed=63)
    for k, sign in ((0, 1), (1, 1), (300, 1), (1023, -1)):
        got = sk.decrypt_packed_bool(engine.batch_trlwe_polymul(L.monomial(k, sign), packed)[0, 0], N)
        want = np.concatenate([~bits[N - k:], bits[:N - k]])
        assert np.array_equal(got, want if sign > 0 else ~want), (k, sign)


def test_cpp_mirror_polymul():
    """tests/cpp/test_polymul.cpp: linear::polymul and linear::monomial against the definition's loops, and the refused
    shapes."""
    import tempfile

    from test_polymul_host import build_cpp_polymul

    with tempfile.TemporaryDirectory() as d:
        exe = build_cpp_polymul(d)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test_polymul ok" in r.stdout
