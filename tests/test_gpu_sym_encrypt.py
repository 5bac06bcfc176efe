"""Symmetric encryption on the GPU (csrc/sym_encrypt.hpp: k_lwe_rows of csrc/keygen.hpp behind tfhe_hip_batch_encrypt[_dev] /
tfhe_hip_gen_public_key / tfhe_hip_gen_reenc_key_symmetric) held to the term-by-term CPU model of
tests/sym_encrypt_model.py.

Under a fixed generator key every mask word and every noise sample is a keystream position the model knows: at
alpha = 0 the words must be EQUAL; with noise a body may differ from the model's by exactly +-1 LSB only where the
long-double sampler marks its sample borderline, at most 16 words a case (KM.compare_words; the cap on the inputs is
checked on the CPU by tests/test_sym_encrypt_host.py).  The shapes are the smallest at which the kernel can go wrong:
n = 33 (n % 16 = 1: the tail block), n = 16 (exactly one block), n = 48 (whole blocks), and one real set with n > 1024
for the wave's second pass over the blocks.  The model could share a mistake with the kernel; the statistics of noise
recovered with the secret key alone, and decryption, could not.

Every test prints its figures (`SYMENCRYPT {json}` lines; run with -s) before it asserts."""
import json
import subprocess

import numpy as np
import pytest

import dev_buffers as DB
import keygen_model as KM
import sym_encrypt_model as SM
from test_sym_encrypt_host import build_cpp_sym_encrypt
from rs_tfhe_amd.client import SecretKey, f64_to_torus

pytestmark = pytest.mark.gpu

K, SEED = SM.K, SM.SEED
SHAPE = SM.SHAPES[0]


def _say(**kv):
    print("SYMENCRYPT " + json.dumps(kv, default=float))


def _dev_encrypt(eng, key_lv0, plain, alpha, first_index, full, rng_key=K):
    """batch_encrypt_dev on a stream of the caller's, back on the host: [count][n+1] (full) or the bodies"""
    import torch

    tp = torch.from_numpy(np.ascontiguousarray(plain, np.uint32).view(np.int32)).cuda()
    out = torch.empty((len(plain), eng.params.n + 1), dtype=torch.int32, device="cuda") if full else None
    bod = None if full else torch.empty(len(plain), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.batch_encrypt_dev(key_lv0, tp, alpha, SEED, rng_key, first_index, bodies=bod, out=out, stream=s)
    s.synchronize()
    return (out if full else bod).cpu().numpy().view(np.uint32)


def _phase_error(sk, cts, plain):
    return (sk.phase(cts) - np.asarray(plain, np.uint32)).view(np.int32).astype(np.float64) / 2.0 ** 32


# ---- 1. bulk encryption ----------------------------------------------------------------------------------------------
def _bulk_case(p, sk, count, first_index, alpha):
    import rs_tfhe_amd as R
    from rs_tfhe_amd.seeded import SeededCiphertexts

    plain = SM.plaintexts(count, p.n + count)
    eng = R.Engine(p, 0)
    try:
        full, sc = eng.batch_encrypt(sk.key_lv0, plain, alpha, K, SEED, first_index, full=True, bodies=True)
        only_full = eng.batch_encrypt(sk.key_lv0, plain, alpha, K, SEED, first_index)
        only_bodies = eng.batch_encrypt(sk.key_lv0, plain, alpha, K, SEED, first_index, full=False, bodies=True)
        dev_full = _dev_encrypt(eng, sk.key_lv0, plain, alpha, first_index, True)
        dev_bodies = _dev_encrypt(eng, sk.key_lv0, plain, alpha, first_index, False)
        expanded = eng.expand_seeded(SeededCiphertexts(p, SEED, first_index, only_bodies.bodies))
    finally:
        eng.close()
    want, border = SM.bulk(sk.key_lv0, plain, first_index, alpha)
    _say(case="bulk", n=p.n, count=count, first_index=first_index, alpha=alpha, words=int(want.size),
         full_differing=int((full != want).sum()), bodies_differing=int((only_bodies.bodies != want[:, -1]).sum()),
         borderline=int(border.sum()))
    assert full.shape == want.shape == (count, p.n + 1)
    if alpha == 0.0:
        assert not border.any() and np.array_equal(full, want) and np.array_equal(only_bodies.bodies, want[:, -1])
    assert KM.compare_words(full, want, border, f"bulk full form n {p.n} count {count}")[0] <= KM.MAX_MISMATCHES
    assert KM.compare_words(only_bodies.bodies, want[:, -1], border[:, -1], f"bulk bodies n {p.n} count {count}")[0] \
        <= KM.MAX_MISMATCHES
    # one kernel, one answer: whichever outputs are asked for, host form or device form
    assert np.array_equal(only_full, full) and np.array_equal(sc.bodies, full[:, -1])
    assert np.array_equal(only_bodies.bodies, full[:, -1])
    assert np.array_equal(dev_full, full), "host form != _dev form"
    assert np.array_equal(dev_bodies, full[:, -1]), "host form != _dev form (bodies only)"
    assert np.array_equal(expanded, full), "expand_seeded_tlwe(S, first_index, bodies) != the full form"
    assert (sc.mask_seed, sc.first_index) == (SEED, first_index)
    if alpha > 0:
        assert np.abs(_phase_error(sk, full, plain)).max() < 6 * alpha


@pytest.mark.parametrize("first_index", SM.FIRST, ids=["first0", "firstHIGH"])
@pytest.mark.parametrize("count", SM.COUNTS)
@pytest.mark.parametrize("shape", SM.SHAPES, ids=lambda s: f"n{s[0]}")
def test_bulk_words_equal_the_model(shape, count, first_index):
    p = KM.shape_params(shape)
    _bulk_case(p, KM.secret_key(p), count, first_index, SM.ALPHA)


@pytest.mark.parametrize("shape", SM.SHAPES, ids=lambda s: f"n{s[0]}")
def test_bulk_zero_alpha_is_equality(shape):
    p = KM.shape_params(shape)
    _bulk_case(p, KM.secret_key(p), 257, SM.HIGH, 0.0)


@pytest.mark.parametrize("count,first_index", [(1, 0), (257, SM.HIGH)])
def test_bulk_second_block_pass(count, first_index):
    """SECURITY_UINT5, n = 1071: 67 mask blocks, so lanes 0..2 make a second block and lane 3 the noise"""
    import rs_tfhe_amd as R

    p = R.params.SECURITY_UINT5
    _bulk_case(p, SecretKey.new(p, 4000 + p.n), count, first_index, SM.ALPHA)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [SM.SHAPES[1], SM.SHAPES[0]], ids=lambda s: f"n{s[0]}")
def test_rows_land_at_any_word_of_a_chunk(shape, offset):
    """The row kernel stores a staged row in 16-byte chunks of its destination's alignment.  Rows written through a view
    that starts `offset` words into a larger tensor, by expand_seeded_dev and by batch_encrypt_dev (full rows, alpha 0:
    no noise, so equality), are the CPU form, and no word before the first row or after the last is touched."""
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd.seeded import SeededCiphertexts

    p = KM.shape_params(shape)
    sk = KM.secret_key(p)
    count, width = 17, p.n + 1
    plain = SM.plaintexts(count, p.n + offset)
    want, border = SM.bulk(sk.key_lv0, plain, SM.HIGH, 0.0)
    assert not border.any()
    sc = SeededCiphertexts(p, SEED, SM.HIGH, want[:, -1].copy())
    assert np.array_equal(sc.expand(), want)
    eng = R.Engine(p, 0)
    try:
        def through_view(call):
            big, view = DB.frame(want, offset, fill="sentinel")  # (the rows' shape; every word the sentinel)
            assert big.data_ptr() % 16 == 0 and DB.span(big, view) == (DB.PAD + offset, count * width)
            call(view)
            torch.cuda.synchronize()
            return big

        tb = torch.from_numpy(sc.bodies.view(np.int32)).cuda()
        tp = torch.from_numpy(np.ascontiguousarray(plain, np.uint32).view(np.int32)).cuda()
        got = {
            "expand_seeded_dev": through_view(lambda v: eng.expand_seeded_dev(SEED, SM.HIGH, tb, v)),
            "batch_encrypt_dev": through_view(lambda v: eng.batch_encrypt_dev(sk.key_lv0, tp, 0.0, SEED, K, SM.HIGH, out=v)),
        }
    finally:
        eng.close()
    for name, big in got.items():
        span = (DB.PAD + offset, count * width)
        rows = DB.view_words(big, span).reshape(count, width)
        _say(case="alignment", call=name, n=p.n, offset=offset, differing=int((rows != want).sum()))
        assert np.array_equal(rows, want), name
        g = DB.host_words(big).view(np.uint32)
        outside = np.concatenate([g[:span[0]], g[span[0] + span[1]:]])
        assert len(outside) == 2 * DB.PAD + offset and (outside == DB.SENTINEL).all(), f"{name} wrote outside its rows"
        assert DB.check_frame(big, span, "sentinel", name) == ""


def test_bulk_refusals():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi

    C = _capi.C
    p = KM.shape_params(SHAPE)
    sk = KM.secret_key(p)
    plain = SM.plaintexts(5, 1)
    eng = R.Engine(p, 0)
    try:
        lib, ctx = eng._lib, eng._ctx
        k0 = sk.key_lv0.ctypes.data_as(C.c_void_p)
        pl = plain.ctypes.data_as(C.c_void_p)
        out = np.zeros((5, p.n + 1), np.uint32)
        po = out.ctypes.data_as(C.c_void_p)
        seed = (C.c_uint8 * 32).from_buffer_copy(SEED)
        sd = C.addressof(seed)
        call = lib.tfhe_hip_batch_encrypt
        assert call(ctx, None, pl, 5, C.c_double(0.0), None, sd, 0, None, po) == _capi.EINVAL
        assert call(ctx, k0, None, 5, C.c_double(0.0), None, sd, 0, None, po) == _capi.EINVAL
        assert call(ctx, k0, pl, 5, C.c_double(0.0), None, None, 0, None, po) == _capi.EINVAL
        assert call(ctx, k0, pl, 5, C.c_double(0.0), None, sd, 0, None, None) == _capi.EINVAL
        assert call(ctx, k0, pl, 5, C.c_double(-1.0), None, sd, 0, None, po) == _capi.EINVAL
        assert call(ctx, k0, pl, 5, C.c_double(float("nan")), None, sd, 0, None, po) == _capi.EINVAL
        assert call(ctx, k0, pl, 5, C.c_double(0.0), None, sd, C.c_uint64((1 << 64) - 4), None, po) == _capi.EINVAL
        assert not out.any()
        assert call(ctx, k0, pl, 5, C.c_double(0.0), None, sd, C.c_uint64((1 << 64) - 5), None, po) == _capi.OK
        assert np.array_equal(out, SM.bulk(sk.key_lv0, plain, (1 << 64) - 5, 0.0)[0])
        assert call(ctx, k0, pl, 0, C.c_double(0.0), None, sd, 0, None, None) == _capi.OK
        assert eng.batch_encrypt(sk.key_lv0, np.zeros(0, np.uint32), 0.0, K, SEED).shape == (0, p.n + 1)
    finally:
        eng.close()


# ---- 2. the public key ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 66, 8192])
def test_public_key_equals_the_model_and_loads_the_same(size):
    import rs_tfhe_amd as R

    p = KM.shape_params(SHAPE)
    sk = KM.secret_key(p)
    plain = SM.plaintexts(40, size)
    gen, other = R.Engine(p, 0), R.Engine(p, 0)
    try:
        assert not gen.public_key_is_loaded()
        enc = gen.gen_public_key(sk.key_lv0, size, SM.ALPHA, K)
        assert gen.public_key_is_loaded()
        on_gen = gen.batch_pk_encrypt(plain, 0.0, K, 3)
        other.load_public_key(enc)
        on_other = other.batch_pk_encrypt(plain, 0.0, K, 3)
        assert other.gen_public_key(sk.key_lv0, size, SM.ALPHA, K, download=False) is None
        on_quiet = other.batch_pk_encrypt(plain, 0.0, K, 3)
    finally:
        gen.close()
        other.close()
    want, border = SM.public_key(sk.key_lv0, size, SM.ALPHA)
    _say(case="public key", size=size, words=int(want.size), words_differing=int((enc != want).sum()),
         borderline=int(border.sum()), loaded_equal=bool(np.array_equal(on_gen, on_other)))
    assert KM.compare_words(enc, want, border, f"public key size {size}")[0] <= KM.MAX_MISMATCHES
    assert np.abs(_phase_error(sk, enc, 0)).max() < 6 * SM.ALPHA
    assert np.array_equal(on_gen, on_other), "the generating handle holds another public key than encryptions_out"
    assert np.array_equal(on_gen, on_quiet), "encryptions_out = NULL left another key on the handle"


def test_public_key_refusals_leave_the_previous_key():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi

    p = KM.shape_params(SHAPE)
    sk = KM.secret_key(p)
    plain = SM.plaintexts(9, 2)
    eng = R.Engine(p, 0)
    try:
        eng.gen_public_key(sk.key_lv0, 66, SM.ALPHA, K, download=False)
        before = eng.batch_pk_encrypt(plain, 0.0, K, 0)
        for bad in (0, 8193):
            with pytest.raises(_capi.TfheHipError) as err:
                eng.gen_public_key(sk.key_lv0, bad, SM.ALPHA, K, download=False)
            assert err.value.code == _capi.EINVAL
            assert eng.public_key_is_loaded() and np.array_equal(eng.batch_pk_encrypt(plain, 0.0, K, 0), before)
        for bad in (-1.0, float("nan")):
            with pytest.raises(_capi.TfheHipError) as err:
                eng.gen_public_key(sk.key_lv0, 66, bad, K)
            assert err.value.code == _capi.EINVAL
        assert eng._lib.tfhe_hip_gen_public_key(eng._ctx, None, 66, _capi.C.c_double(0.0), None, None) == _capi.EINVAL
        assert eng.public_key_is_loaded() and np.array_equal(eng.batch_pk_encrypt(plain, 0.0, K, 0), before)
    finally:
        eng.close()


# ---- 3. the symmetric re-encryption key -----------------------------------------------------------------------------
def test_symmetric_key_equals_the_model_and_loads_the_same():
    import rs_tfhe_amd as R

    p = KM.shape_params(SHAPE)
    alice, bob = SecretKey.new(p, 77), SecretKey.new(p, 78)
    ca = alice.encrypt_bool(np.random.default_rng(5).integers(0, 2, 70).astype(bool), 80)
    gen, quiet = R.Engine(p, 0), R.Engine(p, 0)
    try:
        key = gen.gen_reenc_key_symmetric(alice.key_lv0, bob.key_lv0, rng_key=K)
        assert gen.reenc_key_is_loaded()
        on_gen = gen.batch_reencrypt(ca)
        other = gen.new_key_view()
        other.load_reenc_key(key)
        on_other = other.batch_reencrypt(ca)
        other.close()
        assert quiet.gen_reenc_key_symmetric(alice.key_lv0, bob.key_lv0, rng_key=K, download=False) is None
        on_quiet = quiet.batch_reencrypt(ca)
    finally:
        gen.close()
        quiet.close()
    want, border = SM.reenc_key(p, alice.key_lv0, bob.key_lv0, p.alpha_lv0)
    _say(case="symmetric key", words=int(want.size), words_differing=int((key != want).sum()), borderline=int(border.sum()),
         loaded_equal=bool(np.array_equal(on_gen, on_other)), no_download_equal=bool(np.array_equal(on_gen, on_quiet)))
    shaped = key.reshape(p.n, p.iks_t, p.base, p.n + 1)
    assert not shaped[:, :, 0, :].any(), "a k = 0 row is not zero"
    assert KM.compare_words(key, want, border, "symmetric key")[0] <= KM.MAX_MISMATCHES
    assert np.array_equal(on_gen, on_other), "the generating handle holds another key than key_out"
    assert np.array_equal(on_gen, on_quiet), "key_out = NULL left another key on the handle"


def test_symmetric_key_refusals_leave_the_keys():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi
    from rs_tfhe_amd.engine import NAND

    p = KM.shape_params(SHAPE)
    alice, bob = SecretKey.new(p, 77), SecretKey.new(p, 78)
    ca = alice.encrypt_bool([1, 0, 1, 1], 81)
    eng = R.Engine(p, 0)
    try:
        eng.gen_reenc_key_symmetric(alice.key_lv0, bob.key_lv0, rng_key=K, download=False)
        before = eng.batch_reencrypt(ca)
        for bad in (-1.0, float("nan")):
            with pytest.raises(_capi.TfheHipError) as err:
                eng.gen_reenc_key_symmetric(alice.key_lv0, bob.key_lv0, alpha=bad, rng_key=K)
            assert err.value.code == _capi.EINVAL
        k0 = alice.key_lv0.ctypes.data_as(_capi.C.c_void_p)
        call = eng._lib.tfhe_hip_gen_reenc_key_symmetric
        assert call(eng._ctx, None, k0, _capi.C.c_double(0.0), None, None) == _capi.EINVAL
        assert call(eng._ctx, k0, None, _capi.C.c_double(0.0), None, None) == _capi.EINVAL
        assert eng.reenc_key_is_loaded() and np.array_equal(eng.batch_reencrypt(ca), before)
    finally:
        eng.close()
    # n > 1024: refused with the message load gives, and the cloud key on the handle bootstraps as before
    pb = KM.shape_params(KM.SHAPES[3])
    sb = KM.secret_key(pb)
    a, b = sb.encrypt_bool([1, 1, 0, 0], 82), sb.encrypt_bool([1, 0, 1, 0], 83)
    big = R.Engine(pb, 0)
    try:
        big.gen_cloud_key(sb.key_lv0, sb.key_lv1, seed=5)
        before = big.batch_gate(NAND, a, b)
        with pytest.raises(_capi.TfheHipError, match="n <= N") as err:
            big.gen_reenc_key_symmetric(sb.key_lv0, sb.key_lv0, rng_key=K)
        assert err.value.code == _capi.EINVAL
        assert not big.reenc_key_is_loaded()
        assert np.array_equal(big.batch_gate(NAND, a, b), before), "the cloud key no longer bootstraps as it did"
    finally:
        big.close()


# ---- 4. statistics of the OS-keyed route ----------------------------------------------------------------------------
def test_os_keyed_noise_statistics():
    """262,144 rows at n = 16, alpha 2e-5, rng_key = NULL: the noise recovered with the secret key alone sits within
    6 SE of numpy's own normal(0, alpha) on every statistic of KM.noise_report (the OS-keyed bar of DESIGN 11.3), and two
    calls share no noise: two independent samples at sigma = 85,899 torus steps are the same word with probability
    1 / (2 sqrt(pi) sigma) = 3.3e-6, 0.86 rows of the 262,144 by chance, so more than 8 equal words (a 1e-6 event) is a
    repeated stream."""
    import rs_tfhe_amd as R

    p = KM.shape_params(SM.SHAPES[1])
    sk = KM.secret_key(p)
    count = 262144
    plain = SM.plaintexts(count, 3)
    eng = R.Engine(p, 0)
    try:
        first, second = (eng.batch_encrypt(sk.key_lv0, plain, SM.ALPHA, None, SEED, 0) for _ in range(2))
    finally:
        eng.close()
    e1, e2 = (sk.phase(c) - plain for c in (first, second))
    rep = KM.noise_report(e1.view(np.int32), SM.ALPHA, KM.REF_SEED, mask=first[:, 0])
    shared = int((e1 == e2).sum())
    _say(case="os-keyed statistics", M=count, worst=KM.worst(rep), shared_noise_words=shared,
         **{k: rep[k] for k in KM.STATISTICS if k in rep})
    assert np.array_equal(first[:, :-1], second[:, :-1])  # (one S, one index range: the same masks)
    KM.check_report(rep, 6.0, "OS-keyed bulk noise")
    assert shared <= 8, "two OS-keyed calls share their noise"


# ---- 5. end to end --------------------------------------------------------------------------------------------------
def test_end_to_end_at_security_128_bit(O):
    import rs_tfhe_amd as R
    from conftest import oracle_keys
    from rs_tfhe_amd import proxy_reenc as PR

    p = R.params.SECURITY_128_BIT
    osk, ock = oracle_keys(O, O.SECURITY_128_BIT, with_time=True)
    sk = SecretKey(p, osk.key_lv0, osk.key_lv1)
    ck = R.CloudKey(p, ock.bootstrapping_key, ock.key_switching_key, ock.decomposition_offset, ock.blind_rotate_testvec)
    rng = np.random.default_rng(14)
    A, B = rng.integers(0, 2, 1024).astype(bool), rng.integers(0, 2, 1024).astype(bool)
    # encrypt on the device, NAND under the cloud key, decrypt
    ca, cb = sk.encrypt_bool(A, device=0), sk.encrypt_bool(B, device=0)
    sb = sk.encrypt_bool_seeded(B, device=0)
    out = R.gates.batch_nand(ca, cb, ck)
    nand_ok = int((sk.decrypt_bool(out) == ~(A & B)).sum())
    seeded_ok = int((sk.decrypt_bool(sb.expand()) == B).sum())
    # the public key made on the device encrypts
    pk = PR.PublicKeyLv0.new(sk, device=0)
    assert pk._view is not None and pk._view[1].public_key_is_loaded()  # generated in place: nothing to upload
    pk_ok = int((sk.decrypt_bool(pk.encrypt_bool(A, p.alpha_lv0, device=0)) == A).sum())
    pk.close()
    # the symmetric key made on the device re-encrypts
    bob = SecretKey.new(p, 78)
    with PR.ProxyReencryptionKey.new_symmetric(sk, bob, device=0) as rk:
        assert rk._view is not None and rk._view[1].reenc_key_is_loaded()
        re = rk.reencrypt(ca)
        zero_rows = not rk.key_encryptions.reshape(p.n, p.iks_t, p.base, p.n + 1)[:, :, 0, :].any()
    rate = float((bob.decrypt_bool(re) == A).mean())
    _say(case="end to end", nand_correct=nand_ok, seeded_correct=seeded_ok, pk_correct=pk_ok, reencrypt_rate=rate)
    assert nand_ok == 1024 and seeded_ok == 1024 and pk_ok == 1024
    assert zero_rows and rate > 0.90


# ---- 6. C++ ---------------------------------------------------------------------------------------------------------
def test_cpp_encrypts_and_generates_the_same_words(tmp_path):
    """encrypt_batch, PublicKeyLv0::generate and generate_symmetric under the fixed K: the checksums the program prints
    are the Python route's."""
    import rs_tfhe_amd as R

    p = KM.shape_params(SHAPE)
    alice, bob = SecretKey.new(p, 77), SecretKey.new(p, 78)
    count, first_index, size = 70, 9, 66
    plain = f64_to_torus(np.where(np.arange(count) % 3 == 0, 0.125, -0.125))
    eng = R.Engine(p, 0)
    try:
        enc = eng.batch_encrypt(alice.key_lv0, plain, p.alpha_lv0, K, SEED, first_index)
        pk = eng.gen_public_key(bob.key_lv0, size, p.alpha_lv0, K)
        key = eng.gen_reenc_key_symmetric(alice.key_lv0, bob.key_lv0, rng_key=K)
        re = eng.batch_reencrypt(enc)
    finally:
        eng.close()
    blob = tmp_path / "in.bin"
    blob.write_bytes(K + SEED + np.ascontiguousarray(alice.key_lv0, "<u4").tobytes() + np.ascontiguousarray(bob.key_lv0, "<u4").tobytes())
    exe = build_cpp_sym_encrypt(str(tmp_path))
    args = [str(v) for v in SHAPE] + [repr(p.alpha_lv0), str(size), str(count), str(first_index), str(blob)]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    _say(case="c++", returncode=r.returncode, stdout=r.stdout.strip().splitlines())
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(ln.split(" ", 1) for ln in r.stdout.strip().splitlines())
    assert int(lines["enc_checksum"]) == SM.PM.checksum(enc)
    assert int(lines["pk_checksum"]) == SM.PM.checksum(pk)
    assert int(lines["key_checksum"]) == SM.PM.checksum(key)
    assert int(lines["reenc_checksum"]) == SM.PM.checksum(re)
