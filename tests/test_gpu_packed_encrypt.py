"""Packed TRLWE encryption on the GPU (csrc/trlwe_encrypt.hpp: k_trlwe_rows / k_expand_trlwe behind
tfhe_hip_batch_encrypt_trlwe[_dev] / tfhe_hip_expand_seeded_trlwe[_dev]) held to the term-by-term CPU model of
tests/packed_encrypt_model.py.

Under a fixed generator key every mask word and every noise sample is a keystream position the model knows: at
alpha = 0 the words must be EQUAL; with noise a body word may differ from the model's by exactly +-1 LSB only where the
long-double sampler marks its sample borderline, at most 16 words a call (KM.compare_words; the cap on the inputs is
checked on the CPU by tests/test_packed_encrypt_host.py).  The sizes are the smallest at which the kernel can go wrong:
one slot, one short of a group, a whole group, one over, several groups with a ragged last one, and 65 groups; a first
group above 2^32 whose batch crosses a carry of the low nonce word; plaintexts with 0xFFFFFFFF / 0x80000000 at every
group's first and last slot.  A wave of k_trlwe_rows takes one group whatever the grid, so no case is sized from it.
The model could share a mistake with the kernel; the statistics of noise recovered with the secret key alone, and
decryption, could not.

Every test prints its figures (`PACKEDENCRYPT {json}` lines; run with -s) before it asserts."""
import functools
import json
import subprocess

import numpy as np
import pytest

import keygen_model as KM
import packed_encrypt_model as PM
from test_packed_encrypt_host import build_cpp_packed_encrypt
from rs_tfhe_amd.client import SecretKey, f64_to_torus
from rs_tfhe_amd.params import N

pytestmark = pytest.mark.gpu

K, SEED = PM.K, PM.SEED
P = KM.shape_params(KM.SHAPES[2])  # the calls read key_lv1 only and need no key on the handle: a small set serves


def _say(**kv):
    print("PACKEDENCRYPT " + json.dumps(kv, default=float))


@functools.lru_cache(maxsize=None)
def _model(key, count, first_group, alpha):
    """(plain, words, border) of one case, computed once and shared (read-only)"""
    plain = PM.plaintexts(count, count % 97)
    want, border = PM.encrypt(PM.keys()[key], plain, count, first_group, alpha)
    for a in (plain, want, border):
        a.setflags(write=False)
    return plain, want, border


def _t(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint32).view(np.int32)).to("cuda:0")  # (a copy: the shared cases are read-only)


def _dev_encrypt(eng, key_lv1, plain, alpha, first_group, full, rng_key=K):
    """batch_encrypt_trlwe_dev on a stream of the caller's, back on the host: [groups][2][N] (full) or the bodies"""
    import torch

    groups = PM.groups_of(len(plain))
    tp = _t(plain)
    out = torch.full((groups, 2, N), -1, dtype=torch.int32, device="cuda:0") if full else None
    bod = None if full else torch.full((groups, N), -1, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream(0)
    s.wait_stream(torch.cuda.current_stream(0))
    with torch.cuda.stream(s):
        eng.batch_encrypt_trlwe_dev(key_lv1, tp, alpha, SEED, rng_key, first_group, bodies=bod, out=out, stream=s)
    s.synchronize()
    return (out if full else bod).cpu().numpy().view(np.uint32)


def _case(key, count, first_group, alpha):
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd.seeded import SeededPackedCiphertexts

    s1 = PM.keys()[key]
    plain, want, border = _model(key, count, first_group, alpha)
    groups = PM.groups_of(count)
    eng = R.Engine(P, 0)
    try:
        full, sc = eng.batch_encrypt_trlwe(s1, plain, alpha, K, SEED, first_group, full=True, bodies=True)
        only_full = eng.batch_encrypt_trlwe(s1, plain, alpha, K, SEED, first_group)
        only_bodies = eng.batch_encrypt_trlwe(s1, plain, alpha, K, SEED, first_group, full=False, bodies=True)
        dev_full = _dev_encrypt(eng, s1, plain, alpha, first_group, True)
        dev_bodies = _dev_encrypt(eng, s1, plain, alpha, first_group, False)
        expanded = eng.expand_seeded_trlwe(only_bodies)
        tout = torch.full((groups, 2, N), -1, dtype=torch.int32, device="cuda:0")
        side = torch.cuda.Stream(0)
        tb = _t(only_bodies.bodies)
        side.wait_stream(torch.cuda.current_stream(0))
        eng.expand_seeded_trlwe_dev(SEED, first_group, tb, tout, stream=side)
        side.synchronize()
        dev_expanded = tout.cpu().numpy().view(np.uint32)
    finally:
        eng.close()
    _say(case="bulk", key=key, count=count, first_group=first_group, alpha=alpha, words=int(want.size),
         full_differing=int((full != want).sum()), bodies_differing=int((only_bodies.bodies != want[:, 1]).sum()),
         borderline=int(border.sum()))
    assert full.shape == want.shape == (groups, 2, N)
    if alpha == 0.0:
        assert not border.any() and np.array_equal(full, want) and np.array_equal(only_bodies.bodies, want[:, 1])
    assert KM.compare_words(full, want, border, f"full form {key} count {count}")[0] <= KM.MAX_MISMATCHES
    assert KM.compare_words(only_bodies.bodies, want[:, 1], border[:, 1], f"bodies {key} count {count}")[0] <= KM.MAX_MISMATCHES
    # one kernel, one answer: whichever outputs are asked for, host form or device form
    assert np.array_equal(only_full, full) and np.array_equal(sc.bodies, full[:, 1])
    assert np.array_equal(only_bodies.bodies, full[:, 1]), "the bodies-only output is not the B half of the full form"
    assert np.array_equal(dev_full, full), "host form != _dev form"
    assert np.array_equal(dev_bodies, full[:, 1]), "host form != _dev form (bodies only)"
    assert np.array_equal(expanded, full), "expand_seeded_trlwe(S, first_group, bodies) != the full form"
    assert np.array_equal(dev_expanded, full), "expand_seeded_trlwe_dev != the full form"
    assert np.array_equal(SeededPackedCiphertexts(P, SEED, first_group, only_bodies.bodies, count).expand(), full)
    assert (sc.mask_seed, sc.first_group, sc.count) == (SEED, first_group, count)
    # every slot decrypts; the unused slots of the last group hold noise only (exactly 0 at alpha = 0)
    e, _ = PM.recover_noise(s1, full, plain, count)
    assert np.abs(e).max() <= 6 * alpha * 2.0 ** 32
    sk = SecretKey(P, np.zeros(P.n, np.uint32), s1)
    unused = sk.packed_phase(full, groups * N)[count:].view(np.int32)
    assert np.array_equal(unused, e.reshape(-1)[count:]) and np.abs(unused).max(initial=0) <= 6 * alpha * 2.0 ** 32


@pytest.mark.parametrize("first_group", PM.FIRST, ids=["first0", "firstHIGH"])
@pytest.mark.parametrize("count", PM.COUNTS)
def test_words_equal_the_model(count, first_group):
    _case("random", count, first_group, PM.ALPHA)


@pytest.mark.parametrize("key", ["ones", "zeros", "last"])
def test_edge_keys(key):
    _case(key, 3 * N + 5, PM.HIGH, PM.ALPHA)


@pytest.mark.parametrize("key", ["random", "ones"])
def test_zero_alpha_is_equality(key):
    _case(key, 3 * N + 5, PM.HIGH, 0.0)


def test_error_codes():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi

    C = _capi.C
    s1 = PM.keys()["random"]
    plain = PM.plaintexts(N + 5, 1)
    eng = R.Engine(P, 0)
    try:
        lib, ctx = eng._lib, eng._ctx
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        out, bod = np.zeros((2, 2, N), np.uint32), np.zeros((2, N), np.uint32)
        seed = (C.c_uint8 * 32).from_buffer_copy(SEED)
        sd, z, cnt = C.addressof(seed), C.c_double(0.0), N + 5
        host = lambda *a: lib.tfhe_hip_batch_encrypt_trlwe(ctx, *a)  # noqa: E731
        dev = lambda *a: lib.tfhe_hip_batch_encrypt_trlwe_dev(ctx, *a, None)  # noqa: E731
        for call in (host, dev):  # (every refusal comes before a pointer is followed on the device: host arrays serve both)
            assert call(None, ptr(plain), cnt, z, None, sd, 0, None, ptr(out)) == _capi.EINVAL
            assert call(ptr(s1), None, cnt, z, None, sd, 0, None, ptr(out)) == _capi.EINVAL
            assert call(ptr(s1), ptr(plain), cnt, z, None, None, 0, None, ptr(out)) == _capi.EINVAL
            assert call(ptr(s1), ptr(plain), cnt, z, None, sd, 0, None, None) == _capi.EINVAL
            assert b"no output" in lib.tfhe_hip_last_error(ctx)
            assert call(ptr(s1), ptr(plain), cnt, C.c_double(-1.0), None, sd, 0, None, ptr(out)) == _capi.EINVAL
            assert call(ptr(s1), ptr(plain), cnt, C.c_double(float("nan")), None, sd, 0, None, ptr(out)) == _capi.EINVAL
            bad = s1.copy()
            bad[N - 1] = 2
            assert call(ptr(bad), ptr(plain), cnt, z, None, sd, 0, None, ptr(out)) == _capi.EINVAL
            assert b"binary" in lib.tfhe_hip_last_error(ctx)
            assert call(ptr(s1), ptr(plain), 1 << 31, z, None, sd, 0, None, ptr(out)) == _capi.EINVAL
            assert call(ptr(s1), ptr(plain), cnt, z, None, sd, C.c_uint64((1 << 64) - 1), None, ptr(out)) == _capi.EINVAL
            assert call(ptr(s1), ptr(plain), 0, z, None, sd, 0, None, None) == _capi.OK
        assert not out.any() and not bod.any()
        # the last two groups of the index space are not past it
        assert host(ptr(s1), ptr(plain), cnt, z, None, sd, C.c_uint64((1 << 64) - 2), ptr(bod), ptr(out)) == _capi.OK
        want = PM.encrypt(s1, plain, cnt, (1 << 64) - 2, 0.0)[0]
        assert np.array_equal(out, want) and np.array_equal(bod, want[:, 1])
        assert eng.batch_encrypt_trlwe(s1, np.zeros(0, np.uint32), 0.0, K, SEED).shape == (0, 2, N)
        xhost = lambda *a: lib.tfhe_hip_expand_seeded_trlwe(ctx, *a)  # noqa: E731
        xdev = lambda *a: lib.tfhe_hip_expand_seeded_trlwe_dev(ctx, *a, None)  # noqa: E731
        out2 = np.zeros((2, 2, N), np.uint32)
        for call in (xhost, xdev):
            assert call(None, 0, ptr(bod), 2, ptr(out2)) == _capi.EINVAL
            assert call(sd, 0, None, 2, ptr(out2)) == _capi.EINVAL
            assert call(sd, 0, ptr(bod), 2, None) == _capi.EINVAL
            assert call(sd, C.c_uint64((1 << 64) - 1), ptr(bod), 2, ptr(out2)) == _capi.EINVAL
            assert call(sd, 0, ptr(bod), 1 << 31, ptr(out2)) == _capi.EINVAL
            assert call(sd, 0, ptr(bod), 0, ptr(out2)) == _capi.OK
        assert not out2.any()
        assert xhost(sd, C.c_uint64((1 << 64) - 2), ptr(bod), 2, ptr(out2)) == _capi.OK and np.array_equal(out2, want)
        # _dev: pointers off a 16-byte boundary are refused before anything is queued
        import torch

        tp, big = _t(plain), torch.zeros(2 * 2 * N + 4, dtype=torch.int32, device="cuda:0")
        off = C.c_void_p(big.data_ptr() + 4)
        assert dev(ptr(s1), C.c_void_p(tp.data_ptr()), cnt, z, None, sd, 0, None, off) == _capi.EINVAL
        assert dev(ptr(s1), C.c_void_p(tp.data_ptr()), cnt, z, None, sd, 0, off, None) == _capi.EINVAL
        assert xdev(sd, 0, off, 1, C.c_void_p(big.data_ptr())) == _capi.EINVAL
        torch.cuda.synchronize()
        assert not big.any().item()
    finally:
        eng.close()


def _stats(e, a, alpha, bound, label):
    rep = KM.noise_report(e, alpha, KM.REF_SEED, mask=a)
    _say(case=label, M=int(e.size), worst=KM.worst(rep), **{k: rep[k] for k in KM.STATISTICS if k in rep})
    KM.check_report(rep, bound, label)


def test_noise_statistics_os_keyed_and_fixed_key():
    """256 groups (262,144 samples) at alpha_lv1, rng_key = NULL: the noise recovered with the secret key alone sits
    within 6 SE of numpy's own normal(0, alpha) on every statistic of KM.noise_report (the OS-keyed bar of DESIGN 11.3);
    under the fixed K within 5 SE."""
    import rs_tfhe_amd as R

    s1 = PM.keys()["random"]
    count = 256 * N
    plain = PM.plaintexts(count, 5)
    eng = R.Engine(P, 0)
    try:
        os_keyed = eng.batch_encrypt_trlwe(s1, plain, PM.ALPHA, None, SEED, 7)
        fixed = eng.batch_encrypt_trlwe(s1, plain, PM.ALPHA, K, SEED, 7)
    finally:
        eng.close()
    assert np.array_equal(os_keyed[:, 0], fixed[:, 0])  # (one S, one index range: the same masks)
    e_os, a = PM.recover_noise(s1, os_keyed, plain, count)
    e_fixed, _ = PM.recover_noise(s1, fixed, plain, count)
    _stats(e_os, a, PM.ALPHA, 6.0, "OS-keyed packed noise")
    _stats(e_fixed, a, PM.ALPHA, 5.0, "fixed-key packed noise")


def test_two_os_keyed_calls_share_no_row():
    """encrypt_packed_f64(device=0) twice: a fresh S and a fresh K each, so no mask polynomial and no noise polynomial is
    common to the two (any pair of groups, not only the same index)"""
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    sk = SecretKey(p, np.zeros(p.n, np.uint32), PM.keys()["random"])
    pt = np.random.default_rng(3).uniform(-0.5, 0.5, 8 * N)
    first, second = (sk.encrypt_packed_f64(pt, device=0) for _ in range(2))
    noise = [PM.recover_noise(sk.key_lv1, c, f64_to_torus(pt), len(pt))[0] for c in (first, second)]
    masks = np.concatenate([first[:, 0], second[:, 0]])
    rows = np.concatenate(noise)
    _say(case="two OS-keyed calls", distinct_masks=len(np.unique(masks, axis=0)), distinct_noise=len(np.unique(rows, axis=0)))
    assert len(np.unique(masks, axis=0)) == 16 and len(np.unique(rows, axis=0)) == 16
    # ... and not one word of noise in common beyond chance: two samples at sigma = 86 steps are equal with probability
    # 1 / (2 sqrt(pi) sigma) = 3.3e-3, 27 of the 8,192 by chance (sd 5.2): 80 is ten sd out
    assert int((noise[0] == noise[1]).sum()) < 80
    assert np.abs(noise[0]).max() < 6 * p.alpha_lv1 * 2.0 ** 32


def test_end_to_end_at_security_128_bit():
    """encrypt_packed_bool(device=0) -> unpack -> batch_nand -> pack -> decrypt_packed_bool(device=0) gives the truth table;
    encrypt_packed_lwe_message(device=0) -> batch_trlwe_matmul -> decrypt_lwe_message equals the plain product mod m."""
    import os

    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.bootstrap import keyed_engine
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    sk = SecretKey.new(p, 91)
    ck = sk.cloud_key(seed=92, device=0)
    pk = sk.packing_key(rng_key=os.urandom(32), device=0)
    rng = np.random.default_rng(93)
    va, vb = rng.integers(0, 2, 1500).astype(bool), rng.integers(0, 2, 1500).astype(bool)
    pa, pb = sk.encrypt_packed_bool(va, device=0), sk.encrypt_packed_bool(vb, device=0, first_group=2)
    assert pa.shape == (2, 2, N)
    a, b = PK.unpack(pa, ck, len(va)), PK.unpack(pb, ck, len(vb))
    out = R.gates.batch_nand(a, b, ck)
    got = sk.decrypt_packed_bool(PK.pack(out, ck, pk), len(va), device=0)
    nand_ok = int((got == ~(va & vb)).sum())
    seeded_ok = int((sk.decrypt_packed_bool(sk.encrypt_packed_bool_seeded(vb, device=0).expand(), len(vb)) == vb).sum())
    # a 5 x 24 int8 layer over the first 24 slots of 3 groups of messages mod 4
    m, cols = 4, 24
    msgs = rng.integers(0, m, 2 * N + cols)
    w = rng.integers(-3, 4, (5, cols)).astype(np.int8)
    pm = sk.encrypt_packed_lwe_message(msgs, m, device=0)
    with keyed_engine(ck, 0) as eng:
        rows = eng.batch_trlwe_matmul(w, pm, keyswitch=True)
    assert rows.shape == (3, 5, p.n + 1)
    want = (w.astype(np.int64) @ np.stack([msgs[g * N:g * N + cols] for g in range(3)]).T).T % m  # [groups][rows]
    dec = sk.decrypt_lwe_message(rows.reshape(-1, p.n + 1), m).reshape(3, 5)
    _say(case="end to end", nand_correct=nand_ok, seeded_correct=seeded_ok, matmul_correct=int((dec == want).sum()))
    assert nand_ok == 1500 and seeded_ok == 1500
    assert np.array_equal(dec, want)


def test_cpp_encrypts_the_same_words(tmp_path):
    """encrypt_packed_batch and expand_seeded_packed under the fixed K: the checksums the program prints are the Python
    route's."""
    import packing_keygen_model as PKM
    import rs_tfhe_amd as R

    s1 = PM.keys()["random"]
    count, first_group = 2 * N + 70, PM.HIGH
    plain = f64_to_torus(np.where(np.arange(count) % 3 == 0, 0.125, -0.125))
    eng = R.Engine(P, 0)
    try:
        enc = eng.batch_encrypt_trlwe(s1, plain, P.alpha_lv1, K, SEED, first_group)
    finally:
        eng.close()
    blob = tmp_path / "in.bin"
    blob.write_bytes(K + SEED + np.ascontiguousarray(s1, "<u4").tobytes())
    exe = build_cpp_packed_encrypt(str(tmp_path))
    args = [str(v) for v in KM.SHAPES[2]] + [repr(P.alpha_lv1), str(count), str(first_group), str(blob)]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    _say(case="c++", returncode=r.returncode, stdout=r.stdout.strip().splitlines())
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(ln.split(" ", 1) for ln in r.stdout.strip().splitlines())
    assert int(lines["enc_checksum"]) == PKM.checksum(enc)
    assert int(lines["bodies_checksum"]) == PKM.checksum(enc[:, 1])
