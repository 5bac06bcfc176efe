"""The packing key generated on the GPU (csrc/packing_keygen.hpp: k_gen_packing_key behind tfhe_hip_gen_packing_key) held
to the CPU model of tests/packing_keygen_model.py, sample for sample, and to what it is for.

Under a fixed generator key every mask word and every Gaussian sample is a keystream position the model knows: the mask
seed must be the model's, and a body may differ from the model's by exactly +-1 LSB only where the long-double sampler
marks its noise sample borderline, at most 16 words a key (KM.compare_words).  The handle must hold the key its outputs
describe: packing on the generating handle, on a handle that loaded (S, bodies) and in packing.pack_model give the same
words.  The model could share a mistake with the kernel; the statistics could not: they recover the noise with the secret
key alone and hold it to numpy's normal(0, alpha) in standard errors (5 SE under the fixed key, 6 SE OS-keyed; DESIGN
section 11.3).

Every test prints its figures (`PACKKEYGEN {json}` lines; run with -s) before it asserts."""
import json
import subprocess

import numpy as np
import pytest

import keygen_model as KM
import packing_keygen_model as PM
from test_packing_keygen_host import build_cpp_packing_keygen
from rs_tfhe_amd.params import N

pytestmark = pytest.mark.gpu

K = KM.GEN_KEY
ALPHA = KM.ALPHA_BSK  # 2e-8
_MODELS, _KEYS = {}, {}


def _say(**kv):
    print("PACKKEYGEN " + json.dumps(kv, default=float))


def _params(shape, alpha=ALPHA):
    return KM.shape_params(shape, alpha_bsk=alpha)


def _model(shape, alpha=ALPHA):
    if (shape, alpha) not in _MODELS:
        p = _params(shape, alpha)
        sk = KM.secret_key(p)
        _MODELS[(shape, alpha)] = PM.model(p, sk.key_lv0, sk.key_lv1, K, alpha)
    return _MODELS[(shape, alpha)]


def _generate(shape, alpha=ALPHA, rng_key=K):
    """packing.PackingKey that Engine.gen_packing_key returns on a fresh context (kept for the fixed generator key)"""
    import rs_tfhe_amd as R

    if rng_key is not None and (shape, alpha) in _KEYS:
        return _KEYS[(shape, alpha)]
    p = _params(shape, alpha)
    sk = KM.secret_key(p)
    eng = R.Engine(p, 0)
    try:
        pk = eng.gen_packing_key(sk.key_lv0, sk.key_lv1, rng_key=rng_key, alpha=alpha)
        assert eng.packing_key_is_loaded() and eng._packing_key is pk
    finally:
        eng.close()
    if rng_key is not None:
        _KEYS[(shape, alpha)] = pk
    return pk


_ids = lambda v: str(v).replace(" ", "")  # noqa: E731
WORD_CASES = [(s, ALPHA) for s in PM.SHAPES] + [(KM.SHAPES[2], KM.ALPHA_BSK_UINT), (KM.SHAPES[0], 0.5)]


# ---- 1. every word against the model --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,alpha", WORD_CASES, ids=_ids)
def test_every_word_equals_the_model(shape, alpha):
    """The mask seed and every body word of k_gen_packing_key.  At alpha = 2.2e-16 the noise truncates to zero in any
    arithmetic, so the comparison is plain equality; at alpha = 0.5 |g| > 1 occurs and fmod folds it (56 borderline
    samples in the model there; the cap of 16 differing words is compare_words' own)."""
    pk = _generate(shape, alpha)
    m = _model(shape, alpha)
    border = int(m.border.sum())
    differ = int((pk.bodies != m.bodies).sum())
    _say(case="words", shape=list(shape), alpha=alpha, words=int(m.bodies.size), words_differing=differ, borderline=border,
         seed_equal=pk.mask_seed == m.mask_seed)
    assert pk.mask_seed == m.mask_seed == PM.mask_seed(K)
    assert pk.bodies.shape == m.bodies.shape
    if alpha == KM.ALPHA_BSK_UINT:
        assert not m.e.words.any() and border == 0
        assert np.array_equal(pk.bodies, m.bodies)
    else:
        assert m.e.words.any()
        if alpha == ALPHA:
            assert border <= KM.MAX_MISMATCHES
    mism, _ = KM.compare_words(pk.bodies, m.bodies, m.border, f"packing key {shape} alpha {alpha}")
    assert mism <= KM.MAX_MISMATCHES


# ---- 2. the handle holds what the outputs describe ------------------------------------------------------------------
def test_the_handle_holds_the_key_its_outputs_describe():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi, packing as PK

    shape = KM.SHAPES[0]
    p = _params(shape)
    sk = KM.secret_key(p)
    cts = np.random.default_rng(77).integers(0, 1 << 32, (70, p.n + 1), dtype=np.uint64).astype(np.uint32)
    gen, other, quiet = R.Engine(p, 0), R.Engine(p, 0), R.Engine(p, 0)
    try:
        gen.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=5)
        assert gen._lib.tfhe_hip_key_is_loaded(gen._ctx) == 1 and not gen.packing_key_is_loaded()
        pk = gen.gen_packing_key(sk.key_lv0, sk.key_lv1, rng_key=K, alpha=ALPHA)
        assert gen._lib.tfhe_hip_key_is_loaded(gen._ctx) == 1, "generating the packing key dropped the cloud key"
        ones = gen.batch_gate(R.engine.NAND, sk.encrypt_bool([1, 0, 1], 3), sk.encrypt_bool([1, 1, 0], 4))
        assert list(sk.decrypt_bool(ones)) == [False, True, True]
        on_gen = gen.pack(cts)
        other.load_packing_key(pk)
        on_other = other.pack(cts)
        want = PK.pack_model(p, pk.mask_seed, pk.bodies, cts)
        assert quiet.gen_packing_key(sk.key_lv0, sk.key_lv1, rng_key=K, alpha=ALPHA, download=False) is None
        on_quiet = quiet.pack(cts)
        _say(case="handle", generating_equals_model=bool(np.array_equal(on_gen, want)),
             loaded_equals_model=bool(np.array_equal(on_other, want)), no_download_equals_model=bool(np.array_equal(on_quiet, want)))
        assert np.array_equal(on_gen, want), "the generating handle packs under another key than (S, bodies)"
        assert np.array_equal(on_other, want)
        assert np.array_equal(on_quiet, want), "bodies = NULL left another key on the handle"
        assert np.array_equal(pk.bodies, _generate(shape).bodies) and pk.mask_seed == _generate(shape).mask_seed
        # a refused call leaves the previous packing key packing
        for bad in (-1.0, float("nan")):
            with pytest.raises(_capi.TfheHipError) as err:
                gen.gen_packing_key(sk.key_lv0, sk.key_lv1, rng_key=K, alpha=bad)
            assert err.value.code == _capi.EINVAL
            assert gen.packing_key_is_loaded() and np.array_equal(gen.pack(cts), want)
        seed = (_capi.C.c_uint8 * 32)()
        k0 = np.ascontiguousarray(sk.key_lv0, np.uint32)
        rc = gen._lib.tfhe_hip_gen_packing_key(gen._ctx, k0.ctypes.data, None, _capi.C.c_double(ALPHA), None, seed, None)
        assert rc == _capi.EINVAL and np.array_equal(gen.pack(cts), want)
    finally:
        for e in (gen, other, quiet):
            e.close()
    wide = R.Engine(KM.shape_params((16, 1, 22, 8, 3)), 0)  # basebit 8: no packing, no packing key
    try:
        with pytest.raises(_capi.TfheHipError) as err:
            wide.gen_packing_key(np.zeros(16, np.uint32), np.zeros(N, np.uint32), rng_key=K, alpha=ALPHA)
        assert err.value.code == _capi.EINVAL and not wide.packing_key_is_loaded()
    finally:
        wide.close()


# ---- 3. end to end at a real set -----------------------------------------------------------------------------------
def test_end_to_end_at_security_128_bit():
    """OS-keyed, in a key view SecretKey.packing_key(device=0) closes: 40 fresh encryptions pack and decrypt."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd.client import SecretKey

    P = R.params.SECURITY_128_BIT
    sk = SecretKey.new(P, 31)
    pk = sk.packing_key(device=0)
    assert pk.params == P and pk.bodies.shape == (P.n, P.iks_t, N) and len(pk.mask_seed) == 32
    with pytest.raises(ValueError):
        sk.packing_key(rng_key=4, device=0)
    bits = np.random.default_rng(9).integers(0, 2, 40).astype(bool)
    eng = R.Engine(P, 0)
    try:
        eng.load_packing_key(pk)
        packed = eng.pack(sk.encrypt_bool(bits, 8))
    finally:
        eng.close()
    got = sk.decrypt_packed_bool(packed, 40)
    _say(case="end to end", set=P.name, wrong=int((got != bits).sum()), key_bytes=pk.nbytes)
    assert np.array_equal(got, bits)


# ---- 4. statistics that do not depend on the model ------------------------------------------------------------------
def _report(case, shape, pk, bound):
    p = _params(shape)
    sk = KM.secret_key(p)
    e, a = PM.recover_noise(p, sk.key_lv0, sk.key_lv1, pk.mask_seed, pk.bodies)
    rep = KM.noise_report(e, ALPHA, KM.REF_SEED, mask=a)
    _say(case=case, shape=list(shape), report=rep)
    worst = KM.check_report(rep, bound, f"{case} packing key noise")
    _say(case=case, shape=list(shape), worst=worst)
    return e


@pytest.mark.parametrize("shape", KM.STAT_SHAPES, ids=_ids)
def test_recovered_noise_statistics(shape):
    """e = b - a (*) s1 - s0[i] g_l X^0, recovered with the secret key alone, through noise_report at 5 SE."""
    _report("fixed key", shape, _generate(shape), 5.0)


def test_os_keyed_route():
    """rng_key = NULL: the noise through noise_report at 6 SE; two calls give different seeds and share no noise row."""
    shape = KM.SHAPES[0]
    keys = [_generate(shape, rng_key=None) for _ in range(2)]
    noise = [_report(f"os-keyed #{i}", shape, pk, 6.0) for i, pk in enumerate(keys)]
    assert keys[0].mask_seed != keys[1].mask_seed and keys[0].mask_seed != PM.mask_seed(K)
    both = np.concatenate(noise)
    assert len(np.unique(both, axis=0)) == len(both), "two OS-keyed calls share a noise row"


# ---- 5. pool ---------------------------------------------------------------------------------------------------------
def test_pool_generates_on_the_first_member_and_loads_the_rest():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK

    shape = KM.SHAPES[0]
    p = _params(shape)
    sk = KM.secret_key(p)
    single = _generate(shape)
    cts = np.random.default_rng(78).integers(0, 1 << 32, (2100, p.n + 1), dtype=np.uint64).astype(np.uint32)
    pool = R.Pool(p, [0, 0])
    try:
        pk = pool.gen_packing_key(sk.key_lv0, sk.key_lv1, rng_key=K, alpha=ALPHA)
        assert pk.mask_seed == single.mask_seed and np.array_equal(pk.bodies, single.bodies)
        want = PK.pack_model(p, pk.mask_seed, pk.bodies, cts)  # three groups: both members get whole groups
        got = pool.pack(cts)
        members = [R.Engine.from_pool(pool, i).pack(cts[:70]) for i in range(2)]
        # bodies = NULL: the other member loads from the call's own host buffer; and a pool key view
        assert pool.gen_packing_key(sk.key_lv0, sk.key_lv1, rng_key=K, alpha=ALPHA, download=False) is None
        again = pool.pack(cts)
        view = pool.new_key_view()
        try:
            view.gen_packing_key(sk.key_lv0, sk.key_lv1, rng_key=K, alpha=ALPHA, download=False)
            on_view = view.pack(cts)
        finally:
            view.close()
        _say(case="pool", pack_equals_model=bool(np.array_equal(got, want)), no_download_equals_model=bool(np.array_equal(again, want)),
             view_equals_model=bool(np.array_equal(on_view, want)))
        assert np.array_equal(got, want) and np.array_equal(again, want) and np.array_equal(on_view, want)
        want70 = PK.pack_model(p, pk.mask_seed, pk.bodies, cts[:70])
        assert np.array_equal(members[0], want70) and np.array_equal(members[1], want70), "a member holds another key"
    finally:
        pool.close()


# ---- 6. C++ --------------------------------------------------------------------------------------------------------
def test_cpp_generates_the_same_key(tmp_path):
    """PackingKey::generate under the fixed K, Engine::pack of trivial ciphertexts, decode; the seed and the checksum of
    the bodies it prints are test 1's."""
    shape = KM.SHAPES[0]
    p = _params(shape)
    sk = KM.secret_key(p)
    pk = _generate(shape)
    blob = tmp_path / "key.bin"
    blob.write_bytes(K + np.ascontiguousarray(sk.key_lv0, "<u4").tobytes() + np.ascontiguousarray(sk.key_lv1, "<u4").tobytes())
    exe = build_cpp_packing_keygen(str(tmp_path))
    r = subprocess.run([exe] + [str(v) for v in shape] + [repr(ALPHA), str(blob)], capture_output=True, text=True, timeout=300)
    _say(case="c++", returncode=r.returncode, stdout=r.stdout.strip().splitlines())
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(ln.split(" ", 1) for ln in r.stdout.strip().splitlines())
    assert lines["seed"] == pk.mask_seed.hex()
    assert int(lines["checksum"]) == PM.checksum(pk.bodies)
    assert lines["ok:"].endswith("bytes")
