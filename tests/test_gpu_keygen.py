"""Cloud-key generation on the GPU held to the CPU model of tests/keygen_model.py, sample for sample.

k_lwe_rows (the key-switching key's rows, plain and compressed) / k_gen_bsk<L> (keygen.hpp) and
k_gen_compressed_bsk<L> (seeded.hpp) are the only kernels of the cloud key whose output nobody can recompute from what
they are sent -- unless the generator key is fixed, and then every mask word and every Gaussian sample is a keystream position the model knows.  So: generate on the device, export, take
the BSK spectra back to torus polynomials (O.klemsa_fft, exact), and compare EVERY word.  A body may differ by exactly
+-1 LSB only where the long-double sampler marks its noise sample borderline, at most 16 words a key.

The model could share a mistake with the kernels; the statistics of test_recovered_noise_statistics could not: they
recover the noise with the secret key alone and hold its moments, tails and correlations, in standard errors of each
statistic, to numpy's own normal(0, alpha).  5 SE where the generator key is fixed (deterministic: passes or fails
forever), 6 SE on the OS-keyed routes (about 1e-8 a statistic a run).

The full-size SECURITY_128_BIT compressed key is held to the model in
test_gpu_compressed_key.py::test_gpu_generation_equals_cpu_generation, which already has the zero-noise CPU bodies the
noise is additive on.

Every test prints its figures (`KEYGEN ...` lines; run with -s) before it asserts."""
import json

import numpy as np
import pytest

import keygen_model as KM
from rs_tfhe_amd import seeded as S
from rs_tfhe_amd.params import N

pytestmark = pytest.mark.gpu

K = KM.GEN_KEY
_MODELS, _KEYS = {}, {}


def _say(**kv):
    print("KEYGEN " + json.dumps(kv, default=float))


def _torus(O, key, p):
    """exported CloudKey -> (KSK [N][t][base][n+1], BSK as torus polynomials [n][2l][2][N])"""
    bsk = np.stack([O.klemsa_fft(x) for x in key.bootstrapping_key.reshape(-1, N)]).reshape(p.n, 2 * p.l, 2, N)
    return np.asarray(key.key_switching_key, np.uint32), bsk


def _model(p, gen_key=K):
    k = (p, gen_key)
    if k not in _MODELS:
        sk = KM.secret_key(p)
        _MODELS[k] = KM.plain_key(p, sk.key_lv0, sk.key_lv1, gen_key)
    return _MODELS[k]


def _plain(O, p, **how):
    """(KSK, BSK torus) the plain generator leaves in a context, by route: rng_key=, seed=, or neither (OS-keyed)"""
    import rs_tfhe_amd as R

    fixed = how.get("rng_key") == K
    if fixed and (p, "plain") in _KEYS:
        return _KEYS[(p, "plain")]
    sk = KM.secret_key(p)
    eng = R.Engine(p, 0)
    try:
        eng.gen_cloud_key(sk.key_lv0, sk.key_lv1, **how)
        out = _torus(O, eng.export_cloud_key(), p)
    finally:
        eng.close()
    if fixed:
        _KEYS[(p, "plain")] = out
    return out


def _compressed(O, p, rng_key=K):
    """(CompressedCloudKey, KSK, BSK torus of the generating context) of the compressed generator"""
    import rs_tfhe_amd as R

    if rng_key is not None and (p, "compressed") in _KEYS:
        return _KEYS[(p, "compressed")]
    sk = KM.secret_key(p)
    eng = R.Engine(p, 0)
    try:
        ck = eng.gen_compressed_cloud_key(sk.key_lv0, sk.key_lv1, rng_key=rng_key)
        out = (ck,) + _torus(O, eng.export_cloud_key(), p)
    finally:
        eng.close()
    if rng_key is not None:
        _KEYS[(p, "compressed")] = out
    return out


def _hold_to_model(case, p, ksk, bsk, model):
    mk, bk = KM.compare_words(ksk, model.ksk, model.ksk_border, f"{case} KSK")
    mb, bb = KM.compare_words(bsk, model.bsk, model.bsk_border, f"{case} BSK")
    _say(case=case, shape=p.name, ksk_mismatches=mk, ksk_borderline=bk, bsk_mismatches=mb, bsk_borderline=bb)
    assert mk + mb <= KM.MAX_MISMATCHES
    return mk + mb


PLAIN_CASES = [(s, KM.ALPHA_BSK) for s in KM.SHAPES] + [(KM.SHAPES[2], KM.ALPHA_BSK_UINT)]
_ids = lambda v: str(v).replace(" ", "")  # noqa: E731


# ---- 1. plain generator, rng_key route ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,alpha_bsk", PLAIN_CASES, ids=_ids)
def test_plain_generator_equals_the_model(O, shape, alpha_bsk):
    """Every KSK word and every BSK word (masks, bodies, gadget, the all-zero k = 0 rows) of k_lwe_rows' key rows
    and k_gen_bsk<l>.  At alpha_bsk = 2.2e-16 the reference truncates the noise to zero and so must the device: no sample is
    borderline there, so the comparison is plain equality."""
    p = KM.shape_params(shape, alpha_bsk=alpha_bsk)
    ksk, bsk = _plain(O, p, rng_key=K)
    model = _model(p)
    if alpha_bsk == KM.ALPHA_BSK_UINT:
        assert not model.e_bsk.words.any() and not model.bsk_border.any()
        sk = KM.secret_key(p)
        e, _ = KM.recover_bsk_noise(p, sk.key_lv0, sk.key_lv1, bsk)
        assert not e.any(), "alpha_bsk = 2.2e-16 noise did not truncate to zero on the device"
    else:
        assert model.e_bsk.words.any()
    assert model.e_ksk.words.any()
    _hold_to_model("plain", p, ksk, bsk, model)


# ---- 2. the 64-bit-seed route ------------------------------------------------------------------------------------
def test_seed_route_is_the_model_under_the_splitmix64_key(O):
    import rs_tfhe_amd as R

    p = KM.shape_params(KM.SHAPES[0])
    seed = 0x0123456789ABCDEF
    model = _model(p, KM.key_from_seed(seed))
    ksk, bsk = _plain(O, p, seed=seed)
    _hold_to_model("seed", p, ksk, bsk, model)
    sk = KM.secret_key(p)
    pool = R.Pool(p, [0, 0])
    try:
        pool.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=seed)
        m0, m1 = pool.export_cloud_key(0), pool.export_cloud_key(1)
    finally:
        pool.close()
    assert np.array_equal(m0.key_switching_key, m1.key_switching_key)
    assert np.array_equal(m0.bootstrapping_key.view(np.uint64), m1.bootstrapping_key.view(np.uint64))
    assert np.array_equal(m0.key_switching_key, ksk)
    assert np.array_equal(_torus(O, m0, p)[1], bsk)


# ---- 3. compressed generator at real noise -----------------------------------------------------------------------
COMPRESSED_CASES = [(s, KM.ALPHA_BSK) for s in KM.SHAPES] + [(KM.SHAPES[2], KM.ALPHA_BSK_UINT)]


@pytest.mark.parametrize("shape,alpha_bsk", COMPRESSED_CASES, ids=_ids)
def test_compressed_generator_equals_the_cpu_compressor(O, shape, alpha_bsk):
    """mask_seed, bsk_bodies and ksk_bodies against SecretKey.compressed_cloud_key(rng_key=K) at the set's alphas, and
    the generating context's key against what a load of the CPU-made key leaves in another context."""
    import rs_tfhe_amd as R

    p = KM.shape_params(shape, alpha_bsk=alpha_bsk)
    sk = KM.secret_key(p)
    cpu = sk.compressed_cloud_key(rng_key=K)
    gpu, ksk, bsk = _compressed(O, p)
    ek, eb = KM.compressed_noise(p, K)
    assert bool(eb.words.any()) == (alpha_bsk != KM.ALPHA_BSK_UINT) and ek.words.any()
    assert gpu.mask_seed == cpu.mask_seed == S.mask_seed_of(K)
    assert gpu.decomposition_offset == cpu.decomposition_offset
    mb, bb = KM.compare_words(gpu.bsk_bodies, cpu.bsk_bodies, eb.border, "compressed BSK bodies")
    mk, bk = KM.compare_words(gpu.ksk_bodies, cpu.ksk_bodies, ek.border, "compressed KSK bodies")
    _say(case="compressed", shape=p.name, ksk_mismatches=mk, ksk_borderline=bk, bsk_mismatches=mb, bsk_borderline=bb)
    assert mk + mb <= KM.MAX_MISMATCHES
    other = R.Engine(p, 0)
    try:
        other.load_compressed_cloud_key(cpu)
        loaded = other.export_cloud_key()
    finally:
        other.close()
    lk, lb = _torus(O, loaded, p)
    assert np.array_equal(lk, S.expand_ksk(p, cpu.mask_seed, cpu.ksk_bodies))
    assert np.array_equal(lb, S.expand_bsk_torus(p, cpu.mask_seed, cpu.bsk_bodies))
    kborder = np.zeros(lk.shape, bool)
    kborder[..., -1] = ek.border
    bborder = np.zeros(lb.shape, bool)
    bborder[:, :, 1] = eb.border
    assert KM.compare_words(ksk, lk, kborder, "generating context's KSK")[0] == mk
    assert KM.compare_words(bsk, lb, bborder, "generating context's BSK")[0] == mb


# ---- 4. wrapping noise -------------------------------------------------------------------------------------------
def test_wrapping_noise_equals_the_model(O):
    """alpha = 0.5 on both keys: |g| > 1 occurs and fmod folds it.  Model equality only (the borderline rule's relative
    term is 2^-13 of a torus step here, so more than 16 samples are borderline; at most 16 words may still differ)."""
    import rs_tfhe_amd as R

    p = KM.shape_params(KM.SHAPES[0], alpha_ksk=0.5, alpha_bsk=0.5)
    sk = KM.secret_key(p)
    g0, _ = S.gauss2(KM.bsk_noise_words(K, np.arange(8), KM.PLAIN[3]), 0.5)
    assert (np.abs(g0) > 1.0).any()
    ksk, bsk = _plain(O, p, rng_key=K)
    _hold_to_model("wrapping plain", p, ksk, bsk, _model(p))
    cpu = sk.compressed_cloud_key(rng_key=K)
    gpu, _, _ = _compressed(O, p)
    ek, eb = KM.compressed_noise(p, K)
    mb, bb = KM.compare_words(gpu.bsk_bodies, cpu.bsk_bodies, eb.border, "wrapping compressed BSK bodies")
    mk, bk = KM.compare_words(gpu.ksk_bodies, cpu.ksk_bodies, ek.border, "wrapping compressed KSK bodies")
    _say(case="wrapping compressed", shape=p.name, ksk_mismatches=mk, ksk_borderline=bk, bsk_mismatches=mb, bsk_borderline=bb)
    assert mk + mb <= KM.MAX_MISMATCHES


# ---- 5. statistics that do not depend on the model --------------------------------------------------------------
def _report(case, p, ksk, bsk, bound):
    sk = KM.secret_key(p)
    eb, a = KM.recover_bsk_noise(p, sk.key_lv0, sk.key_lv1, bsk)
    ek, m0 = KM.recover_ksk_noise(p, sk.key_lv0, sk.key_lv1, ksk)
    rb = KM.noise_report(eb, p.alpha_lv1, KM.REF_SEED, mask=a)
    rk = KM.noise_report(ek, p.alpha_lv0, KM.REF_SEED, mask=m0)
    _say(case=case, shape=p.name, bsk=rb, ksk=rk)
    wb = KM.check_report(rb, bound, f"{case} BSK noise")
    wk = KM.check_report(rk, bound, f"{case} KSK noise")
    _say(case=case, shape=p.name, worst_bsk=wb, worst_ksk=wk)
    return eb, a


@pytest.mark.parametrize("generator", ["plain", "compressed"])
@pytest.mark.parametrize("shape", KM.STAT_SHAPES, ids=_ids)
def test_recovered_noise_statistics(O, shape, generator):
    """e_bsk = b - a (*) s1 -+ the gadget terms and e_ksk = body - <a, s0> - f64_to_torus(message), recovered with
    the secret key alone, through noise_report at 5 SE."""
    p = KM.shape_params(shape)
    ksk, bsk = _plain(O, p, rng_key=K) if generator == "plain" else _compressed(O, p)[1:]
    _report(generator, p, ksk, bsk, 5.0)


# ---- 6. OS-keyed routes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("generator", ["plain", "compressed"])
def test_os_keyed_routes(O, generator):
    """gen_cloud_key with nothing given and gen_compressed_cloud_key(rng_key=None): the noise through noise_report at
    6 SE, the share of one bits over all mask words within 6 SE of 1/2, and two calls share no noise row and no mask row."""
    p = KM.shape_params(KM.SHAPES[0])
    seen = []
    for call in range(2):
        ksk, bsk = _plain(O, p) if generator == "plain" else _compressed(O, p, rng_key=None)[1:]
        eb, a = _report(f"os-keyed {generator} #{call}", p, ksk, bsk, 6.0)
        live = KM.ksk_live_rows(p).astype(np.int64)
        kmask = ksk.reshape(-1, p.n + 1)[live, :-1]
        # a[0] of a plain row with q < l carries the gadget: leave coefficient 0 out of the bit count
        bits = KM.ones_share_se(np.concatenate([kmask.reshape(-1), a[:, 1:].reshape(-1)]))
        _say(case=f"os-keyed {generator} #{call}", ones_share_se=bits, mask_words=kmask.size + a[:, 1:].size)
        assert abs(bits) <= 6.0
        seen.append((eb, a[:, 1:], kmask))
    for x, y, what in zip(seen[0], seen[1], ("BSK noise", "BSK mask", "KSK mask")):
        both = np.concatenate([x, y])
        assert len(np.unique(both, axis=0)) == len(both), f"two OS-keyed calls share a {what} row"
