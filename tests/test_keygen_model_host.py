"""The key-generation model and its checkers (tests/keygen_model.py) proven on the CPU, no device: the plain model
agrees with seeded.compress where the two formats must, its rows decrypt exactly at zero noise, the f64 and long-double
samplers give the same torus words away from the borderline samples (at most 16 a key), the model's own noise passes
noise_report at every (shape, alpha) the GPU tests use with a fixed key -- and the checkers FAIL, each for its own
reason, on a sigma 3 % low, a noise nonce without the row, g1 := g0, one zero row, noise copied from the mask and one
word off by one LSB."""
import numpy as np
import pytest

import keygen_model as KM
from rs_tfhe_amd import seeded as S
from rs_tfhe_amd.params import N

K = KM.GEN_KEY
_CACHE = {}


def _noise(shape, streams, alpha_bsk=KM.ALPHA_BSK):
    """(params, secret key, KSK noise of the live rows, BSK noise) of one generator at the set-like alphas"""
    key = (shape, streams, alpha_bsk)
    if key not in _CACHE:
        p = KM.shape_params(shape, alpha_bsk=alpha_bsk)
        ek = KM.ksk_noise(K, KM.ksk_live_rows(p), p.alpha_lv0, streams[1])
        eb = KM.bsk_noise(K, np.arange(p.n * 2 * p.l), p.alpha_lv1, streams[3])
        _CACHE[key] = (p, KM.secret_key(p), ek, eb)
    return _CACHE[key]


def test_key_from_seed_is_splitmix64():
    """Vigna's splitmix64.c: the first outputs for the states 0 and 1234567, low word first."""
    assert KM.key_from_seed(0)[:8] == (0xE220A8397B1DCDAF).to_bytes(8, "little")
    want = (6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431)
    assert KM.key_from_seed(1234567) == b"".join(v.to_bytes(8, "little") for v in want)
    assert KM.key_from_seed(1 << 64) == KM.key_from_seed(0) and len(KM.key_from_seed(7)) == 32


@pytest.mark.parametrize("shape", KM.SHAPES[:3] + KM.SHAPES[4:], ids=str)
def test_plain_model_and_compressor_agree_at_equal_masks_and_noise(shape):
    """Fed the compressor's own masks (under the mask seed) and noise (streams 17 / 19), the plain model's rows are the
    compressed key's expansion up to the one thing the formats differ in: for q < l the plain a carries the gadget
    and the compressed b carries -s0[i] g_q s1 instead."""
    p = KM.shape_params(shape)
    sk = KM.secret_key(p)
    seed, bsk_c, ksk_c, _ = S.compress(p, sk.key_lv0, sk.key_lv1, K)
    rows = np.arange(p.n * 2 * p.l)
    a = S.bsk_masks(p, seed, rows)
    e = KM.bsk_noise(K, rows, p.alpha_lv1, KM.COMPRESSED[3])
    plain = KM.plain_bsk_rows(p, sk.key_lv0, sk.key_lv1, rows, a, e.words)
    q, pg = rows % (2 * p.l), KM.bsk_gadgets(p, sk.key_lv0, rows)
    assert pg.any() and (q < p.l).any()
    with np.errstate(over="ignore"):
        fold = np.where(q < p.l, pg, np.uint32(0))[:, None] * sk.key_lv1[None, :]
        assert np.array_equal(bsk_c.reshape(-1, N), plain[:, 1] - fold)
        assert np.array_equal(plain[:, 0, 1:], a[:, 1:])
        assert np.array_equal(plain[:, 0, 0], a[:, 0] + np.where(q < p.l, pg, np.uint32(0)))
    live = KM.ksk_live_rows(p)
    masks = S.keystream(seed, p.n, live, KM.COMPRESSED[0], S.DOMAIN_KSK)
    ek = KM.ksk_noise(K, live, p.alpha_lv0, KM.COMPRESSED[1])
    bodies = KM.ksk_bodies(p, sk.key_lv0, sk.key_lv1, live, masks, ek.words)
    assert np.array_equal(ksk_c.reshape(-1)[live.astype(np.int64)], bodies)
    assert not ksk_c[:, :, 0].any()
    # compressed_noise is the same noise in the bodies' layout
    ck, cb = KM.compressed_noise(p, K)
    assert np.array_equal(cb.words.reshape(-1, N), e.words) and np.array_equal(ck.words.reshape(-1)[live.astype(np.int64)], ek.words)
    # ... and what the recovery of the GPU tests reads off either form is that noise
    got, _ = KM.recover_bsk_noise(p, sk.key_lv0, sk.key_lv1, plain)
    assert np.array_equal(got.view(np.uint32), e.words)
    got, _ = KM.recover_bsk_noise(p, sk.key_lv0, sk.key_lv1, S.expand_bsk_torus(p, seed, bsk_c))
    assert np.array_equal(got.view(np.uint32), e.words)
    got, m0 = KM.recover_ksk_noise(p, sk.key_lv0, sk.key_lv1, S.expand_ksk(p, seed, ksk_c))
    assert np.array_equal(got.view(np.uint32), ek.words) and np.array_equal(m0, masks[:, 0])


@pytest.mark.parametrize("shape", KM.SHAPES[:3] + KM.SHAPES[4:], ids=str)
def test_plain_model_rows_decrypt_exactly_at_zero_noise(shape):
    p = KM.shape_params(shape)
    sk = KM.secret_key(p)
    key = KM.plain_key(p, sk.key_lv0, sk.key_lv1, K, alpha_ksk=0.0, alpha_bsk=0.0)
    assert not key.ksk_border.any() and not key.bsk_border.any() and not key.e_bsk.words.any()
    s0, s1 = sk.key_lv0, sk.key_lv1
    # KSK: phase k s1[i] 2^(32 - (j+1) basebit); the k = 0 rows are all zero
    ksk = key.ksk.reshape(-1, p.n + 1)
    r = np.arange(len(ksk))
    k, j, i = r % p.base, (r // p.base) % p.iks_t, r // (p.base * p.iks_t)
    phase = ksk[:, -1] - (ksk[:, :-1].astype(np.uint64) @ s0.astype(np.uint64)).astype(np.uint32)
    want = (k * s1[i].astype(np.int64)) << (32 - (j + 1) * p.basebit)
    assert np.array_equal(phase, (want & 0xFFFFFFFF).astype(np.uint32))
    assert not key.ksk[:, :, 0].any()
    # BSK: row (i, q) is a TRLWE of 0 plus s0[i] 2^(32 - (q mod l + 1) bgbit) on a[0] (q < l) or b[0] (q >= l)
    bsk = key.bsk.reshape(-1, 2, N)
    rows = np.arange(len(bsk))
    q = rows % (2 * p.l)
    g = (s0[rows // (2 * p.l)].astype(np.int64) << (32 - (q % p.l + 1) * p.bgbit)).astype(np.uint32)
    with np.errstate(over="ignore"):
        phase = bsk[:, 1] - S.negacyclic_binary(bsk[:, 0], s1)
        want = np.zeros_like(phase)
        want[:, 0] = np.where(q >= p.l, g, np.uint32(0))
        want -= np.where(q < p.l, g, np.uint32(0))[:, None] * s1[None, :]
    assert np.array_equal(phase, want)
    # the masks are the keystream: the plain BSK mask of row r under K is the lane-major reading of stream 2
    a = KM.plain_bsk_masks(K, [5])[0]
    blk = S.chacha20_block(K, 7, 5, 2, S.DOMAIN_BSK)
    assert [int(a[7 + 64 * m]) for m in range(8)] == [int(x) for x in blk[:8]]
    assert [int(a[7 + 64 * m + 512]) for m in range(8)] == [int(x) for x in blk[8:]]


@pytest.mark.parametrize("streams", [KM.PLAIN, KM.COMPRESSED], ids=["plain", "compressed"])
@pytest.mark.parametrize("shape", KM.SHAPES, ids=str)
def test_f64_and_long_double_samplers_agree_away_from_borderline(shape, streams):
    """... and a key has at most 16 borderline samples: a condition the chosen generator key meets, not a measurement."""
    p, _, ek, eb = _noise(shape, streams)
    total = 0
    for e in (ek, eb):
        differ = e.words != e.ld_words
        assert not (differ & ~e.border).any()
        d = (e.words[differ] - e.ld_words[differ]).astype(np.int32)
        assert (np.abs(d) == 1).all()
        total += int(e.border.sum())
    assert total <= KM.MAX_MISMATCHES, total
    assert eb.words.any() and ek.words.any()


def test_uint_set_noise_truncates_to_zero():
    """alpha_bsk = 2.2e-16 (the bgbit 22 sets): 8.58 sigma 2^32 = 8.2e-6 of a torus step, so every sample truncates to
    zero in any arithmetic and none is borderline; the wrapping alpha folds through fmod and agrees too."""
    for streams in (KM.PLAIN, KM.COMPRESSED):
        _, _, _, eb = _noise(KM.SHAPES[2], streams, KM.ALPHA_BSK_UINT)
        assert not eb.words.any() and not eb.ld_words.any() and not eb.border.any()
    e = KM.bsk_noise(K, np.arange(24), 0.5, KM.PLAIN[3])
    g0, _ = S.gauss2(KM.bsk_noise_words(K, np.arange(24), KM.PLAIN[3]), 0.5)
    assert (np.abs(g0) > 1.0).any()  # |g| > 1 occurs and fmod folds it
    assert not ((e.words != e.ld_words) & ~e.border).any()
    assert e.border.mean() < 1e-3


def _masks(p, streams, rows):
    return KM.plain_bsk_masks(K, rows) if streams == KM.PLAIN else S.bsk_masks(p, S.mask_seed_of(K), rows)


@pytest.mark.parametrize("streams", [KM.PLAIN, KM.COMPRESSED], ids=["plain", "compressed"])
@pytest.mark.parametrize("shape", KM.STAT_SHAPES, ids=str)
def test_the_models_own_noise_passes_the_report(shape, streams):
    p, sk, ek, eb = _noise(shape, streams)
    rows = np.arange(p.n * 2 * p.l)
    rep = KM.noise_report(eb.words.view(np.int32), p.alpha_lv1, KM.REF_SEED, mask=_masks(p, streams, rows))
    KM.check_report(rep, 5.0, f"BSK {shape}")
    assert rep["rows_distinct"] and rep["M"] == len(rows) * N and {"pair_corr", "row_corr", "mask_corr", "row_std"} <= set(rep)
    live = KM.ksk_live_rows(p)
    seed = K if streams == KM.PLAIN else S.mask_seed_of(K)
    m0 = S.keystream(seed, 1, live, streams[0], S.DOMAIN_KSK)[:, 0]
    rep = KM.noise_report(ek.words.view(np.int32), p.alpha_lv0, KM.REF_SEED, mask=m0)
    KM.check_report(rep, 5.0, f"KSK {shape}")


# ---- the checkers fail on altered generators ---------------------------------------------------------------------
def _bsk_report(e, mask=None):
    p, sk, _, _ = _noise(KM.SHAPES[0], KM.PLAIN)
    if mask is None:
        mask = KM.plain_bsk_masks(K, np.arange(p.n * 2 * p.l))
    return KM.noise_report(np.ascontiguousarray(e).view(np.int32), p.alpha_lv1, KM.REF_SEED, mask=mask)


def test_report_fails_on_sigma_three_percent_low():
    p, _, _, eb = _noise(KM.SHAPES[0], KM.PLAIN)
    assert eb.words.size >= 60000  # 0.03 sqrt(2 M) = 19 SE here
    low = KM.bsk_noise(K, np.arange(p.n * 2 * p.l), 0.97 * p.alpha_lv1, KM.PLAIN[3])
    rep = _bsk_report(low.words)
    assert "std" in KM.failures(rep, 5.0) and rep["std"] < -10.0
    with pytest.raises(AssertionError, match="std"):
        KM.check_report(rep, 5.0)


def test_report_fails_on_a_noise_nonce_without_the_row():
    p, _, _, _ = _noise(KM.SHAPES[0], KM.PLAIN)
    same = KM.bsk_noise(K, np.arange(p.n * 2 * p.l), p.alpha_lv1, KM.PLAIN[3], no_row=True)
    rep = _bsk_report(same.words)
    bad = KM.failures(rep, 5.0)
    assert "rows_distinct" in bad and "row_corr" in bad


def test_report_fails_on_g1_equal_to_g0():
    _, _, _, eb = _noise(KM.SHAPES[0], KM.PLAIN)
    e = eb.words.copy()
    e[:, 512:] = e[:, :512]
    rep = _bsk_report(e)
    assert "pair_corr" in KM.failures(rep, 5.0)
    assert not {"mean", "std", "kurtosis", "tail", "row_std"} & set(KM.failures(rep, 5.0))


def test_report_fails_on_one_zero_row():
    _, _, _, eb = _noise(KM.SHAPES[0], KM.PLAIN)
    e = eb.words.copy()
    e[77] = 0
    rep = _bsk_report(e)
    assert KM.failures(rep, 5.0) == ["row_std"]  # one row in 198: the whole-key moments move by 1.6 SE and miss it


def test_report_fails_on_noise_copied_from_the_mask():
    p, _, _, _ = _noise(KM.SHAPES[0], KM.PLAIN)
    mask = KM.plain_bsk_masks(K, np.arange(p.n * 2 * p.l))
    e = (mask.view(np.int32) >> 24).astype(np.int32)  # a signed byte of the mask: the noise's size (sigma 86), not its law
    rep = _bsk_report(e, mask)
    assert "mask_corr" in KM.failures(rep, 5.0) and rep["mask_corr"] > 100.0


def test_word_comparison_fails_on_one_lsb():
    _, _, _, eb = _noise(KM.SHAPES[0], KM.PLAIN)
    want, border = eb.words, eb.border
    assert KM.compare_words(want.copy(), want, border) == (0, int(border.sum()))
    r, c = np.argwhere(~border)[12345]
    got = want.copy()
    got[r, c] += 1
    with pytest.raises(AssertionError, match="away from any borderline"):
        KM.compare_words(got, want, border)
    # on a borderline sample one LSB passes, two do not, and neither do seventeen of them
    marked = np.zeros_like(border)
    marked[r, c] = True
    assert KM.compare_words(got, want, marked) == (1, 1)
    got[r, c] += 1
    with pytest.raises(AssertionError, match="off by 2"):
        KM.compare_words(got, want, marked)
    got = want.copy()
    got[0, :17] -= 1
    marked[0, :17] = True
    with pytest.raises(AssertionError, match="17 borderline"):
        KM.compare_words(got, want, marked)
