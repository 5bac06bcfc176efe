"""A CPU model of the two cloud-key generators (csrc/keygen.hpp, csrc/seeded.hpp), sample for sample.  No test functions.

Every mask word and every Gaussian sample of both generators is a fixed position of a ChaCha20 keystream, so the whole
key is a function of (secret key, generator key K, alphas) and numpy can compute it: rs_tfhe_amd.seeded supplies the
keystream (pinned to RFC 8439 in test_compressed_key_host.py), gauss2, f64_to_torus and the exact negacyclic product.

Three pieces sit on top of that:
  * the plain generator in the word order of k_lwe_rows / k_gen_bsk (streams 0/1 "KSK", 2/3 "BSK" under K; the
    compressed generator uses 16/17 and 18/19 with the masks under the mask seed) and key_from_seed, the SplitMix64
    expansion behind the 64-bit-seed entry point;
  * gauss2 in long double, which says where an f64 libm may legitimately land on the neighbouring torus word
    (`borderline`), and compare_words, the word-for-word comparison that allows exactly that and nothing else;
  * noise_report: moments, tails and correlations of recovered noise in standard errors of each statistic, against
    numpy's own normal(0, alpha) pushed through f64_to_torus.  It does not use the model, so it cannot share a mistake
    with the kernels the way the model could.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from rs_tfhe_amd import seeded as S
from rs_tfhe_amd.params import N, SecurityParams

MAX_MISMATCHES = 16  # words of one key that may sit on the other side of a borderline truncation
PLAIN = (0, 1, 2, 3)  # (KSK mask, KSK noise, BSK mask, BSK noise) stream numbers of keygen.hpp
COMPRESSED = (16, 17, 18, 19)  # ... of seeded.hpp
_PI = np.longdouble("3.14159265358979323846264338327950288")
_TWO32 = np.longdouble(4294967296.0)
# the largest radius of gauss2, in sigmas: u1 >= 2^-53
_RAD_MAX = float(np.sqrt(-2.0 * np.log(2.0 ** -53)))


# (n, l, bgbit, basebit, t): the shapes both test files generate keys at.  N stays 1024.
SHAPES = (
    (33, 3, 6, 2, 9),     # k_gen_bsk<3>, the 128-bit KSK geometry, ragged last keystream block
    (48, 2, 10, 2, 8),    # <2>
    (16, 1, 22, 5, 3),    # <1>, general-rounding key scale (2^-42), base 32
    (1279, 1, 10, 2, 2),  # largest n: 80 keystream blocks a row, padded KSK rows
    (1, 3, 6, 2, 3),      # smallest
)
STAT_SHAPES = (SHAPES[0], SHAPES[3])  # where the statistics are taken: 203 k and 2.6 M BSK samples
ALPHA_KSK, ALPHA_BSK, ALPHA_BSK_UINT = 2.0e-5, 2.0e-8, 2.220446049250313e-16  # the sets' (params.py)
GEN_KEY = bytes((37 * i + 11) & 0xFF for i in range(32))  # the fixed generator key of both test files
REF_SEED = 20250  # of noise_report's reference draw


def shape_params(shape, alpha_ksk=ALPHA_KSK, alpha_bsk=ALPHA_BSK) -> SecurityParams:
    n, l, bgbit, basebit, t = shape
    return SecurityParams(f"KEYGEN_{n}_{l}_{bgbit}_{alpha_bsk:g}", 0, n, l, bgbit, basebit, t, alpha_ksk, alpha_bsk)


def secret_key(p: SecurityParams):
    from rs_tfhe_amd.client import SecretKey

    return SecretKey.new(p, 4000 + p.n)


def key_from_seed(seed: int) -> bytes:
    """tfhe_hip.hip key_from_seed: four SplitMix64 outputs, low word first -> the 32-byte generator key."""
    mask = (1 << 64) - 1
    x = int(seed) & mask
    out = b""
    for _ in range(4):
        x = (x + 0x9E3779B97F4A7C15) & mask
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        z ^= z >> 31
        out += z.to_bytes(8, "little")
    return out


# ---- gauss2 in long double and the borderline rule ----------------------------------------------------------------
def gauss2_ld(w: np.ndarray, sigma: float):
    """seeded.gauss2 in np.longdouble.  Returns (x0, x1, g0, g1): the samples g and x = fmod(g, 1) * 2^32, the value
    f64_to_torus truncates toward zero."""
    w = w.astype(np.uint64)
    u1 = (((w[..., 0] << np.uint64(21)) ^ (w[..., 1] >> np.uint64(11))).astype(np.longdouble) + 1) / np.longdouble(2.0 ** 53)
    u2 = ((w[..., 2] << np.uint64(21)) ^ (w[..., 3] >> np.uint64(11))).astype(np.longdouble) / np.longdouble(2.0 ** 53)
    rad = np.sqrt(-2 * np.log(u1)) * np.longdouble(sigma)
    g0, g1 = rad * np.cos(2 * _PI * u2), rad * np.sin(2 * _PI * u2)
    return np.fmod(g0, 1) * _TWO32, np.fmod(g1, 1) * _TWO32, g0, g1


def ld_to_torus(x) -> np.ndarray:
    return np.trunc(x).astype(np.int64).astype(np.uint32)


def borderline(x, g, sigma: float) -> np.ndarray:
    """Where two correct f64 implementations may truncate to neighbouring words: x within max(2^-20, 2^-44 |g| 2^32) of
    an integer.  2^-44 is 256 ulp of f64 relative error, far above what log, sqrt and sincospi of any libm differ by;
    2^-20 covers the small-noise end.  A sigma so small that the largest sample stays below one torus step even with
    that relative error (sigma * 8.58 * 2^32 * (1 + 2^-44) < 1) truncates to zero in any arithmetic: no sample of it is
    borderline, and neither is any at sigma = 0."""
    if sigma * _RAD_MAX * 4294967296.0 * (1.0 + 2.0 ** -44) < 1.0:
        return np.zeros(np.shape(x), bool)
    tol = np.maximum(np.longdouble(2.0 ** -20), np.longdouble(2.0 ** -44) * np.abs(g) * _TWO32)
    return np.abs(x - np.rint(x)) < tol


def compare_words(got, want, border, label="") -> tuple:
    """got == want word for word, except that a word may differ by exactly +-1 LSB where `border` marks its noise
    sample, and at most MAX_MISMATCHES words in all.  Returns (mismatches, borderline samples)."""
    got, want, border = np.asarray(got, np.uint32), np.asarray(want, np.uint32), np.asarray(border, bool)
    assert got.shape == want.shape == border.shape, (label, got.shape, want.shape, border.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    if len(bad):
        d = (got.reshape(-1)[bad] - want.reshape(-1)[bad]).astype(np.int32)
        loose = bad[~border.reshape(-1)[bad]]
        assert len(loose) == 0, f"{label}: {len(loose)} words differ away from any borderline sample, first at flat index " \
                                f"{int(loose[0])}: got {int(got.reshape(-1)[loose[0]]):#x}, want {int(want.reshape(-1)[loose[0]]):#x}"
        assert (np.abs(d) == 1).all(), f"{label}: a borderline word is off by {int(np.abs(d).max())} LSB"
        assert len(bad) <= MAX_MISMATCHES, f"{label}: {len(bad)} borderline words differ (at most {MAX_MISMATCHES})"
    return len(bad), int(border.sum())


# ---- keystream positions ----------------------------------------------------------------------------------------
def ksk_live_rows(p: SecurityParams) -> np.ndarray:
    r = np.arange(N * p.iks_t * p.base, dtype=np.uint64)
    return r[(r % np.uint64(p.base)) != 0]


def _coeff_order(x):
    """[rows, lane, m] -> [rows, 64 m + lane]"""
    return x.transpose(0, 2, 1).reshape(x.shape[0], -1)


def plain_bsk_masks(K: bytes, rows) -> np.ndarray:
    """k_gen_bsk: block `lane` of (row, 2, "BSK") gives a[lane + 64 m] = w[m], a[lane + 64 m + 512] = w[8 + m]."""
    rows = np.asarray(rows, np.uint64)
    w = S.chacha20_block(K, np.arange(64, dtype=np.uint64), rows[:, None], PLAIN[2], S.DOMAIN_BSK)  # [rows, lane, 16]
    return np.concatenate([_coeff_order(w[:, :, :8]), _coeff_order(w[:, :, 8:])], axis=1)


def bsk_noise_words(K: bytes, rows, stream: int, no_row: bool = False) -> np.ndarray:
    """The four words of every Gaussian pair: [rows, lane, h, m, 4], blocks 2 lane + h of (row, stream, "BSK").
    no_row: the altered generator whose nonce forgets the row (test_keygen_model_host.py)."""
    rows = np.asarray(rows, np.uint64)
    nonce = np.zeros_like(rows) if no_row else rows
    w = S.chacha20_block(K, np.arange(128, dtype=np.uint64), nonce[:, None], stream, S.DOMAIN_BSK)
    return w.reshape(len(rows), 64, 2, 4, 4)


def _pairs_to_poly(a0, a1):
    """pair (lane, h, m) -> coefficients lane + 64 (4h + m) (first sample) and + 512 (second)"""
    r = a0.shape[0]
    return np.concatenate([_coeff_order(a0.reshape(r, 64, 8)), _coeff_order(a1.reshape(r, 64, 8))], axis=1)


@dataclass
class Noise:
    words: np.ndarray  # f64_to_torus of the f64 samples: what the generators add
    ld_words: np.ndarray  # the same through long double
    border: np.ndarray  # bool, the borderline rule


def bsk_noise(K: bytes, rows, alpha: float, stream: int, chunk: int = 256, **alter) -> Noise:
    """Noise polynomials [rows, N] of BSK rows `rows`, in k_gen_bsk's order (compress_bsk uses it with stream 19)."""
    rows = np.asarray(rows, np.uint64)
    out = Noise(np.zeros((len(rows), N), np.uint32), np.zeros((len(rows), N), np.uint32), np.zeros((len(rows), N), bool))
    for lo in range(0, len(rows), chunk):
        w = bsk_noise_words(K, rows[lo:lo + chunk], stream, **alter)
        g0, g1 = S.gauss2(w, alpha)
        x0, x1, l0, l1 = gauss2_ld(w, alpha)
        sl = slice(lo, lo + w.shape[0])
        out.words[sl] = _pairs_to_poly(S.f64_to_torus(g0), S.f64_to_torus(g1))
        out.ld_words[sl] = _pairs_to_poly(ld_to_torus(x0), ld_to_torus(x1))
        out.border[sl] = _pairs_to_poly(borderline(x0, l0, alpha), borderline(x1, l1, alpha))
    return out


def ksk_noise(K: bytes, rows, alpha: float, stream: int) -> Noise:
    """One sample a KSK row: g0 of gauss2(block(K, 0, row, stream, "KSK")[:4])."""
    w = S.chacha20_block(K, 0, np.asarray(rows, np.uint64), stream, S.DOMAIN_KSK)[:, :4]
    g0, _ = S.gauss2(w, alpha)
    x0, _, l0, _ = gauss2_ld(w, alpha)
    return Noise(S.f64_to_torus(g0), ld_to_torus(x0), borderline(x0, l0, alpha))


# ---- the rows, from given masks and noise ------------------------------------------------------------------------
def ksk_messages(p: SecurityParams, s1, rows) -> np.ndarray:
    """f64_to_torus(k s1[i] / 2^((j+1) basebit)) of rows base t i + base j + k"""
    r = np.asarray(rows, np.uint64)
    k = (r % np.uint64(p.base)).astype(np.int64)
    j = ((r // np.uint64(p.base)) % np.uint64(p.iks_t)).astype(np.int64)
    i = (r // np.uint64(p.base * p.iks_t)).astype(np.int64)
    s1 = np.asarray(s1, np.uint32).reshape(N).astype(np.int64)
    return S.f64_to_torus((k * s1[i]).astype(np.float64) / np.exp2(((j + 1) * p.basebit).astype(np.float64)))


def ksk_bodies(p: SecurityParams, s0, s1, rows, masks, e) -> np.ndarray:
    """<a, s0> + e + message, wrapping"""
    s0 = np.asarray(s0, np.uint32).reshape(p.n).astype(bool)
    with np.errstate(over="ignore"):
        inner = masks[:, s0].sum(axis=1, dtype=np.uint64).astype(np.uint32)
        return inner + np.asarray(e, np.uint32) + ksk_messages(p, s1, rows)


def bsk_gadgets(p: SecurityParams, s0, rows) -> np.ndarray:
    """s0[i] g_{q mod l} of rows i 2l + q"""
    r = np.asarray(rows, np.int64)
    g = np.array([S.gadget(p, d) for d in range(p.l)], np.uint32)
    return np.asarray(s0, np.uint32).reshape(p.n)[r // (2 * p.l)] * g[(r % (2 * p.l)) % p.l]


def plain_bsk_rows(p: SecurityParams, s0, s1, rows, a, e) -> np.ndarray:
    """k_gen_bsk from given masks and noise: b = e + a (*) s1 with the product taken BEFORE the gadget, then
    a[0] += s0[i] g_q (q < l) or b[0] += s0[i] g_{q-l}.  Returns [rows, 2, N]."""
    r = np.asarray(rows, np.int64)
    q = r % (2 * p.l)
    pg = bsk_gadgets(p, s0, r)
    out = np.empty((len(r), 2, N), np.uint32)
    with np.errstate(over="ignore"):
        out[:, 0] = a
        out[:, 1] = S.negacyclic_binary(np.asarray(a, np.uint32), np.asarray(s1, np.uint32).reshape(N)) + np.asarray(e, np.uint32)
        out[:, 0, 0] += np.where(q < p.l, pg, np.uint32(0))
        out[:, 1, 0] += np.where(q >= p.l, pg, np.uint32(0))
    return out


@dataclass
class PlainKey:
    ksk: np.ndarray  # [N][t][base][n+1] u32
    bsk: np.ndarray  # [n][2l][2][N] u32 torus polynomials
    ksk_border: np.ndarray  # [N][t][base][n+1] bool: only the body word of a live row can be set
    bsk_border: np.ndarray  # [n][2l][2][N] bool: only b words can be set
    e_ksk: Noise  # of the live rows, in row order
    e_bsk: Noise  # [n 2l, N]


def plain_key(p: SecurityParams, s0, s1, K: bytes, alpha_ksk=None, alpha_bsk=None) -> PlainKey:
    """tfhe_hip_gen_cloud_key_with_key(K) on the CPU."""
    a0 = p.alpha_lv0 if alpha_ksk is None else float(alpha_ksk)
    a1 = p.alpha_lv1 if alpha_bsk is None else float(alpha_bsk)
    rows_k = N * p.iks_t * p.base
    ksk = np.zeros((rows_k, p.n + 1), np.uint32)
    kb = np.zeros((rows_k, p.n + 1), bool)
    live = ksk_live_rows(p)
    ek = ksk_noise(K, live, a0, PLAIN[1])
    for lo in range(0, len(live), 4096):
        r = live[lo:lo + 4096]
        masks = S.keystream(K, p.n, r, PLAIN[0], S.DOMAIN_KSK)
        ksk[r.astype(np.int64), :-1] = masks
        ksk[r.astype(np.int64), -1] = ksk_bodies(p, s0, s1, r, masks, ek.words[lo:lo + 4096])
    kb[live.astype(np.int64), -1] = ek.border
    rows_b = np.arange(p.n * 2 * p.l, dtype=np.uint64)
    eb = bsk_noise(K, rows_b, a1, PLAIN[3])
    bsk = np.empty((len(rows_b), 2, N), np.uint32)
    for lo in range(0, len(rows_b), 256):
        r = rows_b[lo:lo + 256]
        bsk[lo:lo + 256] = plain_bsk_rows(p, s0, s1, r, plain_bsk_masks(K, r), eb.words[lo:lo + 256])
    bb = np.zeros(bsk.shape, bool)
    bb[:, 1] = eb.border
    return PlainKey(ksk.reshape(N, p.iks_t, p.base, p.n + 1), bsk.reshape(p.n, 2 * p.l, 2, N),
                    kb.reshape(N, p.iks_t, p.base, p.n + 1), bb.reshape(p.n, 2 * p.l, 2, N), ek, eb)


def compressed_noise(p: SecurityParams, K: bytes, alpha_ksk=None, alpha_bsk=None):
    """(KSK noise [N][t][base] with the k = 0 slots zero, BSK noise [n][2l][N]) of seeded.compress under K, as Noise."""
    a0 = p.alpha_lv0 if alpha_ksk is None else float(alpha_ksk)
    a1 = p.alpha_lv1 if alpha_bsk is None else float(alpha_bsk)
    live = ksk_live_rows(p).astype(np.int64)
    ek = ksk_noise(K, live, a0, COMPRESSED[1])
    full = Noise(*(np.zeros(N * p.iks_t * p.base, x.dtype) for x in (ek.words, ek.ld_words, ek.border)))
    for dst, src in ((full.words, ek.words), (full.ld_words, ek.ld_words), (full.border, ek.border)):
        dst[live] = src
    shape_k, shape_b = (N, p.iks_t, p.base), (p.n, 2 * p.l, N)
    eb = bsk_noise(K, np.arange(p.n * 2 * p.l), a1, COMPRESSED[3])
    return (Noise(full.words.reshape(shape_k), full.ld_words.reshape(shape_k), full.border.reshape(shape_k)),
            Noise(eb.words.reshape(shape_b), eb.ld_words.reshape(shape_b), eb.border.reshape(shape_b)))


# ---- noise recovered with the secret key (no model, no keystream) ------------------------------------------------
def recover_ksk_noise(p: SecurityParams, s0, s1, ksk):
    """(e, first mask word) of the live rows of a full KSK [N][t][base][n+1]: e = body - <a, s0> - message, as int32."""
    live = ksk_live_rows(p)
    rows = np.asarray(ksk, np.uint32).reshape(-1, p.n + 1)[live.astype(np.int64)]
    inner = (rows[:, :-1].astype(np.uint64) @ np.asarray(s0, np.uint64).reshape(p.n)).astype(np.uint32)
    with np.errstate(over="ignore"):
        e = rows[:, -1] - inner - ksk_messages(p, s1, live)
    return e.view(np.int32), rows[:, 0].copy()


def recover_bsk_noise(p: SecurityParams, s0, s1, bsk):
    """(e, a) of BSK torus polynomials [n][2l][2][N]: e = b - a (*) s1 + s0[i] g_q s1 for q < l, and
    b - a (*) s1 - s0[i] g_{q-l} X^0 for q >= l, as [rows, N] int32.  One formula serves both generators: the plain
    one moves a[0] by the gadget after the product, the compressed one folds -s0[i] g_q s1 into b instead."""
    rows = np.arange(p.n * 2 * p.l)
    x = np.asarray(bsk, np.uint32).reshape(len(rows), 2, N)
    s1 = np.asarray(s1, np.uint32).reshape(N)
    q = rows % (2 * p.l)
    pg = bsk_gadgets(p, s0, rows)
    with np.errstate(over="ignore"):
        e = x[:, 1] - S.negacyclic_binary(x[:, 0], s1)
        e += np.where(q < p.l, pg, np.uint32(0))[:, None] * s1[None, :]
        e[:, 0] -= np.where(q >= p.l, pg, np.uint32(0))
    return e.view(np.int32), x[:, 0].copy()


# ---- statistics in standard errors ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=16)
def _reference_draw(alpha: float, draws: int, rng_seed: int):
    """(std, excess kurtosis, share beyond 3 std) of numpy's normal(0, alpha) through f64_to_torus, in torus steps.
    The target is never alpha 2^32: truncation toward zero lowers the std by 0.6 % at alpha = 2e-8."""
    x = S.f64_to_torus(np.random.default_rng(rng_seed).normal(0.0, alpha, draws)).view(np.int32).astype(np.float64)
    sd = x.std()
    return sd, _kurtosis(x), float((np.abs(x) > 3.0 * sd).mean())


def _kurtosis(x):
    d = x - x.mean()
    m2 = (d * d).mean()
    return float((d ** 4).mean() / (m2 * m2) - 3.0)


def _corr(a, b):
    a, b = a.reshape(-1) - a.mean(), b.reshape(-1) - b.mean()
    den = np.sqrt((a * a).sum() * (b * b).sum())
    return float((a * b).sum() / den) if den > 0 else float("nan")


ROW = 1024  # BSK noise comes as rows of 1024; a 1-D array (KSK) is one sample a key row


def noise_report(e, alpha: float, rng_seed: int, mask=None) -> dict:
    """Every statistic of recovered noise `e` (int32; [rows, 1024] for a BSK, [M] for a KSK) as a count of ITS OWN
    standard errors, against a reference draw of at least 8 M samples:
        mean              mean, SE sigma / sqrt(M)
        std               std / reference std - 1, SE 1 / sqrt(2 M)
        kurtosis          excess kurtosis - the reference's, SE sqrt(24 / M)
        tail              share beyond 3 sigma - the reference's p, SE sqrt(p / M)
        pair_corr         coefficient c against c + 512 (the g0 / g1 of one Box-Muller pair), SE 1 / sqrt(M')
        row_corr          row r against row r + 1 (a KSK: sample r against r + 1), SE 1 / sqrt(M')
        mask_corr         noise against the mask word at the same position, SE 1 / sqrt(M)
        row_std           the worst single row's std / reference std - 1, SE 1 / sqrt(2 * 1024)  (BSK only)
    plus rows_distinct (bool; BSK only).  check_report holds them to a bound."""
    e = np.asarray(e)
    assert e.dtype == np.int32 and e.ndim in (1, 2) and (e.ndim == 1 or e.shape[1] == ROW)
    x = e.astype(np.float64)
    m = x.size
    sd, kurt, p3 = _reference_draw(float(alpha), max(8 * m, 1 << 20), int(rng_seed))
    rep = {
        "M": m,
        "mean": x.mean() / (sd / np.sqrt(m)),
        "std": (x.std() / sd - 1.0) * np.sqrt(2.0 * m),
        "kurtosis": (_kurtosis(x) - kurt) / np.sqrt(24.0 / m),
        "tail": (float((np.abs(x) > 3.0 * sd).mean()) - p3) / np.sqrt(p3 / m),
    }
    if e.ndim == 2:
        rep["pair_corr"] = _corr(x[:, :ROW // 2], x[:, ROW // 2:]) * np.sqrt(m / 2.0)
        rep["row_corr"] = _corr(x[:-1], x[1:]) * np.sqrt(m - ROW) if len(x) > 1 else 0.0
        rep["row_std"] = float(np.abs(x.std(axis=1) / sd - 1.0).max()) * np.sqrt(2.0 * ROW)
        rep["rows_distinct"] = len(np.unique(e, axis=0)) == len(e)
    else:
        rep["row_corr"] = _corr(x[:-1], x[1:]) * np.sqrt(m - 1.0)
    if mask is not None:
        mk = np.asarray(mask, np.uint32).view(np.int32).astype(np.float64)
        assert mk.shape == x.shape
        rep["mask_corr"] = _corr(x, mk) * np.sqrt(m)
    return rep


STATISTICS = ("mean", "std", "kurtosis", "tail", "pair_corr", "row_corr", "mask_corr", "row_std")


def failures(rep: dict, bound: float) -> list:
    """names of the statistics of `rep` beyond `bound` standard errors (NaN counts as beyond), and rows_distinct"""
    bad = [k for k in STATISTICS if k in rep and not abs(rep[k]) <= bound]
    if rep.get("rows_distinct") is False:
        bad.append("rows_distinct")
    return bad


def worst(rep: dict) -> tuple:
    k = max((k for k in STATISTICS if k in rep), key=lambda k: abs(rep[k]))
    return k, float(rep[k])


def check_report(rep: dict, bound: float, label="") -> tuple:
    bad = failures(rep, bound)
    assert not bad, f"{label}: beyond {bound} SE: " + ", ".join(f"{k} = {rep[k]}" for k in bad) + f"  (M = {rep['M']})"
    return worst(rep)


def ones_share_se(words) -> float:
    """(share of one bits - 1/2) of mask words in its standard error 1 / (2 sqrt(bits))"""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1)
    bits = w.size * 32
    ones = int(np.unpackbits(w.view(np.uint8)).sum(dtype=np.int64))
    return (ones / bits - 0.5) * 2.0 * np.sqrt(bits)
