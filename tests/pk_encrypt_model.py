"""A CPU model of public-key encryption and of the asymmetric re-encryption key in the keyed format of
include/tfhe_hip.h ("public-key encryption and the asymmetric re-encryption key"), term by term.  No test functions.

The package's CPU form (rs_tfhe_amd.proxy_reenc.encrypt_rows) turns the selectors into a +-1 / 0 matrix and multiplies
in f64; the kernels split the public key into byte planes and multiply on the matrix cores.  This model does neither: it
reads every selector bit off seeded.chacha20_block at the position the header states and walks the entries one by one
with wrapping u32 adds.  keygen_model (KM) supplies the long-double sampler and the borderline rule for the one noise
sample a row has.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

import keygen_model as KM
from rs_tfhe_amd import seeded as S
from rs_tfhe_amd.params import SecurityParams

PKE = (0x504B45, 0x504B4E)  # "PKE", "PKN"
RKE = (0x524B45, 0x524B4E)  # "RKE", "RKN"
K = KM.GEN_KEY
HIGH = (1 << 32) - 5  # a first index whose rows cross 2^32: the nonce's second word comes into play
SHAPE = (33, 3, 6, 2, 9)  # the small asymmetric-key shape

# (n, size, count, first_index, alpha): every n, size, count, first index and alpha of the list once, not the grid.
#   n     33 (ragged second tile), 255 (exactly one 8-tile group), 256 (a second group holding one column), 700
#   size  1, 31, 32, 33, 2n, 1399          count  1, 31, 32, 33, 3000
CASES = (
    (33, 1, 1, 0, 0.0),
    (33, 31, 31, HIGH, 2e-5),
    (33, 66, 3000, 0, 2e-5),
    (255, 32, 32, 0, 0.0),
    (255, 33, 33, HIGH, 0.5),
    (256, 512, 31, 0, 2e-5),
    (256, 33, 1, HIGH, 0.0),
    (700, 1399, 33, HIGH, 2e-5),
    (700, 1400, 32, 0, 0.5),
)


def params(n: int) -> SecurityParams:
    return KM.shape_params((n,) + SHAPE[1:])


def public_key(n: int, size: int) -> np.ndarray:
    """[size][n+1] encryptions of zero under KM.secret_key(params(n)) (numpy's generator: reproducible)"""
    p = params(n)
    return KM.secret_key(p).encrypt_f64(np.zeros(size), 9000 + size, p.alpha_lv0)


def adversarial_key(n: int, size: int) -> np.ndarray:
    """Words 0x80000000 and 0x7F7F7F80: plane bytes -128 and +127 / -128, a carry out of every plane"""
    e = np.empty((size, n + 1), np.uint32)
    e[...] = np.where((np.arange(size)[:, None] + np.arange(n + 1)[None, :]) % 2 == 0, 0x80000000, 0x7F7F7F80)
    return e


def row_indices(first_index: int, count: int) -> np.ndarray:
    return np.uint64(int(first_index)) + np.arange(count, dtype=np.uint64)


def selector_bits(key: bytes, rows, size: int, domain: int):
    """(take, sign) [rows][size] bool: entry e reads bits 2 (e % 16) and 2 (e % 16) + 1 of selector word w = e / 16, which
    is word w % 16 of block w / 16 of the stream (g & 0xffffffff, g >> 32, domain)."""
    g = np.asarray(rows, np.uint64).reshape(-1)
    take = np.zeros((len(g), size), bool)
    sign = np.zeros((len(g), size), bool)
    for blk in range((size + 255) // 256):
        w = S.chacha20_block(key, blk, g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), domain)  # [rows, 16]
        for e in range(256 * blk, min(size, 256 * (blk + 1))):
            word = w[:, (e // 16) % 16]
            take[:, e] = (word >> np.uint32(2 * (e % 16))) & np.uint32(1)
            sign[:, e] = (word >> np.uint32(2 * (e % 16) + 1)) & np.uint32(1)
    return take, sign


def _walk(enc: np.ndarray, take: np.ndarray, sign: np.ndarray) -> np.ndarray:
    """out[r] = sum_e c_e E[e], one entry at a time, wrapping u32"""
    out = np.zeros((take.shape[0], enc.shape[1]), np.uint32)
    tmp = np.empty_like(out)
    coef = np.where(take, np.where(sign, np.uint32(0xFFFFFFFF), np.uint32(1)), np.uint32(0)).astype(np.uint32)
    with np.errstate(over="ignore"):
        for e in range(enc.shape[0]):
            np.multiply(coef[:, e, None], enc[e][None, :], out=tmp)  # +E[e], -E[e] (mod 2^32) or 0
            out += tmp
    return out


def subset_sums(enc, take, sign, threads: int = 16, chunk: int = 1024) -> np.ndarray:
    """_walk over row chunks (numpy releases the interpreter lock: the large key takes seconds, not a minute)"""
    spans = [(lo, min(lo + chunk, len(take))) for lo in range(0, len(take), chunk)]
    if len(spans) <= 1:
        return _walk(enc, take, sign)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda s: _walk(enc, take[s[0]:s[1]], sign[s[0]:s[1]]), spans))
    return np.concatenate(parts)


def noise(key: bytes, rows, alpha: float, domain: int) -> KM.Noise:
    """One sample a row: g0 of gauss2(words 0..3 of block 0 of (g & 0xffffffff, g >> 32, domain))"""
    g = np.asarray(rows, np.uint64).reshape(-1)
    w = S.chacha20_block(key, 0, g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), domain)[:, :4]
    g0, _ = S.gauss2(w, alpha)
    x0, _, l0, _ = KM.gauss2_ld(w, alpha)
    return KM.Noise(S.f64_to_torus(g0), KM.ld_to_torus(x0), KM.borderline(x0, l0, alpha))


def encrypt(enc, key: bytes, rows, plain, alpha: float, domains=PKE):
    """(words [rows][n+1], border [rows][n+1]): the rows `rows` of the format; only a body can be borderline"""
    enc = np.ascontiguousarray(enc, np.uint32)
    take, sign = selector_bits(key, rows, enc.shape[0], domains[0])
    out = subset_sums(enc, take, sign)
    e = noise(key, rows, alpha, domains[1])
    border = np.zeros(out.shape, bool)
    with np.errstate(over="ignore"):
        out[:, -1] += np.asarray(plain, np.uint32).reshape(-1) + e.words
    border[:, -1] = e.border
    return out, border


def reenc_plaintexts(p: SecurityParams, key_from) -> np.ndarray:
    """f64_to_torus(((k key_from[i]) as u32 as f64) / 2^((j+1) basebit)) of every row base t i + base j + k"""
    r = np.arange(p.n * p.iks_t * p.base, dtype=np.int64)
    k, j, i = r % p.base, (r // p.base) % p.iks_t, r // (p.base * p.iks_t)
    val = ((k * np.asarray(key_from, np.int64).reshape(p.n)[i]) & 0xFFFFFFFF).astype(np.float64)
    return S.f64_to_torus(val / np.exp2(((j + 1) * p.basebit).astype(np.float64)))


def reenc_key(p: SecurityParams, enc, key_from, key: bytes, alpha: float):
    """(key [n t base][n+1], border): the asymmetric re-encryption key; the k = 0 rows zero, their streams unused"""
    rows = np.arange(p.n * p.iks_t * p.base, dtype=np.uint64)
    live = (rows % np.uint64(p.base)) != 0
    out = np.zeros((len(rows), p.n + 1), np.uint32)
    border = np.zeros(out.shape, bool)
    out[live], border[live] = encrypt(enc, key, rows[live], reenc_plaintexts(p, key_from)[live], alpha, RKE)
    return out, border


def checksum(words) -> int:
    """sum of (2 x + 1) w[x] mod 2^64 over the flat words (tests/cpp/test_pk_encrypt.cpp prints the same)"""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int((w * (np.uint64(2) * np.arange(len(w), dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))
