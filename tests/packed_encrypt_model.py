"""A CPU model of packed TRLWE encryption in the format of include/tfhe_hip.h ("packed encryption"), term by term.
No test functions.

The package's CPU form (rs_tfhe_amd.seeded.symmetric_trlwe_rows) draws a group's mask with seeded.keystream and its
product with seeded.negacyclic_binary.  This model does neither: it reads the mask words off seeded.chacha20_block
block by block at the position the header states, and forms a (*) s1 coefficient by coefficient from the signs of
X^N = -1 (one key index at a time, an index gather, no extended row).  keygen_model (KM) supplies the long-double
sampler, the borderline rule, compare_words and noise_report; packing_keygen_model (PKM) the `_coeff_order` noise
layout of the BSK generators.  What is restated here is the little that is this format's own:
  * the nonce (g & 0xffffffff, g >> 32, domain) of group g = first_group + m, no stream number;
  * the domains "ERL" (masks under S) and "ERN" (noise under K);
  * the body b = a (*) s1 + e + plain, the slots at or past `count` encrypting 0;
  * recover_noise, which reads e off ciphertexts with the secret key and the plaintext alone.

`alter` names a deliberately wrong variant (test_packed_encrypt_host.py shows that each fails its check):
    "ignore_high"             the high nonce word (g >> 32) is forgotten
    "noise_from_mask_domain"  the noise is drawn from the mask's domain word
    "same_pair"               g1 of every Box-Muller pair is written as g0
    "plain_next_group"        the plaintext of group m is added to group m + 1 (cyclically)
"""
from __future__ import annotations

import numpy as np

import keygen_model as KM
import packing_keygen_model as PKM
from rs_tfhe_amd import seeded as S
from rs_tfhe_amd.params import N

DOMAIN_MASK, DOMAIN_NOISE = 0x45524C, 0x45524E  # "ERL", "ERN"
K = KM.GEN_KEY
SEED = bytes((59 * i + 23) & 0xFF for i in range(32))  # the public mask seed S of the tests
HIGH = (1 << 32) + 0xFFFFFFFE  # a first_group whose groups cross a carry of the low nonce word
FIRST = (0, HIGH)
COUNTS = (1, N - 1, N, N + 1, 3 * N + 5, 65 * N)
ALPHA = KM.ALPHA_BSK  # alpha_lv1 of SECURITY_128_BIT
ALTERS = ("ignore_high", "noise_from_mask_domain", "same_pair", "plain_next_group")


def groups_of(count: int) -> int:
    return -(-int(count) // N)


def group_indices(first_group: int, groups: int) -> np.ndarray:
    return np.uint64(int(first_group)) + np.arange(groups, dtype=np.uint64)


def _nonce(idx, alter):
    g = np.asarray(idx, np.uint64).reshape(-1)
    lo, hi = g & np.uint64(0xFFFFFFFF), g >> np.uint64(32)
    if alter == "ignore_high":
        hi = np.zeros_like(hi)
    return lo, hi


def masks(seed: bytes, idx, alter=None) -> np.ndarray:
    """[groups][N]: coefficient c is word c % 16 of the block with counter c / 16 of (g lo, g hi, "ERL")"""
    lo, hi = _nonce(idx, alter)
    out = np.empty((len(lo), N), np.uint32)
    for blk in range(N // 16):
        out[:, 16 * blk:16 * blk + 16] = S.chacha20_block(seed, blk, lo, hi, DOMAIN_MASK)
    return out


def noise(rng_key: bytes, idx, alpha: float, alter=None, chunk: int = 128) -> KM.Noise:
    """Noise polynomials [groups, N]: blocks 2 lane + h of (g lo, g hi, "ERN"), pair q of a block -> coefficients
    lane + 64 (4h + q) (g0) and + 512 (g1)"""
    lo, hi = _nonce(idx, alter)
    domain = DOMAIN_MASK if alter == "noise_from_mask_domain" else DOMAIN_NOISE
    out = KM.Noise(np.zeros((len(lo), N), np.uint32), np.zeros((len(lo), N), np.uint32), np.zeros((len(lo), N), bool))
    for at in range(0, len(lo), chunk):
        sl = slice(at, at + chunk)
        w = S.chacha20_block(rng_key, np.arange(128, dtype=np.uint64), lo[sl, None], hi[sl, None], domain)
        w = w.reshape(w.shape[0], 64, 2, 4, 4)  # [groups, lane, h, q, word]
        g0, g1 = S.gauss2(w, alpha)
        x0, x1, l0, l1 = KM.gauss2_ld(w, alpha)
        if alter == "same_pair":
            g1, x1, l1 = g0, x0, l0
        out.words[sl] = PKM._pairs_to_poly(S.f64_to_torus(g0), S.f64_to_torus(g1))
        out.ld_words[sl] = PKM._pairs_to_poly(KM.ld_to_torus(x0), KM.ld_to_torus(x1))
        out.border[sl] = PKM._pairs_to_poly(KM.borderline(x0, l0, alpha), KM.borderline(x1, l1, alpha))
    return out


def ring_product(a: np.ndarray, s1) -> np.ndarray:
    """a (*) s1 mod X^N + 1, wrapping u32: (a s)[c] = sum_j s[j] a[c - j], the terms with j > c negated"""
    s1 = np.asarray(s1, np.uint32).reshape(N)
    c = np.arange(N)
    out = np.zeros(a.shape, np.uint32)
    with np.errstate(over="ignore"):
        for j in np.flatnonzero(s1):
            term = a[:, (c - j) % N] * s1[j]
            out += np.where(c >= j, term, np.uint32(0) - term)
    return out


def slots(plain, count: int, alter=None) -> np.ndarray:
    """[groups][N]: slot j of group m is plain[m N + j], zero at or past `count`"""
    groups = groups_of(count)
    msg = np.zeros(groups * N, np.uint32)
    msg[:count] = np.asarray(plain, np.uint32).reshape(-1)[:count]
    msg = msg.reshape(groups, N)
    return np.roll(msg, 1, axis=0) if alter == "plain_next_group" else msg


def encrypt(s1, plain, count: int, first_group: int, alpha: float, mask_seed: bytes = SEED, rng_key: bytes = K, alter=None):
    """tfhe_hip_batch_encrypt_trlwe's full form: (words [groups][2][N], border [groups][2][N]); only a body word can be
    borderline"""
    idx = group_indices(first_group, groups_of(count))
    a = masks(mask_seed, idx, alter)
    e = noise(rng_key, idx, alpha, alter)
    out = np.empty((len(idx), 2, N), np.uint32)
    out[:, 0] = a
    with np.errstate(over="ignore"):
        out[:, 1] = ring_product(a, s1) + e.words + slots(plain, count, alter)
    border = np.zeros(out.shape, bool)
    border[:, 1] = e.border
    return out, border


def recover_noise(s1, packed, plain, count: int):
    """(e, a): e = B - A (*) s1 - plain as [groups, N] int32 and the masks; the secret key and the plaintext alone"""
    packed = np.asarray(packed, np.uint32).reshape(-1, 2, N)
    with np.errstate(over="ignore"):
        e = packed[:, 1] - ring_product(packed[:, 0], s1) - slots(plain, count)
    return e.view(np.int32), packed[:, 0]


def plaintexts(count: int, tag: int) -> np.ndarray:
    """random torus words with 0xFFFFFFFF / 0x80000000 planted at every group's first and last slot, so that a slot taken
    from the neighbouring group shows"""
    p = np.random.default_rng(9100 + tag).integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
    first = np.arange(0, count, N)
    p[first] = np.where((first // N) % 2 == 0, 0xFFFFFFFF, 0x80000000).astype(np.uint32)
    last = np.minimum(first + N - 1, count - 1)
    p[last] = np.where((first // N) % 2 == 0, 0x80000000, 0xFFFFFFFF).astype(np.uint32)
    return p


def keys():
    """the level-1 keys of the tests: random, all ones, all zeros, a single last 1"""
    one_last = np.zeros(N, np.uint32)
    one_last[N - 1] = 1
    return {"random": np.random.default_rng(9001).integers(0, 2, N, dtype=np.uint32), "ones": np.ones(N, np.uint32),
            "zeros": np.zeros(N, np.uint32), "last": one_last}
