"""A CPU model of symmetric encryption in the keyed format of include/tfhe_hip.h ("symmetric encryption"): bulk TLWE
lv0 ciphertexts, the rows of the public key and the rows of the symmetric re-encryption key.  No test functions.

The package's CPU form (rs_tfhe_amd.seeded.symmetric_rows) multiplies the masks into the key; the kernel walks keystream
blocks lane by lane and reduces with shuffles.  This model does neither: it reads the mask words off
seeded.chacha20_block block by block at the position the header states and adds the words the key selects one column at
a time, wrapping u32.  keygen_model (KM) supplies the long-double sampler and the borderline rule for the one noise
sample a row has.

`alter` names a deliberately wrong variant (test_sym_encrypt_host.py shows that each fails its check):
    "noise_from_mask_domain"  the noise is drawn from the mask's domain word
    "no_row"                  the row index is dropped from the nonce
    "ignore_high"             the high nonce word (g >> 32) is ignored
    "k0_not_zero"             the k = 0 rows of the re-encryption key are encrypted like the others
"""
from __future__ import annotations

import numpy as np

import keygen_model as KM
import pk_encrypt_model as PM
from rs_tfhe_amd import seeded as S
from rs_tfhe_amd.params import SecurityParams

TLWE = (0x45574C, 0x45574E)  # "EWL", "EWN"
PK = (0x504B4D, 0x504B5A)  # "PKM", "PKZ"
RK = (0x524B4D, 0x524B53)  # "RKM", "RKS"
K = KM.GEN_KEY
SEED = bytes((101 * i + 7) & 0xFF for i in range(32))  # the public mask seed S of the tests
HIGH = PM.HIGH
SHAPES = ((33, 3, 6, 2, 9), (16, 1, 22, 5, 3), (48, 2, 10, 2, 8))  # tail block, exactly one block, whole blocks
COUNTS = (1, 5, 257, 4099)
FIRST = (0, HIGH)
ALPHA = KM.ALPHA_KSK


def _nonce(rows, alter):
    g = np.asarray(rows, np.uint64).reshape(-1)
    lo, hi = g & np.uint64(0xFFFFFFFF), g >> np.uint64(32)
    if alter == "no_row":
        lo, hi = np.zeros_like(lo), np.zeros_like(hi)
    if alter == "ignore_high":
        hi = np.zeros_like(hi)
    return lo, hi


def masks(key: bytes, rows, n: int, domain: int, alter=None) -> np.ndarray:
    """[rows][n]: mask word x is word x % 16 of the block with counter x / 16 of (g & 0xffffffff, g >> 32, domain)"""
    lo, hi = _nonce(rows, alter)
    out = np.empty((len(lo), n), np.uint32)
    for blk in range((n + 15) // 16):
        w = S.chacha20_block(key, blk, lo, hi, domain)  # [rows, 16]
        take = min(16, n - 16 * blk)
        out[:, 16 * blk:16 * blk + take] = w[:, :take]
    return out


def noise(key: bytes, rows, alpha: float, domain: int, alter=None) -> KM.Noise:
    """One sample a row: g0 of gauss2(words 0..3 of block 0 of (g & 0xffffffff, g >> 32, domain))"""
    lo, hi = _nonce(rows, alter)
    w = S.chacha20_block(key, 0, lo, hi, domain)[:, :4]
    g0, _ = S.gauss2(w, alpha)
    x0, _, l0, _ = KM.gauss2_ld(w, alpha)
    return KM.Noise(S.f64_to_torus(g0), KM.ld_to_torus(x0), KM.borderline(x0, l0, alpha))


def inner(a: np.ndarray, s0) -> np.ndarray:
    """<a, s0>, one column at a time, wrapping u32"""
    s0 = np.asarray(s0, np.uint32).reshape(-1)
    acc = np.zeros(len(a), np.uint32)
    with np.errstate(over="ignore"):
        for x in np.flatnonzero(s0):
            acc += a[:, x] * s0[x]
    return acc


def encrypt(mask_key: bytes, rng_key: bytes, rows, s0, plain, alpha: float, domains, alter=None):
    """(words [rows][n+1], border [rows][n+1]): the rows `rows` of the format; only a body can be borderline"""
    n = len(np.asarray(s0).reshape(-1))
    a = masks(mask_key, rows, n, domains[0], alter)
    e = noise(rng_key, rows, alpha, domains[0] if alter == "noise_from_mask_domain" else domains[1], alter)
    out = np.empty((len(a), n + 1), np.uint32)
    out[:, :-1] = a
    with np.errstate(over="ignore"):
        out[:, -1] = inner(a, s0) + np.broadcast_to(np.asarray(plain, np.uint32).reshape(-1), (len(a),)) + e.words
    border = np.zeros(out.shape, bool)
    border[:, -1] = e.border
    return out, border


def bulk(s0, plain, first_index: int, alpha: float, mask_seed: bytes = SEED, rng_key: bytes = K, alter=None):
    """tfhe_hip_batch_encrypt's full form"""
    return encrypt(mask_seed, rng_key, PM.row_indices(first_index, len(plain)), s0, plain, alpha, TLWE, alter)


def public_key(s0, size: int, alpha: float, rng_key: bytes = K, alter=None):
    """tfhe_hip_gen_public_key's encryptions_out [size][n+1]"""
    return encrypt(rng_key, rng_key, np.arange(size, dtype=np.uint64), s0, 0, alpha, PK, alter)


def reenc_key(p: SecurityParams, key_from, key_to, alpha: float, rng_key: bytes = K, alter=None):
    """tfhe_hip_gen_reenc_key_symmetric's key_out [n t base][n+1]: the k = 0 rows zero, their streams unused"""
    rows = np.arange(p.n * p.iks_t * p.base, dtype=np.uint64)
    live = (rows % np.uint64(p.base)) != 0
    if alter == "k0_not_zero":
        live = np.ones(len(rows), bool)
    out = np.zeros((len(rows), p.n + 1), np.uint32)
    border = np.zeros(out.shape, bool)
    out[live], border[live] = encrypt(rng_key, rng_key, rows[live], key_to, PM.reenc_plaintexts(p, key_from)[live], alpha,
                                      RK, alter)
    return out, border


def plaintexts(count: int, tag: int) -> np.ndarray:
    return np.random.default_rng(7000 + tag).integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
