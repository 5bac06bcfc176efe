"""A numpy model of the packed CMUX (include/tfhe_hip.h, "packed CMUX"; csrc/cmux.hpp).  No test functions.

Everything the section defines, in integers:
  * the digits u_i / d_i of a word for any (beta, t) of the box, rounding or (reference=True) truncating, straight from
    the header's formula -- no carry chain, unlike trlwe_switch_model.digits, which test_cmux_host.py holds it equal to;
  * the external product and the CMUX.  The products sum_i D_i (*) row_i have |digit| <= 64 and 2t N <= 65,536 terms of
    u32 words: below 2^54 in int64.  `external_product` runs them row by row as float64 matmuls of the digits with the
    16-bit halves of the row's negacyclic matrix (|sums| < 2^6 2^16 2^10: exact; BLAS speed, which the chunk-crossing
    GPU case needs), `external_product_int64` as int64 sums term by term for ONE ciphertext;
  * TRGSW encryption from (K, s1, mu): S = block(K, 0, (0, 30, "DES"))[:8], the mask words read off
    seeded.chacha20_block block by block under (r lo, r hi, "EGL"), the noise under (r lo, r hi, "EGN") in the BSK
    generators' word order with keygen_model's long-double sampler and borderline rule, the product a (*) s1 term by
    term (packed_encrypt_model.ring_product), and the gadget polynomial added after the body.

`alter` names a deliberately wrong variant (test_cmux_host.py shows that the word comparison catches each):
    "gadget_before_body"  g_i mu is added to the a half BEFORE b = a (*) s1 + e is formed
    "swap_ab"             rows below t get the gadget on b, the rest on a
    "no_rnd"              the rounding constant is forgotten (cmux / external_product)
    "d0_minus_d1"         x = d0 - d1 (cmux)
"""
from __future__ import annotations

import numpy as np

import keygen_model as KM
import packed_encrypt_model as PEM
import packing_keygen_model as PKM
from rs_tfhe_amd import seeded as S
from rs_tfhe_amd.params import N

DOMAIN_MASK, DOMAIN_NOISE = 0x45474C, 0x45474E  # "EGL", "EGN"
SEED_STREAM = 30
REFERENCE_DIGITS = 1  # TFHE_HIP_CMUX_REFERENCE_DIGITS
SHAPES = ((6, 3), (4, 6), (7, 4), (2, 16), (1, 32))  # (beta, t) of the GPU word tests
CHUNK = 2048  # kCmuxChunk
ALTERS_ENCRYPT = ("gadget_before_body", "swap_ab")
ALTERS_CMUX = ("no_rnd", "d0_minus_d1")


def check_shape(basebit: int, t: int) -> None:
    if not (1 <= basebit <= 7 and 1 <= t <= 32 and basebit * t <= 32):
        raise ValueError("1 <= basebit <= 7, 1 <= t <= 32, basebit * t <= 32")


def gadget(basebit: int, t: int) -> np.ndarray:
    """g_i = 2^(32 - beta (i+1)), i < t, as u32."""
    return np.array([1 << (32 - (i + 1) * basebit) for i in range(t)], np.uint32)


def offset(basebit: int, t: int) -> int:
    """off = sum_i 2^(beta-1) g_i (gen_decomposition_offset of the reference)"""
    return sum((1 << (basebit - 1)) << (32 - (i + 1) * basebit) for i in range(t)) & 0xFFFFFFFF


def rounding(basebit: int, t: int, reference: bool = False) -> int:
    """rnd = 2^(31 - beta t) when beta t < 32, else 0; 0 with the reference's digits"""
    bt = basebit * t
    return 0 if reference or bt >= 32 else 1 << (31 - bt)


def digits(words, basebit: int, t: int, reference: bool = False) -> np.ndarray:
    """d_i(w) = (((w + off + rnd) >> (32 - beta (i+1))) & (2^beta - 1)) - 2^(beta-1): [..., t] int8"""
    check_shape(basebit, t)
    w = (np.asarray(words, np.uint32).astype(np.uint64) + np.uint64(offset(basebit, t) + rounding(basebit, t, reference))) & np.uint64(0xFFFFFFFF)
    out = np.empty(w.shape + (t,), np.int8)
    for i in range(t):
        u = (w >> np.uint64(32 - basebit * (i + 1))) & np.uint64((1 << basebit) - 1)
        out[..., i] = (u.astype(np.int64) - (1 << (basebit - 1))).astype(np.int8)
    return out


def _negacyclic_matrix(p) -> np.ndarray:
    """T[m][i] = ext_p[i - m]: p[i - m] for i >= m, 0 - p[N + i - m] for i < m; (D (*) p)[i] = sum_m D[m] T[m][i].  u32"""
    p = np.asarray(p, np.uint32)
    d = np.arange(N)[None, :] - np.arange(N)[:, None]
    with np.errstate(over="ignore"):
        return np.where(d >= 0, p[d % N], np.uint32(0) - p[d % N])


class Selector:
    """The products under one TRGSW [2t][2][N]: each row's negacyclic matrix is built once, as its two 16-bit halves."""

    def __init__(self, rows, basebit: int, t: int):
        check_shape(basebit, t)
        self.basebit, self.t = basebit, t
        self.rows = np.asarray(rows, np.uint32).reshape(2 * t, 2, N).copy()
        self._halves = None

    def halves(self, r):
        T = np.concatenate([_negacyclic_matrix(self.rows[r, 0]), _negacyclic_matrix(self.rows[r, 1])], axis=1)  # [N][2N]
        return (T & 0xFFFF).astype(np.float64), (T >> 16).astype(np.float64)

    def external_product(self, x, reference: bool = False, alter=None) -> np.ndarray:
        """sum_{i<t} D_i(x.a) (*) row_i + D_i(x.b) (*) row_{t+i} on x [count][2][N]: [count][2][N] u32"""
        x = np.ascontiguousarray(x, np.uint32).reshape(-1, 2, N)
        t = self.t
        if alter == "no_rnd":
            reference = True
        d = digits(x, self.basebit, t, reference)  # [count][2][N][t]
        acc = np.zeros((len(x), 2 * N), np.int64)  # |acc| < 2t N 2^6 2^32 <= 2^54
        for r in range(2 * t):
            lo, hi = self.halves(r)
            dl = d[:, r // t, :, r % t].astype(np.float64)
            acc += (dl @ lo).astype(np.int64) + ((dl @ hi).astype(np.int64) << 16)  # |sums| < 2^6 2^16 2^10: exact
        return (acc & 0xFFFFFFFF).astype(np.uint32).reshape(len(x), 2, N)

    def cmux(self, d0, d1, reference: bool = False, alter=None) -> np.ndarray:
        """d0 + sel (.) (d1 - d0), or sel (.) d1 with d0 None"""
        d1 = np.ascontiguousarray(d1, np.uint32).reshape(-1, 2, N)
        if d0 is None:
            return self.external_product(d1, reference, alter)
        d0 = np.ascontiguousarray(d0, np.uint32).reshape(-1, 2, N)
        with np.errstate(over="ignore"):
            x = d0 - d1 if alter == "d0_minus_d1" else d1 - d0
            return d0 + self.external_product(x, reference, alter)


def external_product(rows, basebit: int, t: int, x, reference: bool = False) -> np.ndarray:
    return Selector(rows, basebit, t).external_product(x, reference)


def cmux(rows, basebit: int, t: int, d0, d1, reference: bool = False, alter=None) -> np.ndarray:
    return Selector(rows, basebit, t).cmux(d0, d1, reference, alter)


def external_product_int64(rows, basebit: int, t: int, x, reference: bool = False) -> np.ndarray:
    """The same for ONE ciphertext [2][N], as int64 sums of digit x word products, term by term (schoolbook)."""
    rows = np.asarray(rows, np.uint32).reshape(2 * t, 2, N).astype(np.int64)
    d = digits(np.asarray(x, np.uint32).reshape(2, N), basebit, t, reference).astype(np.int64)  # [2][N][t]
    acc = np.zeros((2, N), np.int64)
    for r in range(2 * t):
        dr = d[r // t, :, r % t]
        for m in np.nonzero(dr)[0]:
            for c in range(2):
                v = np.roll(rows[r, c], m)
                v[:m] = -v[:m]
                acc[c] += dr[m] * v
    return (acc & 0xFFFFFFFF).astype(np.uint32)


# ---- TRGSW encryption ----------------------------------------------------------------------------------------------------
def mask_seed(K: bytes) -> bytes:
    """S = words 0..7 of block(K, counter 0, nonce (0, 30, "DES"))"""
    return S.chacha20_block(K, 0, 0, SEED_STREAM, S.DOMAIN_SEED)[:8].astype("<u4").tobytes()


def row_indices(first_index: int, count: int, t: int) -> np.ndarray:
    """r = first_index + m 2t + row, as u64 [count 2t]"""
    return np.uint64(int(first_index)) + np.arange(count * 2 * t, dtype=np.uint64)


def masks(seed: bytes, idx) -> np.ndarray:
    """[rows][N]: coefficient c is word c % 16 of the block with counter c / 16 of (r lo, r hi, "EGL")"""
    r = np.asarray(idx, np.uint64).reshape(-1)
    lo, hi = r & np.uint64(0xFFFFFFFF), r >> np.uint64(32)
    out = np.empty((len(r), N), np.uint32)
    for blk in range(N // 16):
        out[:, 16 * blk:16 * blk + 16] = S.chacha20_block(seed, blk, lo, hi, DOMAIN_MASK)
    return out


def noise(K: bytes, idx, alpha: float, chunk: int = 128) -> KM.Noise:
    """[rows][N]: blocks 2 lane + h of (r lo, r hi, "EGN"), pair q of a block -> coefficients lane + 64 (4h + q) (g0) and
    + 512 (g1)"""
    r = np.asarray(idx, np.uint64).reshape(-1)
    lo, hi = r & np.uint64(0xFFFFFFFF), r >> np.uint64(32)
    out = KM.Noise(np.zeros((len(r), N), np.uint32), np.zeros((len(r), N), np.uint32), np.zeros((len(r), N), bool))
    for at in range(0, len(r), chunk):
        sl = slice(at, at + chunk)
        w = S.chacha20_block(K, np.arange(128, dtype=np.uint64), lo[sl, None], hi[sl, None], DOMAIN_NOISE)
        w = w.reshape(w.shape[0], 64, 2, 4, 4)
        g0, g1 = S.gauss2(w, alpha)
        x0, x1, l0, l1 = KM.gauss2_ld(w, alpha)
        out.words[sl] = PKM._pairs_to_poly(S.f64_to_torus(g0), S.f64_to_torus(g1))
        out.ld_words[sl] = PKM._pairs_to_poly(KM.ld_to_torus(x0), KM.ld_to_torus(x1))
        out.border[sl] = PKM._pairs_to_poly(KM.borderline(x0, l0, alpha), KM.borderline(x1, l1, alpha))
    return out


def encrypt_trgsw(s1, mu, basebit: int, t: int, alpha: float, K: bytes, first_index: int = 0, alter=None):
    """tfhe_hip_batch_encrypt_trgsw: (words [count][2t][2][N], border the same shape, S); only a b word can be
    borderline.  mu: [count][N] small integers."""
    check_shape(basebit, t)
    mu = np.asarray(mu, np.int64).reshape(-1, N)
    count = len(mu)
    seed = mask_seed(K)
    idx = row_indices(first_index, count, t)
    a = masks(seed, idx)
    e = noise(K, idx, alpha)
    g = gadget(basebit, t).astype(np.int64)
    add = ((g[None, :, None] * mu[:, None, :]) & 0xFFFFFFFF).astype(np.uint32)  # [count][t][N]
    zero = np.zeros_like(add)
    on_a = np.concatenate([add, zero], axis=1).reshape(count * 2 * t, N)  # rows below t
    on_b = np.concatenate([zero, add], axis=1).reshape(count * 2 * t, N)
    if alter == "swap_ab":
        on_a, on_b = on_b, on_a
    out = np.empty((count * 2 * t, 2, N), np.uint32)
    with np.errstate(over="ignore"):
        if alter == "gadget_before_body":
            a = a + on_a
            out[:, 0] = a
            out[:, 1] = PEM.ring_product(a, s1) + e.words + on_b
        else:
            out[:, 0] = a + on_a
            out[:, 1] = PEM.ring_product(a, s1) + e.words + on_b
    border = np.zeros(out.shape, bool)
    border[:, 1] = e.border
    return out.reshape(count, 2 * t, 2, N), border.reshape(count, 2 * t, 2, N), seed


def phase(ct, s) -> np.ndarray:
    """b - a (*) s of [..., 2, N] under the binary ring key s: [..., N] u32"""
    ct = np.asarray(ct, np.uint32)
    a = ct[..., 0, :].reshape(-1, N)
    with np.errstate(over="ignore"):
        return (ct[..., 1, :].reshape(-1, N) - S.negacyclic_binary(a, np.asarray(s, np.uint32).reshape(N))).reshape(ct.shape[:-2] + (N,))


# ---- the noise of one CMUX, in torus units squared, per coefficient -----------------------------------------------------------
def cmux_variance(basebit: int, t: int, alpha: float, mu: int = 1, ones: float = N / 2) -> float:
    """2t N digits of variance B^2 / 12 times a selector noise sample of variance alpha^2, and for mu = 1 the rounding
    of the words of x.b (1) and of x.a against the key's `ones` coefficients, each uniform over one step 2^(-beta t)"""
    rnd = 0.0 if basebit * t >= 32 else (1.0 + ones) * 2.0 ** (-2 * basebit * t) / 12.0
    return 2 * t * N * (4.0 ** basebit / 12.0) * alpha * alpha + mu * rnd


def lookup_sigma(basebit: int, t: int, alpha_sel: float, alpha_in: float, levels: int) -> float:
    """standard deviation of a slot's phase error after `levels` CMUX levels on a fresh encryption at alpha_in (every
    level adds one CMUX's noise at mu = 1, the larger case)"""
    return float(np.sqrt(alpha_in ** 2 + levels * cmux_variance(basebit, t, alpha_sel, 1)))
