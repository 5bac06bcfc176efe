"""A numpy model of the TRLWE key switch (include/tfhe_hip.h, "TRLWE key switch"; csrc/trlwe_switch.hpp).  No test
functions.

Everything the section defines, in integers:
  * psi_k, the automorphism X -> X^k on N = 1024 wrapping u32 coefficients;
  * the digits of a word for any (beta, t) with beta t <= 32 (packing.digits takes its (beta, t) from a parameter set and
    has no beta t = 32);
  * the switching key from (S, K, secrets): masks under (64 k + l, 27, "TKS") with the vectorised ChaCha20 of
    rs_tfhe_amd.seeded, noise under (64 k + l, 28, "TKS") in the BSK generators' word order (keygen_model supplies the
    long-double sampler and the borderline rule), S = block(K, 0, (0, 29, "DES"))[:8], bodies
    b_l = a_l (*) s_to + e_l + g_l psi_k(s_from);
  * the switch.  The products sum_l D_l (*) K_l have |digit| <= 64 and 1,024 t <= 32,768 terms of u32 words: below 2^53
    in int64.  `switch` runs them row by row as float64 matmuls of the digits with the 16-bit halves of the key row's
    negacyclic matrix (|sums| < 2^32: exact; BLAS speed, which the chunk-crossing GPU case needs) summed in int64,
    `switch_int64` as plain int64 sums term by term; test_trlwe_switch_host.py holds the two equal.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import keygen_model as KM
from rs_tfhe_amd import seeded as S
from rs_tfhe_amd.params import N

DOMAIN = 0x544B53  # "TKS"
MASK_STREAM, NOISE_STREAM, SEED_STREAM = 27, 28, 29
KS = (1, 3, 513, 1025, 2047)  # the automorphisms the tests walk: identity, a small one, N/2 + 1, N + 1, 2N - 1
SHAPES = ((4, 6), (7, 3), (7, 4), (2, 16), (1, 32))  # (beta, t)


def check_shape(k: int, basebit: int, t: int) -> None:
    if not (1 <= k < 2 * N and k & 1):
        raise ValueError("k must be odd, 1 <= k < 2N")
    if not (1 <= basebit <= 7 and 1 <= t <= 64 and basebit * t <= 32):
        raise ValueError("1 <= basebit <= 7, 1 <= t <= 64, basebit * t <= 32")


def psi(p, k: int) -> np.ndarray:
    """psi_k on the last axis: coefficient j goes to position j k mod 2N; a position >= N is position - N, negated."""
    p = np.asarray(p, np.uint32)
    j = np.arange(N)
    pos = (j * k) % (2 * N)
    out = np.empty_like(p)
    with np.errstate(over="ignore"):
        out[..., pos % N] = np.where(pos >= N, np.uint32(0) - p, p)
    return out


def a_bar(words, basebit: int, t: int) -> np.ndarray:
    """The rounding: ((x + 2^(31 - beta t)) mod 2^32) >> (32 - beta t); x itself at beta t = 32.  u64."""
    bt = basebit * t
    a = np.asarray(words, np.uint32).astype(np.uint64)
    rnd = np.uint64(1 << (31 - bt)) if bt < 32 else np.uint64(0)
    return ((a + rnd) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bt)


def digits(words, basebit: int, t: int) -> np.ndarray:
    """The signed digits d_l of the definition, [..., t] int8, d_l in [-B/2, B/2): the base-B decomposition of a_bar
    from the least significant digit up with a carry into the next (the last carry dropped)."""
    base = 1 << basebit
    ab = a_bar(words, basebit, t)
    out = np.empty(ab.shape + (t,), np.int8)
    carry = np.zeros(ab.shape, np.int64)
    for l in range(t - 1, -1, -1):
        v = ((ab >> np.uint64(basebit * (t - 1 - l))) & np.uint64(base - 1)).astype(np.int64) + carry
        neg = v >= base // 2
        out[..., l] = np.where(neg, v - base, v)
        carry = neg.astype(np.int64)
    return out


def gadget(basebit: int, t: int) -> np.ndarray:
    """g_l = 2^(32 - (l+1) beta), l < t, as u32."""
    return np.array([1 << (32 - (l + 1) * basebit) for l in range(t)], np.uint32)


# ---- the key ---------------------------------------------------------------------------------------------------------
def mask_seed(K: bytes) -> bytes:
    """S = words 0..7 of block(K, counter 0, nonce (0, 29, "DES"))"""
    return S.chacha20_block(K, 0, 0, SEED_STREAM, S.DOMAIN_SEED)[:8].astype("<u4").tobytes()


def nonce_rows(k: int, t: int) -> np.ndarray:
    return (64 * k + np.arange(t)).astype(np.uint64)


def key_masks(seed: bytes, k: int, t: int) -> np.ndarray:
    """a_l, natural order: [t, N] u32"""
    return S.keystream(seed, N, nonce_rows(k, t), MASK_STREAM, DOMAIN)


def key_noise(K: bytes, k: int, t: int, alpha: float) -> KM.Noise:
    """e_l as KM.Noise (f64 words, long-double words, the borderline marks), [t, N]: blocks 2 lane + h of
    (64 k + l, 28, "TKS"), pair m < 4 of a block gives e[lane + 64 (4h + m)] and the same + 512."""
    w = S.chacha20_block(K, np.arange(128, dtype=np.uint64), nonce_rows(k, t)[:, None], NOISE_STREAM, DOMAIN)
    w = w.reshape(t, 64, 2, 4, 4)
    g0, g1 = S.gauss2(w, alpha)
    x0, x1, l0, l1 = KM.gauss2_ld(w, alpha)
    return KM.Noise(KM._pairs_to_poly(S.f64_to_torus(g0), S.f64_to_torus(g1)),
                    KM._pairs_to_poly(KM.ld_to_torus(x0), KM.ld_to_torus(x1)),
                    KM._pairs_to_poly(KM.borderline(x0, l0, alpha), KM.borderline(x1, l1, alpha)))


@dataclass
class Key:
    k: int
    basebit: int
    t: int
    mask_seed: bytes
    bodies: np.ndarray  # [t][N] u32
    border: np.ndarray  # [t][N] bool: noise samples within rounding of a torus step


def bodies_from(seed: bytes, s_from, s_to, k: int, basebit: int, t: int, e) -> np.ndarray:
    """b_l = a_l (*) s_to + e_l + g_l psi_k(s_from), the gadget polynomial after the product, wrapping"""
    s_from = np.asarray(s_from, np.uint32).reshape(N)
    s_to = np.asarray(s_to, np.uint32).reshape(N)
    with np.errstate(over="ignore"):
        b = S.negacyclic_binary(key_masks(seed, k, t), s_to) + np.asarray(e, np.uint32)
        b += gadget(basebit, t)[:, None] * psi(s_from, k)[None, :]
    return b


def make_key(s_from, s_to, k: int, basebit: int, t: int, K: bytes, alpha: float) -> Key:
    """tfhe_hip_gen_trlwe_switch_key(K) on the CPU."""
    check_shape(k, basebit, t)
    seed = mask_seed(K)
    e = key_noise(K, k, t, alpha)
    return Key(k, basebit, t, seed, bodies_from(seed, s_from, s_to, k, basebit, t, e.words), e.border)


def key_rows(seed: bytes, k: int, t: int, bodies) -> np.ndarray:
    """[t][2][N]: a_l from S, b_l from the bodies -- what the handle holds"""
    out = np.empty((t, 2, N), np.uint32)
    out[:, 0] = key_masks(seed, k, t)
    out[:, 1] = np.asarray(bodies, np.uint32).reshape(t, N)
    return out


# ---- the switch --------------------------------------------------------------------------------------------------------
def _negacyclic_matrix(p) -> np.ndarray:
    """T[m][i] = ext_p[i - m]: p[i - m] for i >= m, 0 - p[N + i - m] for i < m; (D (*) p)[i] = sum_m D[m] T[m][i].  u32"""
    p = np.asarray(p, np.uint32)
    d = np.arange(N)[None, :] - np.arange(N)[:, None]
    with np.errstate(over="ignore"):
        return np.where(d >= 0, p[d % N], np.uint32(0) - p[d % N])


class Switcher:
    """The switch under one key: rows [t][2][N].  The matrices are built a row at a time (32 rows would be 1 GB)."""

    def __init__(self, rows, k: int, basebit: int, t: int):
        check_shape(k, basebit, t)
        self.k, self.basebit, self.t = k, basebit, t
        self.rows = np.asarray(rows, np.uint32).reshape(t, 2, N).copy()

    def __call__(self, cts) -> np.ndarray:
        cts = np.ascontiguousarray(cts, np.uint32).reshape(-1, 2, N)
        ap, bp = psi(cts[:, 0], self.k), psi(cts[:, 1], self.k)
        d = digits(ap, self.basebit, self.t)  # [count][N][t] int8
        acc = np.zeros((len(cts), 2 * N), np.int64)  # < t 2^48 <= 2^53
        for l in range(self.t):
            T = np.concatenate([_negacyclic_matrix(self.rows[l, 0]), _negacyclic_matrix(self.rows[l, 1])], axis=1)  # [N][2N]
            lo, hi = (T & 0xFFFF).astype(np.float64), (T >> 16).astype(np.float64)
            dl = d[:, :, l].astype(np.float64)
            acc += (dl @ lo).astype(np.int64) + ((dl @ hi).astype(np.int64) << 16)  # |sums| < 2^6 2^16 2^10: exact
        acc = (acc & 0xFFFFFFFF).astype(np.uint32).reshape(len(cts), 2, N)
        out = np.empty_like(cts)
        with np.errstate(over="ignore"):
            out[:, 0] = np.uint32(0) - acc[:, 0]
            out[:, 1] = bp - acc[:, 1]
        return out


def switch(rows, k: int, basebit: int, t: int, cts) -> np.ndarray:
    """out.a = - sum_l D_l (*) a_l, out.b = psi_k(b) - sum_l D_l (*) b_l for cts [count][2][N]: [count][2][N] u32"""
    return Switcher(rows, k, basebit, t)(cts)


def switch_int64(rows, k: int, basebit: int, t: int, ct) -> np.ndarray:
    """The same for ONE ciphertext [2][N], as int64 sums of digit x word products (< 2^53), term by term."""
    rows = np.asarray(rows, np.uint32).reshape(t, 2, N).astype(np.int64)
    ct = np.asarray(ct, np.uint32).reshape(2, N)
    ap, bp = psi(ct[0], k), psi(ct[1], k)
    d = digits(ap, basebit, t).astype(np.int64)  # [N][t]
    acc = np.zeros((2, N), np.int64)
    for l in range(t):
        for m in np.nonzero(d[:, l])[0]:
            for c in range(2):
                r = np.roll(rows[l, c], m)
                r[:m] = -r[:m]
                acc[c] += d[m, l] * r
    out = np.empty((2, N), np.uint32)
    out[0] = ((-acc[0]) & 0xFFFFFFFF).astype(np.uint32)
    out[1] = ((bp.astype(np.int64) - acc[1]) & 0xFFFFFFFF).astype(np.uint32)
    return out


def phase(ct, s) -> np.ndarray:
    """b - a (*) s of [..., 2, N] under the binary ring key s: [..., N] u32"""
    ct = np.asarray(ct, np.uint32)
    a = ct[..., 0, :].reshape(-1, N)
    with np.errstate(over="ignore"):
        return (ct[..., 1, :].reshape(-1, N) - S.negacyclic_binary(a, np.asarray(s, np.uint32).reshape(N))).reshape(ct.shape[:-2] + (N,))


# ---- the noise of one switch, in torus units squared, per coefficient ---------------------------------------------------
def rounding_variance(basebit: int, t: int, ones: float = N / 2) -> float:
    """`ones` key coefficients times the variance of a word's rounding, uniform over one step 2^(-beta t) of the torus;
    nothing is rounded at beta t = 32"""
    return 0.0 if basebit * t >= 32 else ones * 2.0 ** (-2 * basebit * t) / 12.0


def key_noise_variance(basebit: int, t: int, alpha: float) -> float:
    """N t digits of variance B^2 / 12 times a key noise sample of variance alpha^2"""
    return N * t * (4.0 ** basebit / 12.0) * alpha * alpha


def switch_variance(basebit: int, t: int, alpha: float, ones: float = N / 2) -> float:
    return rounding_variance(basebit, t, ones) + key_noise_variance(basebit, t, alpha)


def trace_keys(steps: int):
    """k_s = N / 2^(s-1) + 1, s = 1 .. steps"""
    return [N // (1 << (s - 1)) + 1 for s in range(1, steps + 1)]


def trace(switchers, ct) -> np.ndarray:
    """ct <- ct + switch_{k_s}(ct), s = 1 .. len(switchers), on [count][2][N]"""
    ct = np.ascontiguousarray(ct, np.uint32).reshape(-1, 2, N).copy()
    with np.errstate(over="ignore"):
        for sw in switchers:
            ct = ct + sw(ct)
    return ct
