"""Seeded (compressed) cloud keys and ciphertexts on the host: numpy only, no device.

The format is the normative one of include/tfhe_hip.h ("seeded (compressed) cloud keys and ciphertexts"): every mask
word is a fixed position of a ChaCha20 keystream (RFC 8439 block function) under a public 32-byte mask seed S, so
only the bodies travel.  This module is the client's side of it -- a vectorised ChaCha20, the compressor that makes
the bodies from the secret key (exact integer arithmetic: s1 is binary, so a negacyclic product is a sum of rotated
rows), and the CPU expansion of seeded ciphertexts.  The GPU kernels of csrc/seeded.hpp compute the same words.
"""
from __future__ import annotations

import numpy as np

from .params import N, SecurityParams, gen_decomposition_offset

DOMAIN_KSK = 0x4B534B
DOMAIN_BSK = 0x42534B
DOMAIN_TLWE = 0x45574C
DOMAIN_SEED = 0x444553
# symmetric encryption (include/tfhe_hip.h): (mask domain, noise domain) of the three uses; the index g of a row is 64
# bits and rides in the nonce (g & 0xffffffff, g >> 32, domain)
DOMAINS_SYM_TLWE = (DOMAIN_TLWE, 0x45574E)  # "EWL" masks under the public seed S, "EWN" noise under K
DOMAINS_SYM_PK = (0x504B4D, 0x504B5A)       # "PKM", "PKZ": rows of the public key, both under K
DOMAINS_SYM_RK = (0x524B4D, 0x524B53)       # "RKM", "RKS": rows of the symmetric re-encryption key, both under K
# packed encryption (include/tfhe_hip.h): groups of N slots, indexed like the rows above
DOMAINS_TRLWE = (0x45524C, 0x45524E)        # "ERL" mask polynomials under the public seed S, "ERN" noise under K
DOMAINS_TRGSW = (0x45474C, 0x45474E)        # "EGL", "EGN": the same for the rows of TRGSW selectors ("packed CMUX")
_SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
_QR = ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15),
       (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))


def key_words(key: bytes) -> np.ndarray:
    """32 bytes -> 8 little-endian u32 words (as the C ABI reads seeds and generator keys)."""
    key = bytes(key)
    if len(key) != 32:
        raise ValueError("ChaCha20 keys and mask seeds are 32 bytes")
    return np.frombuffer(key, dtype="<u4").astype(np.uint32)


def chacha20_block(key, counter, n0, n1, n2) -> np.ndarray:
    """RFC 8439 section 2.3 block function, vectorised: counter / n0 / n1 / n2 broadcast against each other; returns
    [..., 16] u32 keystream words."""
    kw = key_words(key) if isinstance(key, (bytes, bytearray)) else np.asarray(key, np.uint32)
    ctr, a, b, c = np.broadcast_arrays(*(np.asarray(v, np.uint64).astype(np.uint32) for v in (counter, n0, n1, n2)))
    shape = ctr.shape
    init = [np.full(shape, w, np.uint32) for w in _SIGMA] + [np.full(shape, w, np.uint32) for w in kw] + \
           [ctr.copy(), a.copy(), b.copy(), c.copy()]
    x = [v.copy() for v in init]
    t = np.empty(shape, np.uint32)
    with np.errstate(over="ignore"):
        for _ in range(10):
            for ia, ib, ic, id_ in _QR:
                for p, q, r, s in ((ia, ib, id_, 16), (ic, id_, ib, 12), (ia, ib, id_, 8), (ic, id_, ib, 7)):
                    # p += q; r ^= p; r = rotl(r, s)
                    x[p] += x[q]
                    x[r] ^= x[p]
                    np.right_shift(x[r], 32 - s, out=t)
                    np.left_shift(x[r], s, out=x[r])
                    x[r] |= t
        for v, w in zip(x, init):
            v += w
    return np.stack(x, axis=-1)


def keystream(key, nwords: int, n0, n1, n2) -> np.ndarray:
    """Words 0..nwords-1 of the streams (n0, n1, n2) (broadcast to [rows]): word x is word x % 16 of block x / 16.
    Returns [rows, nwords] u32."""
    nb = (nwords + 15) // 16
    n0, n1, n2 = (np.asarray(v, np.uint64)[..., None] for v in (n0, n1, n2))
    blocks = chacha20_block(key, np.arange(nb, dtype=np.uint64), n0, n1, n2)
    return blocks.reshape(blocks.shape[:-2] + (nb * 16,))[..., :nwords]


def mask_seed_of(rng_key: bytes) -> bytes:
    """S = words 0..7 of block(K, 0, 0, 20, "DES"): a PRF output of the generator key K."""
    return chacha20_block(rng_key, 0, 0, 20, DOMAIN_SEED)[:8].astype("<u4").tobytes()


def f64_to_torus(d) -> np.ndarray:
    """utils.rs:9-12, element-wise (the sign-keeping fmod, truncation toward zero)."""
    t = np.fmod(np.asarray(d, dtype=np.float64), 1.0) * 4294967296.0
    return t.astype(np.int64).astype(np.uint32)


def gauss2(w: np.ndarray, sigma: float):
    """keygen.hpp gauss2: two N(0, sigma) samples from four keystream words (last axis, Box-Muller)."""
    w = w.astype(np.uint64)
    u1 = (((w[..., 0] << np.uint64(21)) ^ (w[..., 1] >> np.uint64(11))).astype(np.float64) + 1.0) * (1.0 / 9007199254740992.0)
    u2 = ((w[..., 2] << np.uint64(21)) ^ (w[..., 3] >> np.uint64(11))).astype(np.float64) * (1.0 / 9007199254740992.0)
    rad = np.sqrt(-2.0 * np.log(u1)) * sigma
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)


def negacyclic_binary(a: np.ndarray, s: np.ndarray) -> np.ndarray:
    """a (*) s mod (X^N + 1) with wrapping u32 coefficients, s binary: the sum of a rotated by every j with s[j] = 1
    (the wrapped part negated).  a: [rows, N]; exact, no float."""
    n = a.shape[-1]
    a = a.astype(np.uint32)
    ext = np.concatenate([(np.uint32(0) - a), a], axis=-1)  # ext[:, n + c - j] = a[c - j], wrapping with a minus sign
    out = np.zeros_like(a)
    for j in np.flatnonzero(s):
        out += ext[:, n - j: 2 * n - j]
    return out


def gadget(p: SecurityParams, d: int) -> int:
    """f64_to_torus(Bg^-(d+1))."""
    return int(f64_to_torus(2.0 ** -(p.bgbit * (d + 1))))


def compress_ksk(p: SecurityParams, key_lv0, key_lv1, rng_key: bytes, seed: bytes, alpha: float,
                 chunk: int = 4096) -> np.ndarray:
    """KSK bodies [N][t][base] (k = 0 slots 0): <a, s0> + gaussian_f64(k s1[i] / 2^((j+1) basebit))."""
    base, t, n = p.base, p.iks_t, p.n
    s0 = np.asarray(key_lv0, np.uint32).reshape(n).astype(bool)
    s1 = np.asarray(key_lv1, np.uint32).reshape(N)
    rows = N * t * base
    out = np.zeros(rows, np.uint32)
    with np.errstate(over="ignore"):
        for lo in range(0, rows, chunk):
            r = np.arange(lo, min(lo + chunk, rows), dtype=np.uint64)
            k = (r % base).astype(np.int64)
            j = ((r // base) % t).astype(np.int64)
            i = (r // (base * t)).astype(np.int64)
            mask = keystream(seed, n, r, 16, DOMAIN_KSK)
            inner = mask[:, s0].sum(axis=1, dtype=np.uint64).astype(np.uint32)
            g0, _ = gauss2(chacha20_block(rng_key, 0, r, 17, DOMAIN_KSK)[:, :4], alpha)
            phase = (k * s1[i]).astype(np.float64) / np.exp2(((j + 1) * p.basebit).astype(np.float64))
            body = inner + f64_to_torus(g0) + f64_to_torus(phase)
            out[lo:lo + len(r)] = np.where(k == 0, np.uint32(0), body)
    return out.reshape(N, t, base)


def bsk_masks(p: SecurityParams, seed: bytes, rows) -> np.ndarray:
    """Mask polynomials a of the BSK rows `rows` (i * 2l + q): [len(rows), N] u32."""
    return keystream(seed, N, np.asarray(rows, np.uint64), 18, DOMAIN_BSK)


def compress_bsk(p: SecurityParams, key_lv0, key_lv1, rng_key: bytes, seed: bytes, alpha: float,
                 chunk: int = 128) -> np.ndarray:
    """BSK bodies [n][2l][N]: q < l: a (*) s1 + e - p g_q s1;  q >= l: a (*) s1 + e + p g_{q-l} X^0."""
    l2 = 2 * p.l
    s0 = np.asarray(key_lv0, np.uint32).reshape(p.n)
    s1 = np.asarray(key_lv1, np.uint32).reshape(N)
    rows = p.n * l2
    g = np.array([gadget(p, d) for d in range(p.l)], np.uint32)
    out = np.empty((rows, N), np.uint32)
    with np.errstate(over="ignore"):
        for lo in range(0, rows, chunk):
            r = np.arange(lo, min(lo + chunk, rows), dtype=np.uint64)
            q = (r % l2).astype(np.int64)
            pg = s0[(r // l2).astype(np.int64)] * g[q % p.l]
            a = bsk_masks(p, seed, r)
            a[:, 0] -= np.where(q < p.l, pg, np.uint32(0))
            b = negacyclic_binary(a, s1)
            # noise in k_gen_bsk's word order: block 2 lane + h gives the pairs of coefficients lane + 64 (4h + m)
            # (first sample) and lane + 64 (4h + m) + 512 (second), m < 4
            w = chacha20_block(rng_key, np.arange(128, dtype=np.uint64), r[:, None], 19, DOMAIN_BSK)
            g0, g1 = gauss2(w.reshape(len(r), 64, 2, 4, 4), alpha)  # [rows, lane, h, m]
            e = np.concatenate([f64_to_torus(g0).reshape(len(r), 64, 8).transpose(0, 2, 1).reshape(len(r), 512),
                                f64_to_torus(g1).reshape(len(r), 64, 8).transpose(0, 2, 1).reshape(len(r), 512)], axis=1)
            b += e
            b[:, 0] += np.where(q >= p.l, pg, np.uint32(0))
            out[lo:lo + len(r)] = b
    return out.reshape(p.n, l2, N)


def compress(p: SecurityParams, key_lv0, key_lv1, rng_key: bytes, alpha_ksk=None, alpha_bsk=None):
    """(mask seed, bsk bodies, ksk bodies, decomposition offset) of the secret key under the generator key."""
    seed = mask_seed_of(rng_key)
    a0 = p.alpha_lv0 if alpha_ksk is None else float(alpha_ksk)
    a1 = p.alpha_lv1 if alpha_bsk is None else float(alpha_bsk)
    if a0 < 0 or a1 < 0:
        raise ValueError("noise parameters are non-negative")
    return (seed, compress_bsk(p, key_lv0, key_lv1, rng_key, seed, a1), compress_ksk(p, key_lv0, key_lv1, rng_key, seed, a0),
            gen_decomposition_offset(p))


def expand_ksk(p: SecurityParams, seed: bytes, ksk_bodies) -> np.ndarray:
    """The full KSK [N][t][base][n+1] of the compressed form (k = 0 rows zero), on the CPU."""
    rows = N * p.iks_t * p.base
    out = np.zeros((rows, p.n + 1), np.uint32)
    r = np.arange(rows, dtype=np.uint64)
    live = (r % p.base) != 0
    for lo in range(0, rows, 8192):
        sl = slice(lo, min(lo + 8192, rows))
        out[sl, :-1] = keystream(seed, p.n, r[sl], 16, DOMAIN_KSK)
    out[:, -1] = np.asarray(ksk_bodies, np.uint32).reshape(rows)
    out[~live] = 0
    return out.reshape(N, p.iks_t, p.base, p.n + 1)


def expand_bsk_torus(p: SecurityParams, seed: bytes, bsk_bodies) -> np.ndarray:
    """The BSK rows as torus polynomials (a, b): [n][2l][2][N] u32 (the spectra are their transforms)."""
    rows = p.n * 2 * p.l
    out = np.empty((rows, 2, N), np.uint32)
    for lo in range(0, rows, 512):
        r = np.arange(lo, min(lo + 512, rows), dtype=np.uint64)
        out[lo:lo + len(r), 0] = bsk_masks(p, seed, r)
    out[:, 1] = np.asarray(bsk_bodies, np.uint32).reshape(rows, N)
    return out.reshape(p.n, 2 * p.l, 2, N)


def tlwe_masks(seed: bytes, first_index: int, count: int, n: int) -> np.ndarray:
    """Masks of seeded TLWE ciphertexts first_index .. first_index + count - 1: [count, n] u32."""
    g = np.uint64(int(first_index)) + np.arange(count, dtype=np.uint64)
    return keystream(seed, n, g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), DOMAIN_TLWE)


def symmetric_rows(mask_key: bytes, rng_key: bytes, rows, key_lv0, plain, alpha: float, domains, full: bool = True,
                   chunk: int = 8192) -> np.ndarray:
    """The CPU form of the symmetric-encryption format: row g of `rows` (u64 indices) is
    (a, <a, s0> + plain + f64_to_torus(g0)) with the mask a under (mask_key, g, domains[0]) and g0 of
    gauss2(words 0..3 of block 0 of (rng_key, g, domains[1]), alpha).  Returns [rows][n+1], or the bodies with full=False."""
    g = np.asarray(rows, np.uint64).reshape(-1)
    s0 = np.asarray(key_lv0, np.uint32).reshape(-1)
    n = len(s0)
    plain = np.broadcast_to(np.asarray(plain, np.uint32).reshape(-1), g.shape)
    out = np.empty((len(g), n + 1 if full else 1), np.uint32)
    lo32, hi32 = g & np.uint64(0xFFFFFFFF), g >> np.uint64(32)
    with np.errstate(over="ignore"):
        for lo in range(0, len(g), chunk):
            sl = slice(lo, lo + chunk)
            masks = keystream(mask_key, n, lo32[sl], hi32[sl], domains[0])
            g0, _ = gauss2(chacha20_block(rng_key, 0, lo32[sl], hi32[sl], domains[1])[:, :4], float(alpha))
            inner = (masks * s0[None, :]).sum(axis=1, dtype=np.uint32)
            if full:
                out[sl, :-1] = masks
            out[sl, -1] = inner + plain[sl] + f64_to_torus(g0)
    return out if full else out[:, 0].copy()


class SeededCiphertexts:
    """Fresh TLWE lv0 ciphertexts as (mask seed, first index, bodies): 4 bytes a ciphertext plus 40."""

    def __init__(self, params: SecurityParams, mask_seed: bytes, first_index: int, bodies):
        self.params = params
        self.mask_seed = bytes(mask_seed)
        if len(self.mask_seed) != 32:
            raise ValueError("mask_seed is 32 bytes")
        self.first_index = int(first_index)
        if not 0 <= self.first_index < 1 << 64:
            raise ValueError("first_index is a u64")
        self.bodies = np.ascontiguousarray(bodies, dtype=np.uint32).reshape(-1)

    def __len__(self) -> int:
        return len(self.bodies)

    @property
    def nbytes(self) -> int:
        return self.bodies.nbytes + 32 + 8

    def expand(self) -> np.ndarray:
        """[count][n+1] u32 on the CPU (Engine.expand_seeded does it on the GPU)."""
        out = np.empty((len(self), self.params.n + 1), np.uint32)
        for lo in range(0, len(self), 8192):
            hi = min(lo + 8192, len(self))
            out[lo:hi, :-1] = tlwe_masks(self.mask_seed, self.first_index + lo, hi - lo, self.params.n)
        out[:, -1] = self.bodies
        return out


def trlwe_masks(seed: bytes, first_group: int, groups: int) -> np.ndarray:
    """Mask polynomials of packed TRLWE ciphertexts first_group .. first_group + groups - 1, natural order: [groups, N]."""
    g = np.uint64(int(first_group)) + np.arange(groups, dtype=np.uint64)
    return keystream(seed, N, g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), DOMAINS_TRLWE[0])


def symmetric_trlwe_rows(mask_key: bytes, rng_key: bytes, groups_idx, key_lv1, plain, count: int, alpha: float,
                         full: bool = True, chunk: int = 64, domains=DOMAINS_TRLWE) -> np.ndarray:
    """The CPU form of the packed-encryption format: group m of `groups_idx` (u64 indices g) is
    (a, a (*) s1 + f64_to_torus(e) + plain[m N ..]) with a under (mask_key, g, "ERL") in natural order and e under
    (rng_key, g, "ERN") in the BSK generators' word order; the slots at or past `count` encrypt 0.  plain: [count] torus
    words.  Returns [groups][2][N], or the bodies [groups][N] with full=False.  domains: the (mask, noise) domain words,
    DOMAINS_TRGSW for the rows of TRGSW selectors."""
    g = np.asarray(groups_idx, np.uint64).reshape(-1)
    s1 = np.asarray(key_lv1, np.uint32).reshape(N)
    count = int(count)
    if not (len(g) - 1) * N < count <= len(g) * N and not (count == 0 and len(g) == 0):
        raise ValueError(f"{count} values do not fill {len(g)} groups of {N}")
    msg = np.zeros(len(g) * N, np.uint32)
    msg[:count] = np.asarray(plain, np.uint32).reshape(-1)[:count]
    msg = msg.reshape(len(g), N)
    out = np.empty((len(g), 2, N), np.uint32)
    lo32, hi32 = g & np.uint64(0xFFFFFFFF), g >> np.uint64(32)
    with np.errstate(over="ignore"):
        for lo in range(0, len(g), chunk):
            sl = slice(lo, lo + chunk)
            rows = len(g[sl])
            a = keystream(mask_key, N, lo32[sl], hi32[sl], domains[0])
            # block 2 lane + h gives the pairs of coefficients lane + 64 (4h + q) (first sample) and + 512 (second), q < 4
            w = chacha20_block(rng_key, np.arange(128, dtype=np.uint64), lo32[sl, None], hi32[sl, None], domains[1])
            g0, g1 = gauss2(w.reshape(rows, 64, 2, 4, 4), float(alpha))  # [rows, lane, h, q]
            e = np.concatenate([f64_to_torus(g0).reshape(rows, 64, 8).transpose(0, 2, 1).reshape(rows, 512),
                                f64_to_torus(g1).reshape(rows, 64, 8).transpose(0, 2, 1).reshape(rows, 512)], axis=1)
            out[sl, 0] = a
            out[sl, 1] = negacyclic_binary(a, s1) + e + msg[sl]
    return out if full else out[:, 1].copy()


class SeededPackedCiphertexts:
    """Fresh packed TRLWE ciphertexts as (mask seed, first group, bodies [groups][N], count): 4 KiB a ciphertext
    instead of 8, plus 48 bytes."""

    def __init__(self, params: SecurityParams, mask_seed: bytes, first_group: int, bodies, count: int):
        self.params = params
        self.mask_seed = bytes(mask_seed)
        if len(self.mask_seed) != 32:
            raise ValueError("mask_seed is 32 bytes")
        self.first_group = int(first_group)
        self.bodies = np.ascontiguousarray(bodies, dtype=np.uint32).reshape(-1, N)
        self.count = int(count)
        if not 0 <= self.first_group or self.first_group + len(self.bodies) > 1 << 64:
            raise ValueError("the group indices run past 2^64")
        if -(-self.count // N) != len(self.bodies):
            raise ValueError(f"{self.count} values do not fill {len(self.bodies)} groups of {N}")

    def __len__(self) -> int:
        return self.count

    @property
    def groups(self) -> int:
        return len(self.bodies)

    @property
    def nbytes(self) -> int:
        return self.bodies.nbytes + 32 + 8 + 8

    def expand(self) -> np.ndarray:
        """[groups][2][N] u32 on the CPU (Engine.expand_seeded_trlwe does it on the GPU)."""
        out = np.empty((self.groups, 2, N), np.uint32)
        for lo in range(0, self.groups, 1024):
            hi = min(lo + 1024, self.groups)
            out[lo:hi, 0] = trlwe_masks(self.mask_seed, self.first_group + lo, hi - lo)
        out[:, 1] = self.bodies
        return out
