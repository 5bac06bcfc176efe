"""A CPU model of the packing-key generator (csrc/packing_keygen.hpp), sample for sample.  No test functions.

The generated packing key is a function of (secret key, generator key K, alpha): include/tfhe_hip.h, "packing key
switch", Generation.  rs_tfhe_amd.seeded supplies the keystream, gauss2, f64_to_torus and the exact negacyclic product,
packing.key_masks the masks; keygen_model (KM) the long-double sampler, the borderline rule, compare_words and
noise_report.  What is restated here is the little that is the packing key's own:
  * the mask seed, block(K, 0, (0, 26, "DES"))[:8];
  * the noise words under (r, 25, "PKS") in the BSK generators' word order (KM.bsk_noise_words has the BSK domain
    baked in);
  * the body b_r = a_r (*) s1 + e_r + s0[i] g_l X^0;
  * recover_noise, which reads e_r off a key with the secret key alone (no model, no generator key).
The `alter` switches build the wrong generators test_packing_keygen_host.py proves the checkers on."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import keygen_model as KM
from rs_tfhe_amd import packing as PK
from rs_tfhe_amd import seeded as S
from rs_tfhe_amd.params import N, SecurityParams

DOMAIN = 0x504B53  # "PKS"
MASK_STREAM, NOISE_STREAM, SEED_STREAM = 24, 25, 26
WIDE_SHAPE = (20, 1, 22, 7, 3)  # the widest digit packing takes: basebit = 7
SHAPES = KM.SHAPES + (WIDE_SHAPE,)


def mask_seed(K: bytes) -> bytes:
    """S = words 0..7 of block(K, counter 0, nonce (0, 26, "DES"))"""
    return S.chacha20_block(K, 0, 0, SEED_STREAM, S.DOMAIN_SEED)[:8].astype("<u4").tobytes()


def noise_words(K: bytes, rows, stream: int = NOISE_STREAM, no_row: bool = False) -> np.ndarray:
    """The four words of every Gaussian pair: [rows, lane, h, m, 4], blocks 2 lane + h of (row, stream, "PKS").
    no_row: the altered generator whose nonce forgets the row."""
    rows = np.asarray(rows, np.uint64)
    nonce = np.zeros_like(rows) if no_row else rows
    w = S.chacha20_block(K, np.arange(128, dtype=np.uint64), nonce[:, None], stream, DOMAIN)
    return w.reshape(len(rows), 64, 2, 4, 4)


def _coeff_order(x):
    """[rows, lane, m] -> [rows, 64 m + lane]"""
    return x.transpose(0, 2, 1).reshape(x.shape[0], -1)


def _pairs_to_poly(a0, a1):
    """pair (lane, h, m) -> coefficients lane + 64 (4h + m) (first sample) and + 512 (second)"""
    r = a0.shape[0]
    return np.concatenate([_coeff_order(a0.reshape(r, 64, 8)), _coeff_order(a1.reshape(r, 64, 8))], axis=1)


def noise(K: bytes, rows, alpha: float, chunk: int = 256, stream: int = NOISE_STREAM, no_row: bool = False,
          same_pair: bool = False) -> KM.Noise:
    """Noise polynomials [rows, N] as KM.Noise (f64 words, long-double words, the borderline marks).
    same_pair: the altered generator that writes g0 where g1 belongs."""
    rows = np.asarray(rows, np.uint64)
    out = KM.Noise(np.zeros((len(rows), N), np.uint32), np.zeros((len(rows), N), np.uint32), np.zeros((len(rows), N), bool))
    for lo in range(0, len(rows), chunk):
        w = noise_words(K, rows[lo:lo + chunk], stream, no_row)
        g0, g1 = S.gauss2(w, alpha)
        x0, x1, l0, l1 = KM.gauss2_ld(w, alpha)
        if same_pair:
            g1, x1, l1 = g0, x0, l0
        sl = slice(lo, lo + w.shape[0])
        out.words[sl] = _pairs_to_poly(S.f64_to_torus(g0), S.f64_to_torus(g1))
        out.ld_words[sl] = _pairs_to_poly(KM.ld_to_torus(x0), KM.ld_to_torus(x1))
        out.border[sl] = _pairs_to_poly(KM.borderline(x0, l0, alpha), KM.borderline(x1, l1, alpha))
    return out


def gadgets(p: SecurityParams, s0, rows, next_digit: bool = False) -> np.ndarray:
    """s0[i] g_l of rows i t + l, g_l = 2^(32 - (l+1) basebit).  next_digit: the altered generator that takes g_{l+1}."""
    r = np.asarray(rows, np.int64)
    l = r % p.iks_t + (1 if next_digit else 0)
    g = (np.int64(1) << (32 - (l + 1) * p.basebit).clip(0)).astype(np.uint32)
    return np.asarray(s0, np.uint32).reshape(p.n)[r // p.iks_t] * g


@dataclass
class Model:
    mask_seed: bytes
    bodies: np.ndarray  # [n][t][N] u32
    border: np.ndarray  # [n][t][N] bool
    e: KM.Noise  # [n t, N]


def model(p: SecurityParams, s0, s1, K: bytes, alpha=None, chunk: int = 256, gadget_at: int = 0, next_digit: bool = False,
          **alter) -> Model:
    """tfhe_hip_gen_packing_key(K) on the CPU.  gadget_at / next_digit / alter (noise's stream, no_row, same_pair): the
    altered generators."""
    alpha = p.alpha_lv1 if alpha is None else float(alpha)
    seed = mask_seed(K)
    rows = np.arange(p.n * p.iks_t)
    s1 = np.asarray(s1, np.uint32).reshape(N)
    e = noise(K, rows, alpha, **alter)
    bodies = np.empty((len(rows), N), np.uint32)
    with np.errstate(over="ignore"):
        for lo in range(0, len(rows), chunk):
            r = rows[lo:lo + chunk]
            b = S.negacyclic_binary(PK.key_masks(seed, r), s1) + e.words[lo:lo + chunk]
            b[:, gadget_at] += gadgets(p, s0, r, next_digit)
            bodies[lo:lo + chunk] = b
    shape = (p.n, p.iks_t, N)
    return Model(seed, bodies.reshape(shape), e.border.reshape(shape), e)


def recover_noise(p: SecurityParams, s0, s1, mask_seed_: bytes, bodies, chunk: int = 512):
    """(e, a) of a packing key: e = b - a (*) s1 - s0[i] g_l X^0 as [rows, N] int32, a the masks under the key's seed.
    Uses the secret key alone."""
    rows = np.arange(p.n * p.iks_t)
    b = np.asarray(bodies, np.uint32).reshape(len(rows), N)
    s1 = np.asarray(s1, np.uint32).reshape(N)
    e = np.empty((len(rows), N), np.uint32)
    a = np.empty((len(rows), N), np.uint32)
    with np.errstate(over="ignore"):
        for lo in range(0, len(rows), chunk):
            r = rows[lo:lo + chunk]
            a[lo:lo + chunk] = PK.key_masks(mask_seed_, r)
            e[lo:lo + chunk] = b[lo:lo + chunk] - S.negacyclic_binary(a[lo:lo + chunk], s1)
            e[lo:lo + chunk, 0] -= gadgets(p, s0, r)
    return e.view(np.int32), a


def checksum(words) -> int:
    """sum of (2 x + 1) w[x] mod 2^64 over the flat words (tests/cpp/test_packing_keygen.cpp prints the same)"""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int((w * (np.uint64(2) * np.arange(len(w), dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))
