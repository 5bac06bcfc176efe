"""Packing key switch on the host: numpy only, no device.

The format and the result are normative in include/tfhe_hip.h ("packing key switch"): up to N = 1024 TLWE lv0 results
become ONE TRLWE lv1 under s1, each coefficient carrying the phase of one input, so results return 350x smaller on
SECURITY_128_BIT.  This module is the client's side -- the packing key (`make_packing_key`: masks from the seeded
section's ChaCha20 keystream, bodies by exact negacyclic products with the binary s1; given a 32-byte generator key it
is the CPU form of `tfhe_hip_gen_packing_key`, which `Engine.gen_packing_key` runs on the GPU) -- and the integer model of the
server's result (`pack_model`), which the GPU (csrc/packing.hpp, `Engine.pack`) equals word for word.  `pack` runs it
on the key view of a cloud key.

The encrypted-table key switch ("encrypted-table key switch and the tree bootstrap" in the header) reuses the key and
the contraction: `table_model` is its integer model (csrc/table.hpp, `Engine.pack_table`), `bootstrap_func2` runs the
tree bootstrap of a function of two encrypted digits on the GPU.

The way back ("unpacking key switch" in the header): `unpack_model` is the integer model of sample_extract_index
followed by identity_key_switching, `unpack` runs it on the GPU (csrc/unpack.hpp, `Engine.unpack`).

From one ring key to another ("TRLWE key switch" in the header): `TrlweSwitchKey` is what travels, `automorphism`,
`gen_trace_keys` and `trace` run slot automorphisms and the partial trace on the GPU (csrc/trlwe_switch.hpp,
`Engine.batch_trlwe_keyswitch`); proxy_reenc.PackedReencryptionKey is the k = 1 case.  The integer model lives with the
tests (tests/trlwe_switch_model.py).

Selecting between packed ciphertexts under encrypted bits ("packed CMUX" in the header): `Trgsw` is a selector,
`encrypt_trgsw_rows` the CPU form of its encryption, `cmux`, `external_product` and `lookup` run on the GPU
(csrc/cmux.hpp, `Engine.batch_trlwe_cmux`).  The integer model is tests/cmux_model.py.
"""
from __future__ import annotations

import numpy as np

from .params import N, SecurityParams
from .seeded import DOMAIN_SEED, chacha20_block, f64_to_torus, gauss2, keystream, negacyclic_binary

DOMAIN_PACK = 0x504B53
PACK_STREAM = 24  # masks, under the mask seed
PACK_NOISE_STREAM = 25  # noise, under the generator key
PACK_SEED_STREAM = 26  # the mask seed from the generator key (domain "DES"; the compressed cloud key's is 20)


def gadget(p: SecurityParams) -> np.ndarray:
    """g_l = 2^(32 - (l+1) basebit), l < t, as u32."""
    return np.array([1 << (32 - (l + 1) * p.basebit) for l in range(p.iks_t)], np.uint32)


def digits(p: SecurityParams, words) -> np.ndarray:
    """The signed digits d_l of the definition, [..., t] int8: the identity key switch's rounding a_bar, then the
    base-B decomposition from the least significant digit up with a carry into the next (the last carry dropped)."""
    bt, base = p.basebit * p.iks_t, p.base
    a = np.asarray(words, np.uint32).astype(np.uint64)
    abar = ((a + np.uint64(1 << (31 - bt))) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bt)
    out = np.empty(a.shape + (p.iks_t,), np.int8)
    carry = np.zeros(a.shape, np.int64)
    for l in range(p.iks_t - 1, -1, -1):
        v = ((abar >> np.uint64(p.basebit * (p.iks_t - 1 - l))) & np.uint64(base - 1)).astype(np.int64) + carry
        neg = v >= base // 2
        out[..., l] = np.where(neg, v - base, v)
        carry = neg.astype(np.int64)
    return out


def key_masks(seed: bytes, rows) -> np.ndarray:
    """Mask polynomials a_r of the packing key rows `rows` (r = i t + l): [len(rows), N] u32."""
    return keystream(seed, N, np.asarray(rows, np.uint64), PACK_STREAM, DOMAIN_PACK)


def key_rows(p: SecurityParams, mask_seed: bytes, bodies) -> np.ndarray:
    """The packing key as [n t][2N] u32 rows: a_r then b_r."""
    rows = p.n * p.iks_t
    out = np.empty((rows, 2 * N), np.uint32)
    for lo in range(0, rows, 1024):
        hi = min(lo + 1024, rows)
        out[lo:hi, :N] = key_masks(mask_seed, np.arange(lo, hi))
    out[:, N:] = np.asarray(bodies, np.uint32).reshape(rows, N)
    return out


def mask_seed_of(rng_key: bytes) -> bytes:
    """S = words 0..7 of block(K, 0, nonce (0, 26, "DES")): the packing key's public mask seed under generator key K."""
    return chacha20_block(rng_key, 0, 0, PACK_SEED_STREAM, DOMAIN_SEED)[:8].astype("<u4").tobytes()


def key_noise(rng_key: bytes, rows, alpha: float) -> np.ndarray:
    """Noise polynomials e_r of the rows `rows` under generator key K, [len(rows), N] u32: blocks 2 lane + h of
    (r, 25, "PKS"), pair m < 4 of a block gives e[lane + 64 (4h + m)] and the same + 512 (the BSK generators' order)."""
    r = np.asarray(rows, np.uint64)
    w = chacha20_block(rng_key, np.arange(128, dtype=np.uint64), r[:, None], PACK_NOISE_STREAM, DOMAIN_PACK)
    g0, g1 = gauss2(w.reshape(len(r), 64, 2, 4, 4), alpha)  # [rows, lane, h, m]
    return np.concatenate([f64_to_torus(g).reshape(len(r), 64, 8).transpose(0, 2, 1).reshape(len(r), N // 2)
                           for g in (g0, g1)], axis=1)


class PackingKey:
    """The packing key of include/tfhe_hip.h: the public 32-byte mask seed and the bodies [n][t][N] u32."""

    FORMAT_VERSION = 1

    def __init__(self, params: SecurityParams, mask_seed, bodies):
        self.params = params
        self.mask_seed = bytes(mask_seed)
        if len(self.mask_seed) != 32:
            raise ValueError("mask_seed is 32 bytes")
        self.bodies = np.ascontiguousarray(bodies, dtype=np.uint32)
        if self.bodies.size != params.n * params.iks_t * N:
            raise ValueError("bodies has the wrong size for these parameters")
        self.bodies = self.bodies.reshape(params.n, params.iks_t, N)

    @property
    def nbytes(self) -> int:
        """Bytes that travel: the bodies and the seed."""
        return self.bodies.nbytes + len(self.mask_seed)

    def save(self, path) -> None:
        """One .npz file: the parameter set's name, the format version and the fields."""
        with open(path, "wb") as f:
            np.savez(f, format_version=np.uint32(self.FORMAT_VERSION), params=np.array(self.params.name),
                     mask_seed=np.frombuffer(self.mask_seed, np.uint8), bodies=self.bodies)

    @classmethod
    def load(cls, path, params: SecurityParams = None) -> "PackingKey":
        """Inverse of save; refuses another format version, and another parameter set than `params` when given."""
        from .params import PARAM_SETS

        with np.load(path, allow_pickle=False) as z:
            version = int(z["format_version"])
            if version != cls.FORMAT_VERSION:
                raise ValueError(f"packing key format {version}, this library reads {cls.FORMAT_VERSION}")
            name = str(z["params"])
            if name not in PARAM_SETS:
                raise ValueError(f"unknown parameter set {name!r}")
            if params is not None and params.name != name:
                raise ValueError(f"the file holds a {name} key, not {params.name}")
            return cls(PARAM_SETS[name], z["mask_seed"].tobytes(), z["bodies"])


def make_packing_key(params: SecurityParams, key_lv0, key_lv1, rng=None, alpha=None, chunk: int = 512) -> PackingKey:
    """The packing key of (key_lv0, key_lv1): b_r = a_r (*) s1 + e_r + s0[i] g_l X^0.  rng: 32 bytes are the generator
    key K of include/tfhe_hip.h ("Generation"): the mask seed and every noise sample are keystream positions under K,
    as `tfhe_hip_gen_packing_key` makes them on the GPU (the same seed and, away from borderline samples, the same
    bodies).  Otherwise None (the OS CSPRNG), an int seed or a numpy Generator (reproducible: tests only) draws the
    mask seed and the noise.  alpha: the noise's standard deviation, alpha_lv1 of the set by default."""
    from .client import OsRng, _rng

    p = params
    if p.basebit > 7:
        raise ValueError("packing needs basebit <= 7")
    alpha = p.alpha_lv1 if alpha is None else float(alpha)
    if not alpha >= 0:
        raise ValueError("alpha is non-negative")
    rng_key = None
    if isinstance(rng, (bytes, bytearray)):
        rng_key = bytes(rng)
        if len(rng_key) != 32:
            raise ValueError("rng_key is 32 bytes")
        seed = mask_seed_of(rng_key)
    else:
        g = _rng(rng)
        if isinstance(g, OsRng):
            import os

            seed = os.urandom(32)
        else:
            seed = g.integers(0, 1 << 32, 8, dtype=np.uint64).astype("<u4").tobytes()
    s0 = np.asarray(key_lv0, np.uint32).reshape(p.n)
    s1 = np.asarray(key_lv1, np.uint32).reshape(N)
    gl = gadget(p)
    rows = p.n * p.iks_t
    bodies = np.empty((rows, N), np.uint32)
    with np.errstate(over="ignore"):
        for lo in range(0, rows, chunk):
            r = np.arange(lo, min(lo + chunk, rows))
            b = negacyclic_binary(key_masks(seed, r), s1)
            if rng_key is not None:
                b += key_noise(rng_key, r, alpha)
            elif alpha > 0:
                b += f64_to_torus(g.normal(0.0, alpha, len(r) * N)).reshape(len(r), N)
            b[:, 0] += s0[r // p.iks_t] * gl[r % p.iks_t]
            bodies[lo:lo + len(r)] = b
    return PackingKey(p, seed, bodies)


def _key_halves(K):
    """The 16-bit halves of the key rows as float64 matrices (the operands of contraction)."""
    return (K & 0xFFFF).astype(np.float64), (K >> 16).astype(np.float64)


def contraction(params: SecurityParams, halves, cts) -> np.ndarray:
    """P[j] = sum_{i,l} d_l(a_j[i]) K[(i,l)] mod 2^32 for [M][n+1] ciphertexts: [M][2N] u32.  A float64 matmul over
    the 16-bit halves of the key words (|sums| < 2^35: exact).  halves: _key_halves(key_rows(...))."""
    p = params
    k_lo, k_hi = halves
    d = digits(p, cts[:, :p.n]).reshape(len(cts), -1).astype(np.float64)  # column i t + l
    lo = (d @ k_lo).astype(np.int64)
    hi = (d @ k_hi).astype(np.int64)
    return ((lo + (hi << 16)) & 0xFFFFFFFF).astype(np.uint32)


def pack_model(params: SecurityParams, mask_seed: bytes, bodies, cts, rows=None) -> np.ndarray:
    """The definition's result for [count][n+1] ciphertexts: [ceil(count / N)][2][N] u32.  The contraction
    P[j] = sum_{i,l} d_l(a_j[i]) K[(i,l)] is a float64 matmul over the 16-bit halves of the key words (|sums| < 2^35:
    exact), the rotate-and-sum a bincount of u32 values (< 2^42: exact).  rows: key_rows(...) when already made."""
    p = params
    cts = np.ascontiguousarray(cts, dtype=np.uint32).reshape(-1, p.n + 1)
    K = key_rows(p, mask_seed, bodies) if rows is None else rows
    halves = _key_halves(K)
    groups = -(-len(cts) // N)
    out = np.zeros((groups, 2, N), np.uint32)
    xs = np.arange(N)
    for g in range(groups):
        c = cts[g * N:(g + 1) * N]
        m = len(c)
        prod = contraction(p, halves, c)  # [m][2N]
        y = xs[None, :] + np.arange(m)[:, None]  # X^j X^x = X^y, y < 2N - 1
        wrap = y >= N
        for h in range(2):
            v = prod[:, h * N:(h + 1) * N]
            v = np.where(wrap, np.uint32(0) - v, v)
            s = np.bincount((y % N).ravel(), weights=v.ravel().astype(np.float64), minlength=N)
            out[g, h] = np.uint32(0) - (s.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
        out[g, 1, :m] += c[:, p.n]
    return out


def window(q, m: int) -> np.ndarray:
    """X^(-off) (1 + X + ... + X^(W-1)) q on the last axis, W = N / m, off = W / 2, negacyclic mod X^N + 1 and wrapping
    mod 2^32: out[y] = sum_{r < W} q~[y + off - r] (the second half of the encrypted-table key switch)."""
    q = np.asarray(q, np.uint32)
    W = N // m
    off = W // 2
    neg = (np.uint32(0) - q).astype(np.uint64)
    ext = np.concatenate([neg, q.astype(np.uint64), neg], axis=-1)  # index i of q~ at position i + N
    cs = np.concatenate([np.zeros(q.shape[:-1] + (1,), np.uint64), np.cumsum(ext, axis=-1, dtype=np.uint64)], axis=-1)
    y = np.arange(N)
    return ((cs[..., y + off + N + 1] - cs[..., y + off - W + N + 1]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def table_model(params: SecurityParams, mask_seed: bytes, bodies, stage1, m: int, rows=None) -> np.ndarray:
    """The definition's result ("encrypted-table key switch", include/tfhe_hip.h) for stage1 [m][count][n+1],
    function-major: [count][2][N] u32.  pack_model's contraction of every input alone (P_x at slot 0), the monomial
    shifts X^(x W) summed per ciphertext, then `window`.  Integer arithmetic throughout: the GPU
    (csrc/table.hpp, `Engine.pack_table`) equals it word for word.  rows: key_rows(...) when already made."""
    p = params
    if m < 2 or m > 512 or m & (m - 1):
        raise ValueError("m is a power of two in [2, 512]")
    s1 = np.ascontiguousarray(stage1, dtype=np.uint32).reshape(m, -1, p.n + 1)
    count = s1.shape[1]
    K = key_rows(p, mask_seed, bodies) if rows is None else rows
    halves = _key_halves(K)
    flat = s1.reshape(-1, p.n + 1)
    P = np.empty((m * count, 2 * N), np.uint32)
    for lo in range(0, len(flat), N):  # bounds the digits held at once
        P[lo:lo + N] = np.uint32(0) - contraction(p, halves, flat[lo:lo + N])
    P = P.reshape(m, count, 2, N)
    P[:, :, 1, 0] += s1[:, :, p.n]
    W = N // m
    Q = np.zeros((count, 2, N), np.uint32)
    for x in range(m):
        j = x * W
        r = np.roll(P[x], j, axis=-1)
        r[..., :j] = np.uint32(0) - r[..., :j]  # X^(x W): what passes N changes sign
        Q += r
    return window(Q, m)


def pack(cts, cloud_key, packing_key: PackingKey, device: int = 0) -> np.ndarray:
    """The server side: [count][n+1] results -> [ceil(count / N)][2][N] packed TRLWEs on the GPU, on the key view of
    `cloud_key` (bootstrap.keyed_engine), where `packing_key` is loaded once."""
    from .bootstrap import keyed_engine

    with keyed_engine(cloud_key, device) as view:
        with view.lock:  # held through the pack: another thread's packing key cannot replace this one in between
            if view._packing_key is not packing_key or not view.packing_key_is_loaded():
                view.load_packing_key(packing_key)
            return view.pack(cts)


def bootstrap_func2(xs, ys, f, m: int, cloud_key, packing_key: PackingKey, n_luts: int = 1, device: int = 0) -> np.ndarray:
    """The tree bootstrap on the GPU: ciphertexts of f(x, y) for [count][n+1] ciphertexts xs, ys of digits of modulus m
    (Generator(m).generate_bivariate_tables(f, n_luts), then Engine.batch_bootstrap_bivariate), on the key view of
    `cloud_key` (bootstrap.keyed_engine), where `packing_key` is loaded once."""
    from .bootstrap import keyed_engine
    from .lut import Generator

    tables = Generator(m).generate_bivariate_tables(f, n_luts)
    with keyed_engine(cloud_key, device) as view:
        with view.lock:  # as in pack: another thread's packing key cannot replace this one in between
            if view._packing_key is not packing_key or not view.packing_key_is_loaded():
                view.load_packing_key(packing_key)
            return view.batch_bootstrap_bivariate(xs, ys, tables, m, n_luts)


# ---- unpacking key switch: slots of TRLWE lv1 ciphertexts back to lv0 ciphertexts ------------------------------------
def _slots(trlwe, count, slots):
    """(trlwe as [groups][2][N], the slot of every output as int64 [count]) after the header's range checks."""
    trlwe = np.ascontiguousarray(trlwe, dtype=np.uint32).reshape(-1, 2, N)
    if slots is None:
        count = len(trlwe) * N if count is None else int(count)
        if count > len(trlwe) * N:
            raise ValueError(f"{len(trlwe)} TRLWEs hold fewer than {count} slots")
        return trlwe, np.arange(count, dtype=np.int64)
    s = np.asarray(slots).astype(np.int64).reshape(-1)
    if count is not None and int(count) != len(s):
        raise ValueError("count differs from len(slots)")
    if len(s) and (s.min() < 0 or s.max() >= len(trlwe) * N):
        raise ValueError("slot out of range")
    return trlwe, s


def extract_rows(trlwe, slots) -> np.ndarray:
    """trlwe::sample_extract_index (trlwe.rs:106-120) of slot s = G N + j for every s in `slots`: [len(slots)][N+1] u32,
    r[i] = a_G[j - i] for i <= j, Torus::MAX - a_G[N + j - i] for i > j (the reference's negation: ~a, one LSB below
    0 - a), r[N] = b_G[j]."""
    trlwe = np.asarray(trlwe, np.uint32).reshape(-1, 2, N)
    s = np.asarray(slots, np.int64).reshape(-1)
    G, j = s // N, s % N
    i = np.arange(N)
    out = np.empty((len(s), N + 1), np.uint32)
    r = np.take_along_axis(trlwe[G, 0], (j[:, None] - i[None, :]) % N, axis=1)
    out[:, :N] = np.where(i[None, :] > j[:, None], ~r, r)
    out[:, N] = trlwe[G, 1, j]
    return out


def key_switch_model(params: SecurityParams, ksk, rows) -> np.ndarray:
    """trgsw::identity_key_switching (trgsw.rs:332-360) of [M][N+1] lv1 rows under ksk [N][t][base][n+1]: [M][n+1] u32,
    out = (0, .., 0, r[N]) - sum over (i, l) with digit k != 0 of ksk[i][l][k], k = digit l of r[i] + 2^(31 - basebit t).
    Base 4 runs as float64 matmuls of the one-hot digits with the 16-bit halves of the key words (sums < 2^36: exact);
    wider bases, whose one-hot rows are mostly zeros, gather the key rows instead."""
    p = params
    t, bb, base = p.iks_t, p.basebit, p.base
    ksk = np.asarray(ksk, np.uint32).reshape(N, t, base, p.n + 1)
    rows = np.asarray(rows, np.uint32).reshape(-1, N + 1)
    M = len(rows)
    abar = rows[:, :N] + np.uint32(1 << (31 - bb * t))
    k = np.stack([(abar >> np.uint32(32 - (l + 1) * bb)) & np.uint32(base - 1) for l in range(t)], axis=2)  # [M][N][t]
    acc = np.zeros((M, p.n + 1), np.uint32)
    if base <= 4:
        step = 64  # coefficients per product
        for lo in range(0, N, step):
            kk = k[:, lo:lo + step]
            hot = (kk[..., None] == np.arange(1, base, dtype=np.uint32)).astype(np.float64).reshape(M, -1)
            key = ksk[lo:lo + step, :, 1:].reshape(-1, p.n + 1)
            s = (hot @ (key & 0xFFFF).astype(np.float64)).astype(np.int64)
            s += (hot @ (key >> 16).astype(np.float64)).astype(np.int64) << 16
            acc += (s & 0xFFFFFFFF).astype(np.uint32)
    else:
        for i in range(N):
            for l in range(t):
                kk = k[:, i, l]
                acc += ksk[i, l][kk] * (kk != 0).astype(np.uint32)[:, None]
    out = np.uint32(0) - acc
    out[:, p.n] += rows[:, N]
    return out


def unpack_model(params: SecurityParams, ksk, trlwe, count=None, slots=None) -> np.ndarray:
    """The definition's result ("unpacking key switch", include/tfhe_hip.h): output m is the identity key switch, under
    the cloud key's `ksk` [N][t][base][n+1], of the lv1 row extracted at slot slots[m] (m itself with slots None) of
    trlwe [groups][2][N].  [count][n+1] u32; integer arithmetic throughout, so the GPU equals it word for word."""
    trlwe, s = _slots(trlwe, count, slots)
    out = np.empty((len(s), params.n + 1), np.uint32)
    for lo in range(0, len(s), 2048):  # bounds the rows and digits held at once
        out[lo:lo + 2048] = key_switch_model(params, ksk, extract_rows(trlwe, s[lo:lo + 2048]))
    return out


def unpack(packed, cloud_key, count=None, slots=None, device: int = 0) -> np.ndarray:
    """The server side: slots of [groups][2][N] TRLWE lv1 ciphertexts -> [count][n+1] lv0 ciphertexts on the GPU, on
    the key view of `cloud_key` (bootstrap.keyed_engine)."""
    from .bootstrap import keyed_engine

    with keyed_engine(cloud_key, device) as view:
        return view.unpack(packed, count, slots)


# ---- TRLWE key switch: packed re-encryption and slot automorphisms ------------------------------------------------------
TRLWE_SWITCH_CHUNK = 2048  # ciphertexts a pass of the GPU's digit scratch: kTsChunk of csrc/trlwe_switch.hpp
TRLWE_SWITCH_MAX_KEYS = 16  # switching keys a handle holds


class TrlweSwitchKey:
    """A switching key of include/tfhe_hip.h ("TRLWE key switch"): the automorphism k, the decomposition (basebit, t),
    the public 32-byte mask seed and the bodies [t][N] u32 (24 KiB at t = 6).  k = 1 is a re-encryption key."""

    def __init__(self, k: int, basebit: int, t: int, mask_seed, bodies):
        self.k, self.basebit, self.t = int(k), int(basebit), int(t)
        if not (1 <= self.k < 2 * N and self.k & 1):
            raise ValueError("k must be odd, 1 <= k < 2N")
        if not (1 <= self.basebit <= 7 and 1 <= self.t <= 64 and self.basebit * self.t <= 32):
            raise ValueError("1 <= basebit <= 7, 1 <= t <= 64, basebit * t <= 32")
        self.mask_seed = bytes(mask_seed)
        if len(self.mask_seed) != 32:
            raise ValueError("mask_seed is 32 bytes")
        self.bodies = np.ascontiguousarray(bodies, dtype=np.uint32)
        if self.bodies.size != self.t * N:
            raise ValueError("bodies must be [t][N]")
        self.bodies = self.bodies.reshape(self.t, N)

    @property
    def nbytes(self) -> int:
        """Bytes that travel: the bodies and the seed."""
        return self.bodies.nbytes + len(self.mask_seed)


def trace_ks(steps: int):
    """k_s = N / 2^(s-1) + 1 for s = 1 .. steps: psi_{k_s} fixes X^(2^s) and negates X^(2^(s-1))."""
    if not 1 <= int(steps) <= 10:
        raise ValueError("1 <= steps <= 10")
    return [N // (1 << (s - 1)) + 1 for s in range(1, int(steps) + 1)]


def automorphism(packed, k: int, engine):
    """ct(X) -> ct(X^k) on [count][2][N] packed ciphertexts (numpy, or a CUDA tensor on the engine's GPU): slot j moves
    to slot j k mod N, negated when j k mod 2N >= N.  Needs the Galois key for k on `engine`
    (engine.gen_trlwe_switch_key(s1, s1, k, ...) or gen_trace_keys)."""
    return engine.batch_trlwe_keyswitch(int(k), packed)


def gen_trace_keys(engine, sk, steps: int, basebit: int = 4, t: int = 6, rng_key: bytes = None, alpha=None):
    """The Galois keys of `trace(.., steps, ..)` under the secret key `sk` (client.SecretKey): k_s = N / 2^(s-1) + 1,
    s = 1 .. steps, generated on `engine` and left loaded there.  One generator key serves all of them (one key per k).
    Returns the list of TrlweSwitchKey."""
    return [engine.gen_trlwe_switch_key(sk.key_lv1, sk.key_lv1, k, basebit, t, rng_key=rng_key, alpha=alpha)
            for k in trace_ks(steps)]


def trace(packed, steps: int, engine):
    """The partial trace ct <- ct + switch_{k_s}(ct), s = 1 .. steps, on [count][2][N] packed ciphertexts (numpy, or a
    CUDA tensor on the engine's GPU), with the keys of gen_trace_keys loaded on `engine`.  Afterwards the coefficients at
    multiples of 2^steps hold 2^steps times their phase and every other coefficient holds zero plus noise; at steps = 10
    only coefficient 0 survives, times 1,024.  The caller therefore encodes at message / 2^steps: a value that is to
    decode at torus position mu after the trace is encrypted (or scaled by the product's weights) at mu / 2^steps, and
    the noise already in the ciphertext grows by the same 2^steps."""
    ct = packed if type(packed).__module__.startswith("torch") else np.ascontiguousarray(packed, np.uint32).reshape(-1, 2, N)
    for k in trace_ks(steps):
        ct = ct + engine.batch_trlwe_keyswitch(k, ct)  # wrapping: uint32 arrays, int32 tensors
    return ct


# ---- packed CMUX: caller-held TRGSW selectors -----------------------------------------------------------------------------
TRGSW_SEED_STREAM = 30  # the selectors' mask seed from the generator key (domain "DES")
CMUX_CHUNK = 2048  # ciphertexts a pass of the GPU's digit scratch: kCmuxChunk of csrc/cmux.hpp


def check_gadget(basebit: int, t: int) -> None:
    """The box of include/tfhe_hip.h ("packed CMUX"): the TRLWE key switch's with 2t columns."""
    if not (1 <= int(basebit) <= 7 and 1 <= int(t) <= 32 and int(basebit) * int(t) <= 32):
        raise ValueError("1 <= basebit <= 7, 1 <= t <= 32, basebit * t <= 32")


class Trgsw:
    """A TRGSW selector of include/tfhe_hip.h ("packed CMUX"): the gadget (basebit, t) and the rows [2t][2][N] u32 (a
    numpy array, or a CUDA tensor of 32-bit words) -- 48 KiB at t = 3."""

    def __init__(self, basebit: int, t: int, rows):
        check_gadget(basebit, t)
        self.basebit, self.t = int(basebit), int(t)
        if type(rows).__module__.startswith("torch"):
            if rows.numel() != 4 * self.t * N:
                raise ValueError("rows must be [2t][2][N]")
            self.rows = rows.reshape(2 * self.t, 2, N)
        else:
            rows = np.ascontiguousarray(rows, dtype=np.uint32)
            if rows.size != 4 * self.t * N:
                raise ValueError("rows must be [2t][2][N]")
            self.rows = rows.reshape(2 * self.t, 2, N)

    def on(self, engine):
        """The rows as a CUDA tensor on the engine's GPU (uploaded once, then kept)."""
        if not type(self.rows).__module__.startswith("torch"):
            import torch

            self.rows = torch.from_numpy(self.rows.view(np.int32)).to(f"cuda:{engine.device}")
        return self.rows

    def host(self) -> np.ndarray:
        """The rows as a u32 array."""
        if type(self.rows).__module__.startswith("torch"):
            return self.rows.cpu().numpy().view(np.uint32)
        return self.rows


def trgsw_mask_seed(rng_key: bytes) -> bytes:
    """S = words 0..7 of block(K, counter 0, nonce (0, 30, "DES"))"""
    return chacha20_block(rng_key, 0, 0, TRGSW_SEED_STREAM, DOMAIN_SEED)[:8].astype("<u4").tobytes()


def encrypt_trgsw_rows(key_lv1, mu, basebit: int, t: int, alpha: float, rng_key: bytes, first_index: int = 0) -> np.ndarray:
    """The CPU form of `tfhe_hip_batch_encrypt_trgsw`: mu [count][N] small integers -> [count][2t][2][N] u32.  Row
    `row` of selector m is the packed-encryption row of zero at index first_index + m 2t + row under the domains "EGL"
    / "EGN", and g_i mu(X) is added afterwards: to the a half for row = i < t, to the b half for row = t + i."""
    from .seeded import DOMAINS_TRGSW, symmetric_trlwe_rows

    check_gadget(basebit, t)
    mu = np.ascontiguousarray(mu, dtype=np.int64).reshape(-1, N)
    rows = len(mu) * 2 * t
    if int(first_index) < 0 or int(first_index) + rows > 1 << 64:
        raise ValueError("the row indices run past 2^64")
    idx = np.uint64(int(first_index)) + np.arange(rows, dtype=np.uint64)
    out = symmetric_trlwe_rows(trgsw_mask_seed(rng_key), bytes(rng_key), idx, key_lv1, np.zeros(rows * N, np.uint32),
                               rows * N, alpha, domains=DOMAINS_TRGSW).reshape(len(mu), 2, t, 2, N)
    g = np.array([1 << (32 - (i + 1) * basebit) for i in range(t)], np.int64)
    add = ((g[None, :, None] * mu[:, None, :]) & 0xFFFFFFFF).astype(np.uint32)  # [count][t][N]
    with np.errstate(over="ignore"):
        out[:, 0, :, 0] += add
        out[:, 1, :, 1] += add
    return out.reshape(len(mu), 2 * t, 2, N)


def _packed_arg(x, engine):
    """[count][2][N] for the engine: a CUDA tensor as it is, anything else as a u32 array"""
    if x is None or type(x).__module__.startswith("torch"):
        return x
    return np.ascontiguousarray(x, np.uint32).reshape(-1, 2, N)


def cmux(sel: Trgsw, d0, d1, engine, reference_digits: bool = False):
    """d0 + sel (.) (d1 - d0) on [count][2][N] packed ciphertexts (numpy, or CUDA tensors on the engine's GPU): d1 where
    the selector encrypts 1, d0 where it encrypts 0, in every slot, under ONE selector (`Engine.batch_trlwe_cmux`)."""
    d1 = _packed_arg(d1, engine)
    rows = sel.on(engine) if type(d1).__module__.startswith("torch") else sel.host()
    return engine.batch_trlwe_cmux(rows, sel.basebit, sel.t, _packed_arg(d0, engine), d1, reference_digits=reference_digits)


def external_product(sel: Trgsw, d, engine, reference_digits: bool = False):
    """sel (.) d: the ciphertexts of mu(X) times the phases of d, for a selector of message polynomial mu."""
    return cmux(sel, None, d, engine, reference_digits)


def lookup(selectors, table, engine):
    """Entry k of a table of 2^d packed ciphertexts [2^d][2][N] under the encrypted index k = sum_i bit_i 2^i, bit_i the
    message of selectors[i] (least significant first): d CMUX calls, level i running 2^(d-1-i) pairs under selector
    i, between two buffers on the engine's GPU.  The table is laid out in bit-reversed order once, so that the pairs
    of every level are the two contiguous halves of what the level before left.  Returns [2][N] (numpy for a numpy
    table, else a tensor)."""
    import torch

    d = len(selectors)
    tensors = type(table).__module__.startswith("torch")
    tab = table if tensors else torch.from_numpy(np.ascontiguousarray(table, np.uint32).reshape(-1, 2, N).view(np.int32))
    if tab.dim() != 3 or tab.shape[0] != 1 << d or tuple(tab.shape[1:]) != (2, N):
        raise ValueError(f"{d} selectors look up a table of [{1 << d}][2][{N}]")
    tab = tab.to(f"cuda:{engine.device}")
    if d == 0:
        return tab[0] if tensors else tab[0].cpu().numpy().view(np.uint32)
    rev = [int(format(p, f"0{d}b")[::-1], 2) for p in range(1 << d)]
    cur = tab[torch.tensor(rev, device=tab.device)]  # position p holds entry rev(p)
    other = torch.empty_like(cur[: 1 << (d - 1)])
    for i, sel in enumerate(selectors):
        n = 1 << (d - 1 - i)
        engine.batch_trlwe_cmux(sel.on(engine), sel.basebit, sel.t, cur[:n], cur[n:2 * n], out=other[:n])
        cur, other = other, cur
    return cur[0] if tensors else cur[0].cpu().numpy().view(np.uint32)
