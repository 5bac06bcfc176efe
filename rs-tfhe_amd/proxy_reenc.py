"""LWE proxy re-encryption (the reference's feature `proxy-reenc`, src/proxy_reenc.rs).

    PublicKeyLv0::new / new_with_params / encrypt_f64 / encrypt_bool       src/proxy_reenc.rs:95-222
    ProxyReencryptionKey::new_asymmetric[_with_params]                     src/proxy_reenc.rs:271-330
    ProxyReencryptionKey::new_symmetric[_with_params]                      src/proxy_reenc.rs:362-425
    reencrypt_tlwe_lv0                                                     src/proxy_reenc.rs:468-510

Key generation is client-side integer work (numpy, batched; it needs the delegator's secret key).  The re-encryption
itself -- the proxy's job, one digit-lookup walk over n * t rows of n + 1 words per ciphertext, i.e. the identity key
switch with a source of n coefficients -- runs on the GPU through the key-switch kernels
(`tfhe_hip_load_reenc_key` / `tfhe_hip_batch_reencrypt`, include/tfhe_hip.h); there is no CPU path here.

Randomness follows client.py: `seed=None` draws from the operating system; an integer seed is reproducible and for
tests only.

Public-key encryption and the asymmetric key also exist in the keyed format of include/tfhe_hip.h ("public-key
encryption and the asymmetric re-encryption key"): every selector bit and noise sample is a position of a ChaCha20
keystream under a secret 32-byte generator key.  `rng_key=` alone is the CPU form of that format (`encrypt_rows`
below); `device=` runs it on the GPU (`tfhe_hip_batch_pk_encrypt`, `tfhe_hip_gen_reenc_key_asymmetric`), where
rng_key=None draws the key from getrandom(2).  A (rng_key, row index) pair must never encrypt two messages.

What is made with the SECRET key -- `PublicKeyLv0.new` and `ProxyReencryptionKey.new_symmetric` -- takes the same two
arguments, in the format of the header's "symmetric encryption" section (`seeded.symmetric_rows` is its CPU form;
`tfhe_hip_gen_public_key` and `tfhe_hip_gen_reenc_key_symmetric` run it on the GPU and leave the key on its view).  There
a caller-held rng_key is as secret as the secret key, and one rng_key makes one key.
"""
from __future__ import annotations

import numpy as np

from . import seeded
from .client import SecretKey, _rng, f64_to_torus
from .params import SecurityParams

DOMAIN_PKE_SEL, DOMAIN_PKE_NOISE = 0x504B45, 0x504B4E  # "PKE", "PKN": public-key encryptions
DOMAIN_RKE_SEL, DOMAIN_RKE_NOISE = 0x524B45, 0x524B4E  # "RKE", "RKN": rows of the asymmetric re-encryption key
MAX_PUBLIC_KEY_SIZE = 8192


def _key_lv0(key) -> np.ndarray:
    return np.ascontiguousarray(key.key_lv0 if isinstance(key, SecretKey) else key, dtype=np.uint32)


def _rng_key(rng_key) -> bytes:
    if not isinstance(rng_key, (bytes, bytearray)) or len(rng_key) != 32:
        raise ValueError("rng_key is 32 bytes")
    return bytes(rng_key)


def selectors(rng_key: bytes, rows, size: int, domain: int) -> np.ndarray:
    """The coefficients c in {-1, 0, +1} of rows `rows` (u64 indices) as [rows][size] f64: entry e reads bits
    2 (e % 16) (take) and 2 (e % 16) + 1 (sign, 1 = subtract) of word e / 16 of the stream (g lo, g hi, domain)."""
    g = np.asarray(rows, np.uint64)
    w = seeded.keystream(rng_key, (size + 15) // 16, g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), domain)
    e = np.arange(size)
    fields = (w[:, e // 16] >> (2 * (e % 16)).astype(np.uint32)) & np.uint32(3)
    return np.where(fields & 1, np.where(fields & 2, -1.0, 1.0), 0.0)


def encrypt_rows(encryptions: np.ndarray, rng_key: bytes, rows, plain, alpha: float, domains, chunk: int = 2048) -> np.ndarray:
    """The CPU form of the keyed format: row g of `rows` is sum_e c_e E[e] (the exact f64 product: |sum| <= size 2^32
    < 2^53) with plain (torus words) + f64_to_torus(g0 of gauss2(block 0 of the noise stream)) on the body."""
    rng_key = _rng_key(rng_key)
    rows = np.asarray(rows, np.uint64).reshape(-1)
    plain = np.asarray(plain, np.uint32).reshape(-1)
    size, w = encryptions.shape
    enc = encryptions.astype(np.float64)
    out = np.empty((len(rows), w), np.uint32)
    for lo in range(0, len(rows), chunk):
        acc = selectors(rng_key, rows[lo:lo + chunk], size, domains[0]) @ enc
        out[lo:lo + chunk] = np.mod(acc, 4294967296.0).astype(np.uint64).astype(np.uint32)
    nw = seeded.chacha20_block(rng_key, 0, rows & np.uint64(0xFFFFFFFF), rows >> np.uint64(32), domains[1])[:, :4]
    g0, _ = seeded.gauss2(nw, float(alpha))
    out[:, -1] += plain + f64_to_torus(g0)
    return out


class PublicKeyLv0:
    """proxy_reenc.rs:95-99: encryptions of zero under the secret key, [size][n+1]."""

    def __init__(self, params: SecurityParams, encryptions):
        self.params = params
        self.encryptions = np.ascontiguousarray(encryptions, dtype=np.uint32).reshape(-1, params.n + 1)
        self._view = None

    @classmethod
    def new(cls, secret_key: SecretKey, seed=None, rng_key=None, device=None) -> "PublicKeyLv0":
        """proxy_reenc.rs:125-131: 2n encryptions of zero at the level-0 noise."""
        p = secret_key.params
        return cls.new_with_params(secret_key, 2 * p.n, p.alpha_lv0, seed, rng_key, device)

    @classmethod
    def new_with_params(cls, secret_key: SecretKey, size: int, alpha: float, seed=None, rng_key=None,
                        device=None) -> "PublicKeyLv0":
        """proxy_reenc.rs:144-153.
        rng_key / device: the keyed format of include/tfhe_hip.h ("symmetric encryption", row e of the "PKM" / "PKZ"
        streams) -- on the CPU with rng_key alone; with `device` the key is generated in a key view of that GPU
        (`tfhe_hip_gen_public_key`; rng_key=None: a key from getrandom(2)) which the returned object keeps, so
        `encrypt_f64(device=)` uploads nothing.  One rng_key makes one public key."""
        p = secret_key.params
        if rng_key is None and device is None:
            return cls(p, secret_key.encrypt_f64(np.zeros(int(size)), seed, alpha))
        if seed is not None:
            raise ValueError("seed selects numpy's generator; rng_key / device select the keyed format")
        if not 1 <= int(size) <= MAX_PUBLIC_KEY_SIZE:
            raise ValueError(f"public key size must be in [1, {MAX_PUBLIC_KEY_SIZE}]")
        if device is None:
            rows = np.arange(int(size), dtype=np.uint64)
            k = _rng_key(rng_key)
            return cls(p, seeded.symmetric_rows(k, k, rows, secret_key.key_lv0, 0, alpha, seeded.DOMAINS_SYM_PK))
        from .bootstrap import engine_for

        v = engine_for(p, device).new_key_view()
        try:
            pk = cls(p, v.gen_public_key(secret_key.key_lv0, int(size), alpha, rng_key))
        except Exception:
            v.close()
            raise
        pk._view = (device, v)
        return pk

    def encrypt_f64(self, plaintext, alpha: float, seed=None, rng_key=None, first_index: int = 0, device=None) -> np.ndarray:
        """proxy_reenc.rs:168-200, batched over `plaintext`: every encryption of zero joins with probability 1/2, added
        or subtracted with probability 1/2 each; then f64_to_torus(plaintext) and fresh noise N(0, alpha) on b.
        rng_key / first_index / device: the keyed format of include/tfhe_hip.h, ciphertext m at row first_index + m --
        on the CPU with rng_key alone, on GPU `device` otherwise (rng_key=None there: a key from getrandom(2))."""
        pt = np.atleast_1d(np.asarray(plaintext, dtype=np.float64))
        if rng_key is not None or device is not None:
            if seed is not None:
                raise ValueError("seed selects numpy's generator; rng_key / device select the keyed format")
            if not (0 <= int(first_index) and int(first_index) + len(pt) <= 1 << 64):
                raise ValueError("first_index is a u64")
            if device is not None:
                return self.view(device).batch_pk_encrypt(f64_to_torus(pt), alpha, rng_key, first_index)
            rows = np.uint64(int(first_index)) + np.arange(len(pt), dtype=np.uint64)
            return encrypt_rows(self.encryptions, rng_key, rows, f64_to_torus(pt), alpha, (DOMAIN_PKE_SEL, DOMAIN_PKE_NOISE))
        g = _rng(seed)
        size, w = self.encryptions.shape
        enc = self.encryptions.astype(np.float64)  # |sum| <= size * 2^32 < 2^53: the f64 product below is exact
        out = np.empty((len(pt), w), np.uint32)
        for lo in range(0, len(pt), 2048):
            m = min(2048, len(pt) - lo)
            take = g.integers(0, 2, (m, size), dtype=np.uint32).astype(np.float64)
            sign = 1.0 - 2.0 * g.integers(0, 2, (m, size), dtype=np.uint32).astype(np.float64)
            acc = (take * sign) @ enc
            out[lo:lo + m] = np.mod(acc, 4294967296.0).astype(np.uint64).astype(np.uint32)
        noise = f64_to_torus(g.normal(0.0, alpha, len(pt))) if alpha > 0 else np.zeros(len(pt), np.uint32)
        out[:, -1] += f64_to_torus(pt) + noise
        return out

    def encrypt_bool(self, bits, alpha: float, seed=None, rng_key=None, first_index: int = 0, device=None) -> np.ndarray:
        """proxy_reenc.rs:212-215."""
        bits = np.atleast_1d(np.asarray(bits)).astype(bool)
        return self.encrypt_f64(np.where(bits, 0.125, -0.125), alpha, seed, rng_key, first_index, device)

    def view(self, device: int = 0):
        """The key view of the shared context that holds this public key's byte planes (loaded on first use)."""
        if self._view is None or self._view[0] != device:
            from .bootstrap import engine_for

            self.close()
            v = engine_for(self.params, device).new_key_view()
            v.load_public_key(self.encryptions)
            self._view = (device, v)
        return self._view[1]

    def close(self) -> None:
        """Free the device copy (also on garbage collection)."""
        if getattr(self, "_view", None) is not None:
            self._view[1].close()
            self._view = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _engine_params(p: SecurityParams, basebit: int, t: int) -> SecurityParams:
    """The context's parameter set: the ciphertexts' set with the key's (basebit, t) (custom `_with_params` keys)."""
    if (p.basebit, p.iks_t) == (basebit, t):
        return p
    import dataclasses

    return dataclasses.replace(p, name=f"{p.name}+reenc(basebit={basebit},t={t})", basebit=basebit, iks_t=t)


class ProxyReencryptionKey:
    """proxy_reenc.rs:224-233: key_encryptions [n][t][base][n+1] (index base*t*i + base*j + k; the k = 0 entries stay
    zero, :311-313), base, t.  `reencrypt` keeps the key resident on the GPU in a key view of the shared context."""

    def __init__(self, params: SecurityParams, key_encryptions, basebit: int, t: int):
        if params.n > 1024:  # (the key-switch kernels' row count is N = 1024: said here, not at the first reencrypt)
            raise ValueError(f"proxy re-encryption on the GPU needs n <= 1024 ({params.name}: n = {params.n})")
        self.params = params
        self.basebit, self.t, self.base = int(basebit), int(t), 1 << int(basebit)
        self._view = None
        self.key_encryptions = np.ascontiguousarray(key_encryptions, dtype=np.uint32).reshape(
            params.n * self.t * self.base, params.n + 1)

    # the plaintexts both constructors encrypt: k * key_from[i] / 2^((j+1) basebit), k = 1 .. base-1 (:316, :414)
    @staticmethod
    def _plaintexts(key_from: np.ndarray, basebit: int, t: int) -> np.ndarray:
        base = 1 << basebit
        k = np.arange(base, dtype=np.uint32)[None, None, :]
        j = np.arange(t)[None, :, None]
        val = (k * key_from[:, None, None]).astype(np.uint32).astype(np.float64)
        return val / (1 << ((j + 1) * basebit)).astype(np.float64)  # [n][t][base]

    @classmethod
    def new_symmetric(cls, key_from, key_to: SecretKey, seed=None, rng_key=None, device=None) -> "ProxyReencryptionKey":
        """proxy_reenc.rs:362-370: the set's key-switch noise, basebit and t."""
        p = key_to.params
        return cls.new_symmetric_with_params(key_from, key_to, p.alpha_lv0, p.basebit, p.iks_t, seed, rng_key, device)

    @classmethod
    def new_symmetric_with_params(cls, key_from, key_to: SecretKey, alpha: float, basebit: int, t: int,
                                  seed=None, rng_key=None, device=None) -> "ProxyReencryptionKey":
        """proxy_reenc.rs:389-425: TLWELv0::encrypt_f64(p, alpha, key_to) per (i, j, k != 0).
        rng_key / device: the keyed format of include/tfhe_hip.h ("symmetric encryption", row base t i + base j + k of
        the "RKM" / "RKS" streams) -- on the CPU with rng_key alone; with `device` the key is generated in a key view of
        that GPU (`tfhe_hip_gen_reenc_key_symmetric`; rng_key=None: a key from getrandom(2)) which the returned object
        keeps, so `reencrypt` uploads nothing.  One rng_key makes one re-encryption key."""
        p = key_to.params
        pts = cls._plaintexts(_key_lv0(key_from), basebit, t)
        if rng_key is not None or device is not None:
            if seed is not None:
                raise ValueError("seed selects numpy's generator; rng_key / device select the keyed format")
            if device is not None:
                from .bootstrap import engine_for

                if p.n > 1024:
                    raise ValueError(f"proxy re-encryption on the GPU needs n <= 1024 ({p.name}: n = {p.n})")
                v = engine_for(_engine_params(p, int(basebit), int(t)), device).new_key_view()
                try:
                    key = cls(p, v.gen_reenc_key_symmetric(_key_lv0(key_from), key_to.key_lv0, alpha, rng_key), basebit, t)
                except Exception:
                    v.close()
                    raise
                key._view = (device, v)
                return key
            rows = np.arange(pts.size, dtype=np.uint64)
            live = rows % np.uint64(1 << basebit) != 0
            enc = np.zeros((pts.size, p.n + 1), np.uint32)
            k = _rng_key(rng_key)
            enc[live] = seeded.symmetric_rows(k, k, rows[live], key_to.key_lv0, f64_to_torus(pts.reshape(-1)[live]), alpha,
                                              seeded.DOMAINS_SYM_RK)
            return cls(p, enc, basebit, t)
        enc = key_to.encrypt_f64(pts.reshape(-1), seed, alpha).reshape(p.n, t, 1 << basebit, p.n + 1)
        enc[:, :, 0, :] = 0
        return cls(p, enc, basebit, t)

    @classmethod
    def new_asymmetric(cls, key_from, public_key_to: PublicKeyLv0, seed=None, rng_key=None,
                       device=None) -> "ProxyReencryptionKey":
        """proxy_reenc.rs:271-279."""
        p = public_key_to.params
        return cls.new_asymmetric_with_params(key_from, public_key_to, p.alpha_lv0, p.basebit, p.iks_t, seed, rng_key, device)

    @classmethod
    def new_asymmetric_with_params(cls, key_from, public_key_to: PublicKeyLv0, alpha: float, basebit: int, t: int,
                                   seed=None, rng_key=None, device=None) -> "ProxyReencryptionKey":
        """proxy_reenc.rs:294-330: public_key_to.encrypt_f64(p, alpha) per (i, j, k != 0).
        rng_key / device: the keyed format of include/tfhe_hip.h (row base t i + base j + k) -- on the CPU with rng_key
        alone; with `device` the key is generated in a key view of that GPU (`tfhe_hip_gen_reenc_key_asymmetric`;
        rng_key=None: a key from getrandom(2)) which the returned object keeps, so `reencrypt` uploads nothing."""
        p = public_key_to.params
        pts = cls._plaintexts(_key_lv0(key_from), basebit, t)
        if rng_key is not None or device is not None:
            if seed is not None:
                raise ValueError("seed selects numpy's generator; rng_key / device select the keyed format")
            if device is not None:
                from .bootstrap import engine_for

                if p.n > 1024:
                    raise ValueError(f"proxy re-encryption on the GPU needs n <= 1024 ({p.name}: n = {p.n})")
                v = engine_for(_engine_params(p, int(basebit), int(t)), device).new_key_view()
                try:
                    v.load_public_key(public_key_to.encryptions)
                    key = cls(p, v.gen_reenc_key_asymmetric(_key_lv0(key_from), alpha, rng_key), basebit, t)
                except Exception:
                    v.close()
                    raise
                key._view = (device, v)
                return key
            rows = np.arange(pts.size, dtype=np.uint64)
            live = rows % np.uint64(1 << basebit) != 0
            enc = np.zeros((pts.size, p.n + 1), np.uint32)
            enc[live] = encrypt_rows(public_key_to.encryptions, rng_key, rows[live], f64_to_torus(pts.reshape(-1)[live]),
                                     alpha, (DOMAIN_RKE_SEL, DOMAIN_RKE_NOISE))
            return cls(p, enc, basebit, t)
        enc = public_key_to.encrypt_f64(pts.reshape(-1), alpha, seed).reshape(p.n, t, 1 << basebit, p.n + 1)
        enc[:, :, 0, :] = 0
        return cls(p, enc, basebit, t)

    # ---- the proxy's side: on the GPU -------------------------------------------------------------------------
    def _engine_params(self) -> SecurityParams:
        return _engine_params(self.params, self.basebit, self.t)

    def view(self, device: int = 0):
        """The key view that holds this key (created and loaded on first use; `close()` frees its 0.1 GB)."""
        if self._view is None or self._view[0] != device:
            from .bootstrap import engine_for

            self.close()
            v = engine_for(self._engine_params(), device).new_key_view()
            v.load_reenc_key(self.key_encryptions)
            self._view = (device, v)
        return self._view[1]

    def close(self) -> None:
        """Free the key's device memory (also on garbage collection, and at the end of a `with` block)."""
        if getattr(self, "_view", None) is not None:
            self._view[1].close()
            self._view = None

    def __enter__(self) -> "ProxyReencryptionKey":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reencrypt(self, cts, device: int = 0) -> np.ndarray:
        """reencrypt_tlwe_lv0 (proxy_reenc.rs:468-510) over [count][n+1] (or one [n+1]) ciphertexts."""
        arr = np.ascontiguousarray(cts, dtype=np.uint32)
        out = self.view(device).batch_reencrypt(arr.reshape(-1, self.params.n + 1))
        return out.reshape(arr.shape)


def reencrypt_tlwe_lv0(ct_from, reenc_key: ProxyReencryptionKey, device: int = 0) -> np.ndarray:
    """proxy_reenc.rs:468: the free function of the reference; accepts a batch as well."""
    return reenc_key.reencrypt(ct_from, device)


class PackedReencryptionKey:
    """Proxy re-encryption of PACKED ciphertexts: the TRLWE switching key at k = 1 from Alice's ring key to Bob's
    (include/tfhe_hip.h, "TRLWE key switch").  One step per 8 KiB ciphertext of 1,024 values with a key of t N words
    (24 KiB at t = 6), where the lv0 route above takes one re-encryption of 4 (n + 1) bytes per value.  Symmetric only:
    it is made with both secret keys (an asymmetric, public-key variant is not offered)."""

    def __init__(self, params: SecurityParams, key):
        if key.k != 1:
            raise ValueError("a re-encryption key is the switching key at k = 1")
        self.params = params
        self.key = key  # packing.TrlweSwitchKey
        self._view = None

    @classmethod
    def new_symmetric(cls, alice_sk: SecretKey, bob_sk: SecretKey, basebit: int = 4, t: int = 6, rng_key=None,
                      device: int = 0) -> "PackedReencryptionKey":
        """Generated on GPU `device` (`tfhe_hip_gen_trlwe_switch_key`) in a key view that is closed again: the secrets
        do not stay on the device.  rng_key: the 32-byte generator key, None draws it from getrandom(2); the noise is
        alpha_lv1 of the set."""
        if alice_sk.params != bob_sk.params:
            raise ValueError("the two secret keys belong to different parameter sets")
        from .bootstrap import engine_for

        view = engine_for(alice_sk.params, device).new_key_view()
        try:
            key = view.gen_trlwe_switch_key(alice_sk.key_lv1, bob_sk.key_lv1, 1, basebit, t,
                                            rng_key=None if rng_key is None else _rng_key(rng_key))
        finally:
            view.close()
        return cls(alice_sk.params, key)

    def view(self, device: int = 0):
        """The key view that holds this key (created and loaded on first use; `close()` frees it)."""
        if self._view is None or self._view[0] != device:
            from .bootstrap import engine_for

            self.close()
            v = engine_for(self.params, device).new_key_view()
            v.load_trlwe_switch_key(self.key)
            self._view = (device, v)
        return self._view[1]

    def close(self) -> None:
        if getattr(self, "_view", None) is not None:
            self._view[1].close()
            self._view = None

    def __enter__(self) -> "PackedReencryptionKey":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reencrypt(self, packed, device: int = 0) -> np.ndarray:
        """[count][2][N] (or one [2][N]) packed ciphertexts under Alice's key -> the same under Bob's."""
        arr = np.ascontiguousarray(packed, dtype=np.uint32)
        return self.view(device).batch_trlwe_keyswitch(1, arr).reshape(arr.shape)
