"""Client side of the path: secret keys, TLWE encryption and decryption.

Host-side integer work (numpy, batched over ciphertexts); nothing here touches
the GPU except `cloud_key()`, which runs the key generation kernels, and the calls given `device=`.  Mirrors

  key::SecretKey::new                      src/key.rs:21-48
  TLWELv0::encrypt_f64 / encrypt_bool      src/tlwe.rs:37-58
  TLWELv0::decrypt_bool                    src/tlwe.rs:60-68
  TLWELv0::encrypt_lwe_message             src/tlwe.rs:84-98
  TLWELv0::decrypt_lwe_message             src/tlwe.rs:111-126
  utils::f64_to_torus / gaussian_f64       src/utils.rs:9-38
  CloudKey::new(&secret_key)               src/key.rs:59-66

and the seeded (compressed) forms of include/tfhe_hip.h: `compressed_cloud_key` (on the CPU by default, exact
integer arithmetic in seeded.py) and `encrypt_*_seeded`, which return only the bodies of fresh ciphertexts.

The reference draws from `thread_rng` (an OS-seeded ChaCha CSPRNG).  Here `seed=None` -- the
default everywhere -- draws from the operating system's CSPRNG (`os.urandom`); passing an integer
seed or a numpy Generator selects numpy's PCG64 instead, which is reproducible and NOT
cryptographic: tests and benchmarks only.  A guessable generator behind `SecretKey.new`,
`encrypt_*` or `cloud_key` gives the secret key away.

`encrypt_*` and `encrypt_*_seeded` also exist in the keyed format of include/tfhe_hip.h ("symmetric encryption"):
`rng_key=` (a secret 32-byte generator key) alone is its CPU form, `device=` runs it on the GPU
(`tfhe_hip_batch_encrypt`; rng_key=None there draws the key from getrandom(2)), `first_index=` places the batch in the
streams.  A (rng_key, row) pair must never encrypt twice.  `encrypt_packed_*` take the same arguments with `first_group=`
in the format of the header's "packed encryption" section (`tfhe_hip_batch_encrypt_trlwe`), and `encrypt_packed_*_seeded`
return the bodies alone (seeded.SeededPackedCiphertexts).

`phase`, `decrypt_*` and their packed forms take `device=` too (include/tfhe_hip.h, "decryption"): the numpy expressions
here stay the definition, the GPU returns the same words, and a torch CUDA tensor is decrypted where it lies.
"""
from __future__ import annotations

import os

import numpy as np

from .params import N, SecurityParams


def f64_to_torus(d) -> np.ndarray:
    """utils.rs:9-12, element-wise: ((d % 1.0) * 2^32) as i64 as u32 (fmod keeps the sign of d)."""
    t = np.fmod(np.asarray(d, dtype=np.float64), 1.0) * 4294967296.0
    return t.astype(np.int64).astype(np.uint32)


def torus_to_f64(t) -> np.ndarray:
    """utils.rs:14-16."""
    return np.asarray(t, dtype=np.uint32).astype(np.float64) / 4294967296.0


class OsRng:
    """The two draws this module needs, fed by os.urandom (getrandom(2)): the stand-in for the
    reference's OS-seeded thread_rng."""

    def integers(self, low, high, size, dtype=np.uint64):
        span = int(high) - int(low)
        shape = (size,) if np.isscalar(size) else tuple(size)
        count = int(np.prod(shape))
        if span == 2:
            raw = np.frombuffer(os.urandom((count + 7) // 8), np.uint8)
            vals = np.unpackbits(raw)[:count].astype(np.uint64)
        elif span == 1 << 32:
            vals = np.frombuffer(os.urandom(4 * count), np.uint32).astype(np.uint64)
        else:
            raise ValueError("OsRng.integers serves bits and 32-bit words")
        return (vals + np.uint64(int(low))).astype(dtype).reshape(shape)

    def normal(self, mu, sigma, size):
        """Box-Muller over 53-bit uniforms (as the GPU key generator does, keygen.hpp gauss2)."""
        count = int(size)
        u = np.frombuffer(os.urandom(16 * ((count + 1) // 2)), np.uint64).reshape(-1, 2) >> np.uint64(11)
        u1 = (u[:, 0].astype(np.float64) + 1.0) * (1.0 / 9007199254740992.0)  # (0, 1]
        u2 = u[:, 1].astype(np.float64) * (1.0 / 9007199254740992.0)          # [0, 1)
        r = np.sqrt(-2.0 * np.log(u1)) * sigma
        return (mu + np.concatenate([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)]))[:count]


def _rng(seed):
    """None -> OsRng (cryptographic); int / numpy Generator -> PCG64 (reproducible, tests only)."""
    if seed is None:
        return OsRng()
    return seed if isinstance(seed, (np.random.Generator, OsRng)) else np.random.default_rng(seed)


class SecretKey:
    """key_lv0 in {0,1}^n (the TLWE key ciphertexts live under), key_lv1 in {0,1}^N (the ring key)."""

    def __init__(self, params: SecurityParams, key_lv0, key_lv1):
        self.params = params
        self.key_lv0 = np.ascontiguousarray(key_lv0, dtype=np.uint32).reshape(params.n)
        self.key_lv1 = np.ascontiguousarray(key_lv1, dtype=np.uint32).reshape(N)
        if self.key_lv0.max(initial=0) > 1 or self.key_lv1.max(initial=0) > 1:
            raise ValueError("secret keys are binary")

    @classmethod
    def new(cls, params: SecurityParams, seed=None) -> "SecretKey":
        """key.rs:33-48: uniform bits."""
        g = _rng(seed)
        return cls(params, g.integers(0, 2, params.n, dtype=np.uint32), g.integers(0, 2, N, dtype=np.uint32))

    # ---- TLWE level 0 -----------------------------------------------------------------------
    def _inner(self, cts: np.ndarray) -> np.ndarray:
        # sum of the mask words the key selects, wrapping in u32
        return (cts[:, :-1] * self.key_lv0[None, :]).sum(axis=1, dtype=np.uint32)

    def _cts(self, cts) -> np.ndarray:
        return np.ascontiguousarray(cts, dtype=np.uint32).reshape(-1, self.params.n + 1)

    def _keyed(self, seed, rng_key, first_index, device, count: int) -> bool:
        """Whether a call asks for the keyed format of include/tfhe_hip.h ("symmetric encryption"), with its checks"""
        if rng_key is None and device is None:
            if int(first_index) != 0:
                raise ValueError("first_index belongs to the keyed format: give rng_key or device")
            return False
        if seed is not None:
            raise ValueError("seed selects numpy's generator; rng_key / device select the keyed format")
        if rng_key is not None and (not isinstance(rng_key, (bytes, bytearray)) or len(rng_key) != 32):
            raise ValueError("rng_key is 32 bytes")
        if not (0 <= int(first_index) and int(first_index) + count <= 1 << 64):
            raise ValueError("the ciphertext indices run past 2^64")
        return True

    def _encrypt_keyed(self, p, alpha, rng_key, mask_seed, first_index, device, full: bool):
        """encrypt_f64 in the keyed format: [count][n+1] (full) or seeded.SeededCiphertexts"""
        from .seeded import DOMAINS_SYM_TLWE, SeededCiphertexts, symmetric_rows

        mask_seed = os.urandom(32) if mask_seed is None else bytes(mask_seed)
        if len(mask_seed) != 32:
            raise ValueError("mask_seed is 32 bytes")
        if device is not None:
            from .bootstrap import engine_for

            return engine_for(self.params, device).batch_encrypt(self.key_lv0, f64_to_torus(p), alpha, rng_key, mask_seed,
                                                                 first_index, full=full, bodies=not full)
        rows = np.uint64(int(first_index)) + np.arange(len(p), dtype=np.uint64)
        got = symmetric_rows(mask_seed, bytes(rng_key), rows, self.key_lv0, f64_to_torus(p), alpha, DOMAINS_SYM_TLWE, full)
        return got if full else SeededCiphertexts(self.params, mask_seed, first_index, got)

    def encrypt_f64(self, p, seed=None, alpha: float | None = None, rng_key=None, first_index: int = 0, device=None,
                    mask_seed: bytes = None) -> np.ndarray:
        """tlwe.rs:37-53: a uniform, b = <a, s> + f64_to_torus(p) + f64_to_torus(N(0, alpha)).
        p: scalar or [count]; returns [count][n+1] u32.
        rng_key / first_index / device: the keyed format of include/tfhe_hip.h ("symmetric encryption"), ciphertext m at
        row first_index + m: masks under the public mask_seed (None: fresh from the OS), noise under the secret 32-byte
        rng_key -- on the CPU with rng_key alone, on GPU `device` otherwise (rng_key=None there: a key from
        getrandom(2)).  A (rng_key, row) pair must never encrypt twice."""
        p = np.atleast_1d(np.asarray(p, dtype=np.float64))
        alpha = self.params.alpha_lv0 if alpha is None else alpha
        if self._keyed(seed, rng_key, first_index, device, len(p)):
            return self._encrypt_keyed(p, alpha, rng_key, mask_seed, first_index, device, True)
        g = _rng(seed)
        out = np.empty((len(p), self.params.n + 1), np.uint32)
        out[:, :-1] = g.integers(0, 1 << 32, (len(p), self.params.n), dtype=np.uint64).astype(np.uint32)
        noise = f64_to_torus(g.normal(0.0, alpha, len(p))) if alpha > 0 else np.zeros(len(p), np.uint32)
        out[:, -1] = self._inner(out) + f64_to_torus(p) + noise
        return out

    def encrypt_bool(self, bits, seed=None, alpha: float | None = None, rng_key=None, first_index: int = 0, device=None,
                     mask_seed: bytes = None) -> np.ndarray:
        """tlwe.rs:55-58: true -> +1/8, false -> -1/8."""
        bits = np.atleast_1d(np.asarray(bits)).astype(bool)
        return self.encrypt_f64(np.where(bits, 0.125, -0.125), seed, alpha, rng_key, first_index, device, mask_seed)

    def _on_device(self, device, cts, mode, modulus=None, *, lv1=False, packed_count=None):
        """The decode `mode` of cts on GPU `device` (include/tfhe_hip.h, "decryption"): a numpy argument goes through the
        host form and comes back as a numpy array, a torch CUDA tensor through the _dev form on its current stream and
        comes back as a tensor on that device.  [count] 32-bit words."""
        from .bootstrap import engine_for

        e = engine_for(self.params, device)
        key = self.key_lv1 if lv1 or packed_count is not None else self.key_lv0
        if type(cts).__module__.startswith("torch"):
            import torch

            if packed_count is not None:
                cts = cts.reshape(-1, 2, N)
                if cts.shape[0] * N < packed_count:
                    raise ValueError(f"{cts.shape[0]} packed TRLWEs hold fewer than {packed_count} results")
                out = torch.empty(int(packed_count), dtype=torch.int32, device=cts.device)
                if packed_count:
                    e.batch_decrypt_trlwe_dev(key, cts, packed_count, out, mode, modulus)
                return out
            cts = cts.reshape(-1, len(key) + 1)
            out = torch.empty(cts.shape[0], dtype=torch.int32, device=cts.device)
            if cts.shape[0]:
                e.batch_decrypt_dev(key, cts, out, mode, modulus)
            return out
        if packed_count is not None:
            packed = np.ascontiguousarray(cts, dtype=np.uint32).reshape(-1, 2, N)
            if len(packed) * N < packed_count:
                raise ValueError(f"{len(packed)} packed TRLWEs hold fewer than {packed_count} results")
            return e.batch_decrypt_trlwe(key, packed, packed_count, mode, modulus) if packed_count else np.empty(0, np.uint32)
        cts = np.ascontiguousarray(cts, dtype=np.uint32).reshape(-1, len(key) + 1)
        return e.batch_decrypt(key, cts, mode, modulus) if len(cts) else np.empty(0, np.uint32)

    @staticmethod
    def _as(words, dtype):
        """The [count] words of a device decode in the dtype the numpy path returns (bool / int64)"""
        if isinstance(words, np.ndarray):
            return words.astype(dtype)
        import torch

        return words.to(torch.bool if dtype is bool else torch.int64)

    def phase(self, cts, device=None):
        """b - <a, s> (u32).  device: computed on that GPU (numpy in, numpy out through the host form; a torch CUDA
        tensor in, a tensor of the same 32-bit words out through the _dev form); None: numpy on the host."""
        if device is not None:
            return self._on_device(device, cts, "phase")
        cts = self._cts(cts)
        return cts[:, -1] - self._inner(cts)

    def phase_lv1(self, rows, device=None):
        """b - <a, s1> (u32) of lv1 rows [count][N+1] under key_lv1: what batch_sample_extract and
        batch_trlwe_matmul(keyswitch=False) return.  device as in phase."""
        if device is not None:
            return self._on_device(device, rows, "phase", lv1=True)
        rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, N + 1)
        return rows[:, -1] - (rows[:, :-1] * self.key_lv1[None, :]).sum(axis=1, dtype=np.uint32)

    def decrypt_bool(self, cts, device=None):
        """tlwe.rs:60-68: the phase read as i32 is non-negative.  device as in phase."""
        if device is not None:
            return self._as(self._on_device(device, cts, "bool"), bool)
        return self.phase(cts).view(np.int32) >= 0

    def encrypt_lwe_message(self, msgs, message_modulus: int, seed=None, alpha: float | None = None, rng_key=None,
                            first_index: int = 0, device=None, mask_seed: bytes = None) -> np.ndarray:
        """tlwe.rs:84-98: (msg mod m) / (2m)."""
        m = int(message_modulus)
        msgs = np.atleast_1d(np.asarray(msgs)).astype(np.int64) % m
        return self.encrypt_f64(msgs.astype(np.float64) * (1.0 / (2.0 * m)), seed, alpha, rng_key, first_index, device,
                                mask_seed)

    def decrypt_lwe_message(self, cts, message_modulus: int, device=None):
        """tlwe.rs:111-126: ((phase / 2^32) / scale + 0.5) as usize % m, scale = 1/(2m).  device as in phase."""
        m = int(message_modulus)
        if device is not None:
            return self._as(self._on_device(device, cts, "message", m), np.int64)
        scale = 1.0 / (2.0 * m)
        return (torus_to_f64(self.phase(cts)) / scale + 0.5).astype(np.int64) % m

    # ---- packed results (packing key switch, include/tfhe_hip.h) ------------------------------------
    def packing_key(self, rng_key=None, alpha=None, device: int = None):
        """The packing key (packing.PackingKey: mask seed + bodies) under s1 for bits of s0.  device=None makes it on
        the CPU; device=d runs `tfhe_hip_gen_packing_key` there, in a key view it closes after.  rng_key: None draws from
        the OS CSPRNG; 32 bytes are the generator key K of include/tfhe_hip.h (CPU and GPU give the same mask seed and,
        away from borderline samples, the same bodies); an int seed is reproducible (tests only, CPU only).  alpha:
        alpha_lv1 by default."""
        if device is None:
            from .packing import make_packing_key

            return make_packing_key(self.params, self.key_lv0, self.key_lv1, rng=rng_key, alpha=alpha)
        if rng_key is not None and not isinstance(rng_key, (bytes, bytearray)):
            raise ValueError("on a device rng_key is the 32-byte generator key (or None): a seed selects the CPU generator")
        from .bootstrap import engine_for

        view = engine_for(self.params, device).new_key_view()
        try:
            return view.gen_packing_key(self.key_lv0, self.key_lv1, rng_key=rng_key, alpha=alpha)
        finally:
            view.close()

    def packed_phase(self, packed, count: int, device=None):
        """Phases of the first `count` results of [G][2][N] packed TRLWEs: coefficient j of B - A (*) s1 per group.
        device as in phase."""
        from .seeded import negacyclic_binary

        if device is not None:
            return self._on_device(device, packed, "phase", packed_count=int(count))
        packed = np.ascontiguousarray(packed, dtype=np.uint32).reshape(-1, 2, N)
        if len(packed) * N < count:
            raise ValueError(f"{len(packed)} packed TRLWEs hold fewer than {count} results")
        return (packed[:, 1] - negacyclic_binary(packed[:, 0], self.key_lv1)).reshape(-1)[:count]

    def decrypt_packed_bool(self, packed, count: int, device=None):
        """decrypt_bool of packed results.  device as in phase."""
        if device is not None:
            return self._as(self._on_device(device, packed, "bool", packed_count=int(count)), bool)
        return self.packed_phase(packed, count).view(np.int32) >= 0

    def decrypt_packed_lwe_message(self, packed, count: int, message_modulus: int, device=None):
        """decrypt_lwe_message of packed results.  device as in phase."""
        m = int(message_modulus)
        if device is not None:
            return self._as(self._on_device(device, packed, "message", m, packed_count=int(count)), np.int64)
        return (torus_to_f64(self.packed_phase(packed, count)) / (1.0 / (2.0 * m)) + 0.5).astype(np.int64) % m

    # ---- packed inputs (unpacking key switch, include/tfhe_hip.h) ------------------------------------
    def _encrypt_packed_keyed(self, p, alpha, rng_key, mask_seed, first_group, device, full: bool):
        """encrypt_packed_f64 in the keyed format of include/tfhe_hip.h ("packed encryption"): [groups][2][N] (full) or
        seeded.SeededPackedCiphertexts"""
        from .seeded import SeededPackedCiphertexts, symmetric_trlwe_rows

        mask_seed = os.urandom(32) if mask_seed is None else bytes(mask_seed)
        if len(mask_seed) != 32:
            raise ValueError("mask_seed is 32 bytes")
        groups = -(-len(p) // N)
        if device is not None:
            from .bootstrap import engine_for

            return engine_for(self.params, device).batch_encrypt_trlwe(self.key_lv1, f64_to_torus(p), alpha, rng_key, mask_seed,
                                                                       first_group, full=full, bodies=not full)
        idx = np.uint64(int(first_group)) + np.arange(groups, dtype=np.uint64)
        got = symmetric_trlwe_rows(mask_seed, bytes(rng_key), idx, self.key_lv1, f64_to_torus(p), len(p), alpha, full)
        return got if full else SeededPackedCiphertexts(self.params, mask_seed, first_group, got, len(p))

    def encrypt_packed_f64(self, p, seed=None, alpha: float | None = None, rng_key=None, first_group: int = 0, device=None,
                           mask_seed: bytes = None) -> np.ndarray:
        """TRLWELv1::encrypt_f64 (trlwe.rs:30-53) over [count] values, N to a ciphertext: per group a uniform,
        b = a (*) s1 + f64_to_torus(N(0, alpha)) + f64_to_torus(p) per coefficient, alpha_lv1 by default.  Returns
        [ceil(count / N)][2][N] u32 under key_lv1; the unused slots of the last group encrypt 0.
        rng_key / first_group / device: the keyed format of include/tfhe_hip.h ("packed encryption"), group m at index
        first_group + m: masks under the public mask_seed (None: fresh from the OS), noise under the secret 32-byte
        rng_key -- on the CPU with rng_key alone, on GPU `device` otherwise (rng_key=None there: a key from
        getrandom(2)).  A (rng_key, group) pair must never encrypt twice."""
        from .seeded import negacyclic_binary

        p = np.atleast_1d(np.asarray(p, dtype=np.float64)).reshape(-1)
        alpha = self.params.alpha_lv1 if alpha is None else alpha
        groups = -(-len(p) // N)
        if mask_seed is not None and rng_key is None and device is None:
            raise ValueError("mask_seed belongs to the keyed format: give rng_key or device")
        if self._keyed(seed, rng_key, first_group, device, groups):
            return self._encrypt_packed_keyed(p, alpha, rng_key, mask_seed, first_group, device, True)
        g = _rng(seed)
        msg = np.zeros(groups * N, np.float64)
        msg[:len(p)] = p
        out = np.empty((groups, 2, N), np.uint32)
        out[:, 0] = g.integers(0, 1 << 32, (groups, N), dtype=np.uint64).astype(np.uint32)
        noise = f64_to_torus(g.normal(0.0, alpha, groups * N)) if alpha > 0 else np.zeros(groups * N, np.uint32)
        out[:, 1] = negacyclic_binary(out[:, 0], self.key_lv1) + (f64_to_torus(msg) + noise).reshape(groups, N)
        return out

    def encrypt_packed_bool(self, bits, seed=None, alpha: float | None = None, rng_key=None, first_group: int = 0,
                            device=None, mask_seed: bytes = None) -> np.ndarray:
        """TRLWELv1::encrypt_bool (trlwe.rs:55-66): true -> +1/8, false -> -1/8, slot m = bit m."""
        bits = np.atleast_1d(np.asarray(bits)).astype(bool)
        return self.encrypt_packed_f64(np.where(bits, 0.125, -0.125), seed, alpha, rng_key, first_group, device, mask_seed)

    def encrypt_packed_lwe_message(self, msgs, message_modulus: int, seed=None, alpha: float | None = None, rng_key=None,
                                   first_group: int = 0, device=None, mask_seed: bytes = None) -> np.ndarray:
        """encrypt_lwe_message's encoding, (msg mod m) / (2m), in the slots of packed ciphertexts."""
        m = int(message_modulus)
        msgs = np.atleast_1d(np.asarray(msgs)).astype(np.int64) % m
        return self.encrypt_packed_f64(msgs.astype(np.float64) * (1.0 / (2.0 * m)), seed, alpha, rng_key, first_group, device,
                                       mask_seed)

    def encrypt_packed_f64_seeded(self, p, mask_seed: bytes = None, first_group: int = 0, alpha: float | None = None,
                                  rng_key=None, device=None):
        """encrypt_packed_f64 in the seeded form: returns seeded.SeededPackedCiphertexts (bodies only, 4 KiB a
        ciphertext).  Keyed format only: rng_key alone is the CPU form, device= runs on that GPU, where no mask is
        stored at all.  mask_seed=None draws a fresh one from the OS.  Never encrypt twice under one (mask_seed, group)
        or one (rng_key, group)."""
        p = np.atleast_1d(np.asarray(p, dtype=np.float64)).reshape(-1)
        alpha = self.params.alpha_lv1 if alpha is None else alpha
        if not self._keyed(None, rng_key, first_group, device, -(-len(p) // N)):
            raise ValueError("the seeded packed form is keyed: give rng_key or device")
        return self._encrypt_packed_keyed(p, alpha, rng_key, mask_seed, first_group, device, False)

    def encrypt_packed_bool_seeded(self, bits, mask_seed: bytes = None, first_group: int = 0, alpha: float | None = None,
                                   rng_key=None, device=None):
        """encrypt_packed_bool in the seeded form (see encrypt_packed_f64_seeded)."""
        bits = np.atleast_1d(np.asarray(bits)).astype(bool)
        return self.encrypt_packed_f64_seeded(np.where(bits, 0.125, -0.125), mask_seed, first_group, alpha, rng_key, device)

    def encrypt_packed_lwe_message_seeded(self, msgs, message_modulus: int, mask_seed: bytes = None, first_group: int = 0,
                                          alpha: float | None = None, rng_key=None, device=None):
        """encrypt_packed_lwe_message in the seeded form (see encrypt_packed_f64_seeded)."""
        m = int(message_modulus)
        msgs = np.atleast_1d(np.asarray(msgs)).astype(np.int64) % m
        return self.encrypt_packed_f64_seeded(msgs.astype(np.float64) * (1.0 / (2.0 * m)), mask_seed, first_group, alpha,
                                              rng_key, device)

    # ---- TRGSW selectors (packed CMUX, include/tfhe_hip.h) -------------------------------------------
    def encrypt_trgsw(self, mu, basebit: int = 6, t: int = 3, alpha: float | None = None, rng_key=None, first_index: int = 0,
                      device=None):
        """TRGSW selectors of the message polynomials mu (small integers, [N]: one packing.Trgsw; [count][N]: a list)
        under key_lv1, in the format of include/tfhe_hip.h ("packed CMUX") -- TRGSWLv1::encrypt_torus (trgsw.rs:29-49)
        is mu = a constant.  device=None makes them on the CPU (numpy), device=d runs `tfhe_hip_batch_encrypt_trgsw`
        there; rng_key is the 32-byte generator key K (None: fresh from the OS), under which both give the same mask
        seed and, away from borderline noise samples, the same words.  Row `row` of selector m takes index
        first_index + m 2t + row; a (K, index) pair must never encrypt twice.  alpha: alpha_lv1 by default."""
        from .packing import Trgsw, encrypt_trgsw_rows

        mu = np.asarray(mu)
        one = mu.ndim == 1
        mu = np.ascontiguousarray(mu, dtype=np.int32).reshape(-1, N)
        alpha = self.params.alpha_lv1 if alpha is None else alpha
        if rng_key is not None and (not isinstance(rng_key, (bytes, bytearray)) or len(rng_key) != 32):
            raise ValueError("rng_key is 32 bytes")
        if device is not None:
            from .bootstrap import engine_for

            rows = engine_for(self.params, device).batch_encrypt_trgsw(self.key_lv1, mu, basebit, t, alpha, rng_key, first_index)
        else:
            rows = encrypt_trgsw_rows(self.key_lv1, mu, basebit, t, alpha, os.urandom(32) if rng_key is None else bytes(rng_key),
                                      first_index)
        sels = [Trgsw(basebit, t, r) for r in rows]
        return sels[0] if one else sels

    def encrypt_trgsw_bool(self, bits, basebit: int = 6, t: int = 3, alpha: float | None = None, rng_key=None,
                           first_index: int = 0, device=None):
        """Selectors of bits: mu = 0 or 1, a constant polynomial (a scalar: one packing.Trgsw; an array: a list)."""
        bits = np.asarray(bits)
        mu = np.zeros((bits.size, N), np.int32)
        mu[:, 0] = bits.reshape(-1).astype(bool)
        return self.encrypt_trgsw(mu[0] if bits.ndim == 0 else mu, basebit, t, alpha, rng_key, first_index, device)

    # ---- evaluation key ----------------------------------------------------------------------
    def cloud_key(self, seed=None, device: int = 0):
        """CloudKey::new(&secret_key) (key.rs:59-66): generated on the GPU in a fresh key view of the shared context
        for `device` (which stays resident as this key's view: first use uploads nothing), and returned in the
        reference layouts.  seed=None: the generator key comes from the OS (`tfhe_hip_gen_cloud_key_secure`); an
        integer seed gives a reproducible, guessable key (tests only)."""
        from .bootstrap import adopt_view, engine_for

        view = engine_for(self.params, device).new_key_view()
        view.gen_cloud_key(self.key_lv0, self.key_lv1, seed)
        ck = view.export_cloud_key()
        adopt_view(ck, view)
        return ck

    def compressed_cloud_key(self, rng_key: bytes = None, device: int = None, alpha_ksk=None, alpha_bsk=None):
        """The cloud key in its seeded form (key.CompressedCloudKey; format in include/tfhe_hip.h).  device=None makes it
        on the CPU (numpy, exact: a client needs no GPU); device=d runs `tfhe_hip_gen_compressed_cloud_key` there, in a
        key view it closes after.  rng_key: the 32-byte generator key K; None draws it from the OS.  Both give the same
        mask seed and, at zero noise, the same bodies for one K."""
        from .key import CompressedCloudKey
        from .seeded import compress

        rng_key = os.urandom(32) if rng_key is None else bytes(rng_key)
        if len(rng_key) != 32:
            raise ValueError("rng_key is 32 bytes")
        if device is None:
            seed, bsk, ksk, off = compress(self.params, self.key_lv0, self.key_lv1, rng_key, alpha_ksk, alpha_bsk)
            return CompressedCloudKey(self.params, seed, bsk, ksk, off)
        from .bootstrap import engine_for

        view = engine_for(self.params, device).new_key_view()
        try:
            return view.gen_compressed_cloud_key(self.key_lv0, self.key_lv1, rng_key=rng_key, alpha_ksk=alpha_ksk,
                                                 alpha_bsk=alpha_bsk)
        finally:
            view.close()

    def encrypt_f64_seeded(self, p, mask_seed: bytes = None, first_index: int = 0, seed=None, alpha: float | None = None,
                           rng_key=None, device=None):
        """encrypt_f64 with the masks of the seeded TLWE format: returns seeded.SeededCiphertexts (bodies only).
        mask_seed=None draws a fresh one from the OS.  Never encrypt twice under one (mask_seed, index): the
        difference of the two bodies is the difference of the messages plus noise.  `seed` / `alpha` pick the noise
        as in encrypt_f64.  rng_key / device: the noise in the keyed format of include/tfhe_hip.h ("symmetric
        encryption") -- on the CPU with rng_key alone, on GPU `device` otherwise, where no mask is made at all."""
        from .seeded import SeededCiphertexts, tlwe_masks

        p = np.atleast_1d(np.asarray(p, dtype=np.float64))
        alpha = self.params.alpha_lv0 if alpha is None else alpha
        if (rng_key is not None or device is not None) and self._keyed(seed, rng_key, first_index, device, len(p)):
            return self._encrypt_keyed(p, alpha, rng_key, mask_seed, first_index, device, False)
        mask_seed = os.urandom(32) if mask_seed is None else bytes(mask_seed)
        g = _rng(seed)
        sc = SeededCiphertexts(self.params, mask_seed, first_index, np.zeros(len(p), np.uint32))
        if int(first_index) + len(p) > 1 << 64:
            raise ValueError("the ciphertext indices run past 2^64")
        noise = f64_to_torus(g.normal(0.0, alpha, len(p))) if alpha > 0 else np.zeros(len(p), np.uint32)
        s0 = self.key_lv0.astype(bool)
        for lo in range(0, len(p), 8192):
            hi = min(lo + 8192, len(p))
            masks = tlwe_masks(sc.mask_seed, sc.first_index + lo, hi - lo, self.params.n)
            inner = masks[:, s0].sum(axis=1, dtype=np.uint64).astype(np.uint32)
            sc.bodies[lo:hi] = inner + f64_to_torus(p[lo:hi]) + noise[lo:hi]
        return sc

    def encrypt_bool_seeded(self, bits, mask_seed: bytes = None, first_index: int = 0, seed=None,
                            alpha: float | None = None, rng_key=None, device=None):
        """encrypt_bool in the seeded form (see encrypt_f64_seeded)."""
        bits = np.atleast_1d(np.asarray(bits)).astype(bool)
        return self.encrypt_f64_seeded(np.where(bits, 0.125, -0.125), mask_seed, first_index, seed, alpha, rng_key, device)

    def encrypt_lwe_message_seeded(self, msgs, message_modulus: int, mask_seed: bytes = None, first_index: int = 0,
                                   seed=None, alpha: float | None = None, rng_key=None, device=None):
        """encrypt_lwe_message in the seeded form (see encrypt_f64_seeded)."""
        m = int(message_modulus)
        msgs = np.atleast_1d(np.asarray(msgs)).astype(np.int64) % m
        return self.encrypt_f64_seeded(msgs.astype(np.float64) * (1.0 / (2.0 * m)), mask_seed, first_index, seed, alpha,
                                       rng_key, device)
