"""CloudKey: the evaluation key bundle of the reference (src/key.rs:51-56).

This class carries the four fields the hot path borrows, in the flat layouts of
include/tfhe_hip.h.  `CloudKey.new(secret_key)` (src/key.rs:59-66) generates them on
the GPU (client.SecretKey.cloud_key -> tfhe_hip_gen_cloud_key).
"""
from __future__ import annotations

import numpy as np

from .params import N, SecurityParams, f64_to_torus, gen_decomposition_offset


def gen_testvec() -> np.ndarray:
    """src/key.rs:91-100: a = 0, b = f64_to_torus(0.125)."""
    tv = np.zeros((2, N), np.uint32)
    tv[1, :] = f64_to_torus(0.125)
    return tv


class CloudKey:
    @classmethod
    def new(cls, secret_key, seed=None, device: int = 0) -> "CloudKey":
        """CloudKey::new(&secret_key), src/key.rs:59-66.  seed=None draws the generator key from the OS;
        an integer seed is for reproducible tests only (see client.SecretKey.cloud_key)."""
        return secret_key.cloud_key(seed, device)

    def __init__(self, params: SecurityParams, bootstrapping_key, key_switching_key,
                 decomposition_offset=None, blind_rotate_testvec=None):
        self.params = params
        self.decomposition_offset = (
            gen_decomposition_offset(params) if decomposition_offset is None else int(decomposition_offset)
        )
        self.blind_rotate_testvec = gen_testvec() if blind_rotate_testvec is None else np.ascontiguousarray(
            blind_rotate_testvec, dtype=np.uint32
        ).reshape(2, N)
        self.bootstrapping_key = np.ascontiguousarray(bootstrapping_key, dtype=np.float64).reshape(
            params.n, 2 * params.l, 2, N
        )
        self.key_switching_key = np.ascontiguousarray(key_switching_key, dtype=np.uint32).reshape(
            N, params.iks_t, params.base, params.n + 1
        )


class CompressedCloudKey:
    """A cloud key in the seeded form of include/tfhe_hip.h: the public 32-byte mask seed S, the BSK bodies
    [n][2l][N] u32 and the KSK bodies [N][t][base] u32.  The masks are regenerated from S on the device
    (`Engine.load_compressed_cloud_key`): about a tenth of the full key on SECURITY_128_BIT, a fiftieth on
    SECURITY_UINT4."""

    FORMAT_VERSION = 1

    def __init__(self, params: SecurityParams, mask_seed, bsk_bodies, ksk_bodies, decomposition_offset=None,
                 blind_rotate_testvec=None):
        self.params = params
        self.mask_seed = bytes(mask_seed)
        if len(self.mask_seed) != 32:
            raise ValueError("mask_seed is 32 bytes")
        self.bsk_bodies = np.ascontiguousarray(bsk_bodies, dtype=np.uint32)
        self.ksk_bodies = np.ascontiguousarray(ksk_bodies, dtype=np.uint32)
        if self.bsk_bodies.size != params.n * 2 * params.l * N:
            raise ValueError("bsk_bodies has the wrong size for these parameters")
        if self.ksk_bodies.size != N * params.iks_t * params.base:
            raise ValueError("ksk_bodies has the wrong size for these parameters")
        self.bsk_bodies = self.bsk_bodies.reshape(params.n, 2 * params.l, N)
        self.ksk_bodies = self.ksk_bodies.reshape(N, params.iks_t, params.base)
        self.decomposition_offset = (
            gen_decomposition_offset(params) if decomposition_offset is None else int(decomposition_offset)
        )
        self.blind_rotate_testvec = gen_testvec() if blind_rotate_testvec is None else np.ascontiguousarray(
            blind_rotate_testvec, dtype=np.uint32
        ).reshape(2, N)

    @property
    def nbytes(self) -> int:
        """Bytes that travel: bodies and seed (the [2][N] test vector, gen_testvec's by default, not counted)."""
        return self.bsk_bodies.nbytes + self.ksk_bodies.nbytes + len(self.mask_seed)

    def save(self, path) -> None:
        """One .npz file: the parameter set's name, the format version and the fields."""
        with open(path, "wb") as f:
            np.savez(f, format_version=np.uint32(self.FORMAT_VERSION), params=np.array(self.params.name),
                     mask_seed=np.frombuffer(self.mask_seed, np.uint8), bsk_bodies=self.bsk_bodies,
                     ksk_bodies=self.ksk_bodies, decomposition_offset=np.uint32(self.decomposition_offset),
                     blind_rotate_testvec=self.blind_rotate_testvec)

    @classmethod
    def load(cls, path, params: SecurityParams = None) -> "CompressedCloudKey":
        """Inverse of save; refuses another format version, and another parameter set than `params` when given."""
        from .params import PARAM_SETS

        with np.load(path, allow_pickle=False) as z:
            version = int(z["format_version"])
            if version != cls.FORMAT_VERSION:
                raise ValueError(f"compressed cloud key format {version}, this library reads {cls.FORMAT_VERSION}")
            name = str(z["params"])
            if name not in PARAM_SETS:
                raise ValueError(f"unknown parameter set {name!r}")
            if params is not None and params.name != name:
                raise ValueError(f"the file holds a {name} key, not {params.name}")
            return cls(PARAM_SETS[name], z["mask_seed"].tobytes(), z["bsk_bodies"], z["ksk_bodies"],
                       int(z["decomposition_offset"]), z["blind_rotate_testvec"])
