"""Engine: one C-ABI context = one GPU (one process per GPU under torch.distributed)."""
from __future__ import annotations

import ctypes as C
import os
import threading
import weakref
from typing import Optional

import numpy as np

from . import _capi
from .params import N, SecurityParams

# gate selectors (enum tfhe_hip_gate)
NAND, OR, AND, XOR, XNOR, NOR, ANDNY, ANDYN, ORNY, ORYN, COPY = range(11)
GATE_IDS = {
    "nand": NAND, "or": OR, "and": AND, "xor": XOR, "xnor": XNOR, "nor": NOR,
    "and_ny": ANDNY, "and_yn": ANDYN, "or_ny": ORNY, "or_yn": ORYN, "copy": COPY,
}
CMUX_REFERENCE_DIGITS = 1  # TFHE_HIP_CMUX_REFERENCE_DIGITS


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _is_tensor(x) -> bool:
    return type(x).__module__.startswith("torch")


def _tptr(t):
    """Device pointer of a contiguous int32/uint32 CUDA tensor."""
    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous() or t.element_size() != 4:
        raise ValueError("device tensors must be contiguous 32-bit CUDA tensors")
    return C.c_void_p(t.data_ptr())


def pinned_empty(shape, dtype=np.uint32) -> np.ndarray:
    """A numpy array in pinned host memory (`tfhe_hip_host_alloc`).  The host entry points read and write such
    arrays in place over PCIe -- no staging copies -- when every ciphertext operand of the call is pinned."""
    lib = _capi.lib()
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = C.c_void_p()
    rc = lib.tfhe_hip_host_alloc(max(nbytes, 1), C.byref(p))
    if rc != _capi.OK:
        msg = lib.tfhe_hip_last_error(None)
        raise _capi.TfheHipError(rc, msg.decode() if msg else "")
    buf = (C.c_uint8 * max(nbytes, 1)).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    weakref.finalize(buf, lib.tfhe_hip_host_free, C.c_void_p(p.value))  # freed when the last view is gone
    return arr


def _testvec(testvec, count: int):
    """(table, per_ct) of a host bootstrap call: one [2][N] table for the batch, or [count][2][N] for one each."""
    if testvec is None:
        return None, 0
    tv = _u32(testvec)
    per_ct = int(tv.ndim == 3)
    if tv.size != (count if per_ct else 1) * 2 * N:
        raise ValueError("test vector must be [2][N], or [count][2][N] for per-ciphertext tables")
    return tv, per_ct


def _out_like(a: np.ndarray, out) -> np.ndarray:
    if out is None:
        return np.empty_like(a)
    if out.dtype != np.uint32 or out.shape != a.shape or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous uint32 array of the operands' shape")
    return out


def pinned_copy(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    out = pinned_empty(a.shape, a.dtype)
    out[...] = a
    return out


def _seed_bytes(seed) -> bytes:
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("mask_seed is 32 bytes")
    return seed


def _compressed_args(p: SecurityParams, ck):
    """(bsk bodies, ksk bodies, test vector, seed buffer) of a CompressedCloudKey, checked against `p`."""
    bsk, ksk, tv = _u32(ck.bsk_bodies), _u32(ck.ksk_bodies), _u32(ck.blind_rotate_testvec)
    if bsk.size != p.n * 2 * p.l * N or ksk.size != N * p.iks_t * p.base or tv.size != 2 * N:
        raise ValueError("compressed cloud key has the wrong size for these parameters")
    return bsk, ksk, tv, (C.c_uint8 * 32).from_buffer_copy(_seed_bytes(ck.mask_seed))


def device_count() -> int:
    """GPUs this process can open (`tfhe_hip_device_count`): what `Pool(params, range(device_count()))` spans."""
    return int(_capi.lib().tfhe_hip_device_count())


class _Handle:
    """What a context (Engine) and a pool of contexts (Pool) share: the cloud key, the batch calls on host arrays and
    their *_dev forms on torch CUDA tensors, and the lifetime of key views.  A subclass supplies how a C entry point
    is called on its handle (`_call` for `tfhe_hip_<name>` / `tfhe_hip_pool_<name>`; `_call_dev`, whose `home`
    member only a pool's entry points take), `_chk`, `_destroy`, `_device(home)`: the GPU of member `home`, and
    `_member_ctx(member)`: the context handle of a member."""

    # -- lifetime -------------------------------------------------------------
    def _link(self, parent) -> None:
        self._key = None  # the key object currently loaded (held, so its identity cannot be recycled)
        self._packing_key = None  # the packing key loaded beside it (packing.pack loads one once per view)
        self._parent = parent  # a key view keeps its parent alive for as long as it exists
        self._views = []  # weak references to the live key views of this handle (closed before it)
        if parent is not None:
            parent._views.append(weakref.ref(self))

    def close(self) -> None:
        for ref in getattr(self, "_views", []):  # key views go before the handle they run on
            v = ref()
            if v is not None:
                v.close()
        self._views = []
        self._parent = None
        self._destroy()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- cloud key ------------------------------------------------------------
    def load_cloud_key(self, cloud_key) -> None:
        """cloud_key: any object with the reference CloudKey fields (src/key.rs:51-56):
        decomposition_offset, blind_rotate_testvec [2][N], key_switching_key
        [N][t][base][n+1], bootstrapping_key [n][2l][2][N] f64.  A pool uploads it to its first member once and
        replicates it device to device."""
        p = self.params
        bsk = np.ascontiguousarray(cloud_key.bootstrapping_key, dtype=np.float64)
        ksk = _u32(cloud_key.key_switching_key)
        tv = _u32(cloud_key.blind_rotate_testvec)
        if bsk.size != p.n * 2 * p.l * 2 * N:
            raise ValueError("bootstrapping_key has the wrong size for these parameters")
        if ksk.size != N * p.iks_t * p.base * (p.n + 1):
            raise ValueError("key_switching_key has the wrong size for these parameters")
        if tv.size != 2 * N:
            raise ValueError("blind_rotate_testvec must be [2][N]")
        self._call("load_cloud_key", _ptr(bsk), _ptr(ksk), C.c_uint32(int(cloud_key.decomposition_offset)), _ptr(tv))
        self._key = cloud_key

    def load_compressed_cloud_key(self, compressed_key) -> None:
        """`tfhe_hip_load_compressed_cloud_key`: only the bodies are uploaded; the masks are regenerated on the GPU
        (a pool's first member, which replicates the expanded key)."""
        bsk, ksk, tv, seed = _compressed_args(self.params, compressed_key)
        self._call("load_compressed_cloud_key", C.addressof(seed), _ptr(bsk), _ptr(ksk),
                   C.c_uint32(int(compressed_key.decomposition_offset)), _ptr(tv))
        self._key = compressed_key

    def gen_cloud_key(self, key_lv0, key_lv1, seed=None, alpha_ksk=None, alpha_bsk=None, rng_key: bytes = None) -> None:
        """CloudKey::new(&secret_key) (src/key.rs:59-66) on the GPU, straight into this context (or pool).

        seed=None (default): masks and noise come from a ChaCha20 stream keyed by the operating system's CSPRNG
        (`tfhe_hip_gen_cloud_key_secure`), or by the caller's 32-byte `rng_key`.  An integer `seed` makes the key
        reproducible and as guessable as the seed: tests and benchmarks only (include/tfhe_hip.h)."""
        p = self.params
        k0, k1 = _u32(key_lv0).reshape(-1), _u32(key_lv1).reshape(-1)
        if len(k0) != p.n or len(k1) != N:
            raise ValueError("secret key has the wrong size for these parameters")
        a0 = C.c_double(p.alpha_lv0 if alpha_ksk is None else alpha_ksk)
        a1 = C.c_double(p.alpha_lv1 if alpha_bsk is None else alpha_bsk)
        if rng_key is not None:
            if seed is not None or len(rng_key) != 32:
                raise ValueError("rng_key is 32 bytes and excludes seed")
            buf = (C.c_uint8 * 32).from_buffer_copy(bytes(rng_key))
            self._call("gen_cloud_key_with_key", _ptr(k0), _ptr(k1), a0, a1, C.addressof(buf))
        elif seed is None:
            self._call("gen_cloud_key_secure", _ptr(k0), _ptr(k1), a0, a1)
        else:
            self._call("gen_cloud_key", _ptr(k0), _ptr(k1), a0, a1, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF))
        self._key = ("generated", object())

    def export_cloud_key(self):
        """The context's key back as a CloudKey in the reference layouts."""
        return self._export_cloud_key()

    def _export_cloud_key(self, *member):
        from .key import CloudKey

        p = self.params
        bsk = np.empty((p.n, 2 * p.l, 2, N), np.float64)
        ksk = np.empty((N, p.iks_t, p.base, p.n + 1), np.uint32)
        tv = np.empty((2, N), np.uint32)
        off = C.c_uint32(0)
        self._call("export_cloud_key", *member, _ptr(bsk), _ptr(ksk), C.byref(off), _ptr(tv))
        return CloudKey(p, bsk, ksk, int(off.value), tv)

    # -- batched hot path, host arrays -----------------------------------------
    def _cts(self, a) -> np.ndarray:
        return _u32(a).reshape(-1, self.params.n + 1)

    def batch_gate(self, gate: int, a, b=None, out=None) -> np.ndarray:
        """`out`: optional preallocated [count][n+1] uint32 result array -- pass pinned arrays (`pinned_empty`) for
        a, b and out and the call runs without staging copies."""
        a = self._cts(a)
        bb = self._cts(b) if b is not None else None
        if bb is not None and bb.shape != a.shape:
            raise ValueError("operand batches differ in shape")
        out = _out_like(a, out)
        self._call("batch_gate", int(gate), _ptr(a), _ptr(bb), _ptr(out), len(a))
        return out

    def batch_gates_mixed(self, gates, a, b, keyswitch: bool = True) -> np.ndarray:
        """Per-ciphertext gate selectors (one launch for a whole circuit level)."""
        a, b = self._cts(a), self._cts(b)
        g = np.ascontiguousarray(gates, dtype=np.uint8).reshape(-1)
        if len(g) != len(a) or b.shape != a.shape:
            raise ValueError("gates / operand batches differ in length")
        out = np.empty_like(a)
        self._call("batch_gates_mixed" if keyswitch else "batch_gates_mixed_nks", _ptr(g), _ptr(a), _ptr(b), _ptr(out),
                   len(a))
        return out

    def batch_bootstrap(self, cts, testvec=None, keyswitch: bool = True) -> np.ndarray:
        cts = self._cts(cts)
        out = np.empty_like(cts)
        tv, per_ct = _testvec(testvec, len(cts))
        self._call("batch_bootstrap", _ptr(cts), _ptr(tv), per_ct, int(keyswitch), _ptr(out), len(cts))
        return out

    def batch_tlwe_lincomb(self, ca: int, a, cb: int = 0, b=None, cconst: int = 0) -> np.ndarray:
        """ca*a + cb*b on every word, + cconst on the body: TLWE Add / Sub / Neg / AddMul / SubMul
        (src/tlwe.rs:129-214)."""
        a = self._cts(a)
        bb = self._cts(b) if b is not None else None
        if (cb & 0xFFFFFFFF) and (bb is None or bb.shape != a.shape):
            raise ValueError("second operand missing or of a different shape")
        out = np.empty_like(a)
        self._call("batch_tlwe_lincomb", ca & 0xFFFFFFFF, _ptr(a), cb & 0xFFFFFFFF, _ptr(bb), cconst & 0xFFFFFFFF,
                   _ptr(out), len(a))
        return out

    def batch_lincomb_bootstrap(self, ca: int, a, cb: int = 0, b=None, cconst: int = 0, testvec=None,
                                keyswitch: bool = True) -> np.ndarray:
        """bootstrap(ca*a + cb*b + cconst) with an optional LookupTable.poly: the combination is formed in
        the prologue of the blind-rotation kernel (examples/lut_add_two_numbers.rs:124-158)."""
        a = self._cts(a)
        bb = self._cts(b) if b is not None else None
        if (cb & 0xFFFFFFFF) and (bb is None or bb.shape != a.shape):
            raise ValueError("second operand missing or of a different shape")
        tv, per_ct = _testvec(testvec, len(a))
        out = np.empty_like(a)
        self._call("batch_lincomb_bootstrap", ca & 0xFFFFFFFF, _ptr(a), cb & 0xFFFFFFFF, _ptr(bb), cconst & 0xFFFFFFFF,
                   _ptr(tv), per_ct, int(keyswitch), _ptr(out), len(a))
        return out

    def batch_lincomb_bootstrap_many(self, ca: int, a, cb: int = 0, b=None, cconst: int = 0, testvec=None,
                                     n_luts: int = 2, keyswitch: bool = True) -> np.ndarray:
        """Many-LUT bootstrap of ca*a + cb*b + cconst: n_luts functions packed in `testvec`
        (Generator.generate_many_lookup_table) from ONE blind rotation each.  Returns [n_luts][count][n+1]:
        [j] is what batch_lincomb_bootstrap would give for function j alone (tfhe_hip_batch_lincomb_bootstrap_many).
        n_luts, a missing table and a missing second operand are checked by the library."""
        a = self._cts(a)
        bb = self._cts(b) if b is not None else None
        if (cb & 0xFFFFFFFF) and bb is not None and bb.shape != a.shape:
            raise ValueError("second operand of a different shape")
        tv, per_ct = _testvec(testvec, len(a))
        out = np.empty((int(n_luts),) + a.shape, np.uint32) if n_luts in (1, 2, 4, 8) else np.empty(1, np.uint32)
        self._call("batch_lincomb_bootstrap_many", ca & 0xFFFFFFFF, _ptr(a), cb & 0xFFFFFFFF, _ptr(bb),
                   cconst & 0xFFFFFFFF, _ptr(tv), per_ct, int(n_luts), int(keyswitch), _ptr(out), len(a))
        return out

    def batch_blind_rotate(self, cts, testvec=None) -> np.ndarray:
        cts = self._cts(cts)
        out = np.empty((len(cts), 2, N), np.uint32)
        tv = _u32(testvec) if testvec is not None else None
        if tv is not None and tv.size != 2 * N:
            raise ValueError("test vector must be [2][N]")
        self._call("batch_blind_rotate", _ptr(cts), _ptr(tv), _ptr(out), len(cts))
        return out

    def batch_mux(self, a, b, c, naive: bool) -> np.ndarray:
        a, b, c = self._cts(a), self._cts(b), self._cts(c)
        if b.shape != a.shape or c.shape != a.shape:
            raise ValueError("operand batches differ in shape")
        out = np.empty_like(a)
        self._call("batch_mux", int(bool(naive)), _ptr(a), _ptr(b), _ptr(c), _ptr(out), len(a))
        return out

    # -- packing key switch (include/tfhe_hip.h): up to N lv0 results in one TRLWE lv1 under s1 ----------------------
    def load_packing_key(self, packing_key) -> None:
        """packing.PackingKey (mask seed + bodies [n][t][N]) -> this handle, beside its cloud key (every member of a
        pool expands it); packing needs no cloud key, and a cloud-key load leaves the packing key in place."""
        p = self.params
        if packing_key.params != p:
            raise ValueError(f"packing key of {packing_key.params.name} on a {p.name} handle")
        bodies = _u32(packing_key.bodies).reshape(-1)
        if bodies.size != p.n * p.iks_t * N:
            raise ValueError("packing key bodies have the wrong size for these parameters")
        seed = (C.c_uint8 * 32).from_buffer_copy(_seed_bytes(packing_key.mask_seed))
        self._call("load_packing_key", C.addressof(seed), _ptr(bodies))
        self._packing_key = packing_key

    def gen_packing_key(self, key_lv0, key_lv1, rng_key: bytes = None, alpha=None, download: bool = True):
        """The packing key of the secret key, generated on the GPU (`tfhe_hip_gen_packing_key`; a pool's first member,
        whose bodies every other member loads) and left loaded on this handle.  rng_key: the 32-byte generator key K,
        None draws it from getrandom(2); alpha: alpha_lv1 of the set by default.  Returns the packing.PackingKey, or
        None with download=False (the bodies stay on the GPU)."""
        from .packing import PackingKey

        p = self.params
        k0, k1 = _u32(key_lv0).reshape(-1), _u32(key_lv1).reshape(-1)
        if len(k0) != p.n or len(k1) != N:
            raise ValueError("secret key has the wrong size for these parameters")
        rk = None
        if rng_key is not None:
            if len(rng_key) != 32:
                raise ValueError("rng_key is 32 bytes")
            rk = (C.c_uint8 * 32).from_buffer_copy(bytes(rng_key))
        seed = (C.c_uint8 * 32)()
        bodies = np.empty((p.n, p.iks_t, N), np.uint32) if download else None
        self._call("gen_packing_key", _ptr(k0), _ptr(k1), C.c_double(p.alpha_lv1 if alpha is None else alpha),
                   C.addressof(rk) if rk is not None else None, C.addressof(seed), _ptr(bodies))
        self._packing_key = PackingKey(p, bytes(seed), bodies) if download else ("generated", object())
        return self._packing_key if download else None

    def packing_key_is_loaded(self) -> bool:
        return self._lib.tfhe_hip_packing_key_is_loaded(self._member_ctx(0)) == 1  # 0 / 1; anything else is not "loaded"

    def pack(self, cts) -> np.ndarray:
        """[count][n+1] lv0 ciphertexts -> [ceil(count / N)][2][N] TRLWE lv1 (`tfhe_hip_batch_pack_tlwe`)."""
        cts = self._cts(cts)
        out = np.empty((-(-len(cts) // N), 2, N), np.uint32)
        self._call("batch_pack_tlwe", _ptr(cts), len(cts), _ptr(out))
        return out

    def pack_dev(self, cts, out, stream=None, home=None) -> None:
        """Device form: cts [count][n+1] and out [ceil(count / N)][2][N] 32-bit CUDA tensors on the call's GPU."""
        h = self._home(home)
        count = self._dev_batch(h, cts)
        if out is None or out.numel() != -(-count // N) * 2 * N:
            raise ValueError("out must be [ceil(count / N)][2][N]")
        self._call_dev("batch_pack_tlwe_dev", h, self._tp(h, cts), count, self._tp(h, out), self._stream_ptr(h, stream))

    # -- tree bootstrap (include/tfhe_hip.h): any function of two encrypted digits -------------------------------------
    def batch_bootstrap_bivariate(self, x, y, testvecs, m: int, n_luts: int = 1, keyswitch: bool = True) -> np.ndarray:
        """out[c] = f(x[c], y[c]) for digits of modulus m: the m / n_luts many-LUT bootstraps of y with `testvecs`
        [m / n_luts][2][N] (Generator.generate_bivariate_tables), the encrypted-table key switch of their results, then
        the bootstrap of x with that per-ciphertext table (`tfhe_hip_batch_bootstrap_bivariate`).  Needs the cloud key
        and the packing key; m, n_luts and missing tables are checked by the library."""
        x, y = self._cts(x), self._cts(y)
        if y.shape != x.shape:
            raise ValueError("operand batches differ in shape")
        tv = _u32(testvecs) if testvecs is not None else None
        good = isinstance(m, int) and isinstance(n_luts, int) and n_luts > 0 and m % n_luts == 0
        if tv is not None and good and tv.size != (m // n_luts) * 2 * N:
            raise ValueError("testvecs must be [m / n_luts][2][N]")
        out = np.empty_like(x)
        self._call("batch_bootstrap_bivariate", _ptr(x), _ptr(y), _ptr(tv), int(m), int(n_luts), int(keyswitch),
                   _ptr(out), len(x))
        return out

    # -- unpacking key switch (include/tfhe_hip.h): slots of TRLWE lv1 ciphertexts back to lv0 ciphertexts --------------
    def unpack(self, trlwe, count=None, slots=None) -> np.ndarray:
        """[groups][2][N] TRLWE lv1 -> [count][n+1] lv0 ciphertexts under the cloud key's key-switching key
        (`tfhe_hip_batch_unpack_trlwe`).  slots=None takes slots 0 .. count-1 (count=None: every slot); otherwise
        output m takes slot slots[m] (any order, duplicates allowed) and count is len(slots)."""
        trlwe = _u32(trlwe).reshape(-1, 2, N)
        sl = None
        if slots is not None:
            sl = np.ascontiguousarray(slots, dtype=np.uint32).reshape(-1)
            if count is not None and int(count) != len(sl):
                raise ValueError("count differs from len(slots)")
            count = len(sl)
        elif count is None:
            count = len(trlwe) * N
        out = np.empty((int(count), self.params.n + 1), np.uint32)
        self._call("batch_unpack_trlwe", _ptr(trlwe), len(trlwe), _ptr(sl), int(count), _ptr(out))
        return out

    def unpack_dev(self, trlwe, out, count, slots=None, stream=None, home=None) -> None:
        """Device form: trlwe [groups][2][N], out [count][n+1] and slots [count] (or None) 32-bit CUDA tensors on the
        call's GPU.  The slots are not checked (the call only enqueues): every entry is < groups * N."""
        h = self._home(home)
        count = int(count)
        if trlwe is None or trlwe.numel() % (2 * N) != 0:
            raise ValueError("trlwe must be [groups][2][N]")
        if self._dev_batch(h, out) != count:
            raise ValueError("out must be [count][n+1]")
        if slots is not None and slots.numel() != count:
            raise ValueError("slots must be [count]")
        self._call_dev("batch_unpack_trlwe_dev", h, self._tp(h, trlwe), trlwe.numel() // (2 * N), self._tp(h, slots), count,
                       self._tp(h, out), self._stream_ptr(h, stream))

    # -- device-resident path (torch CUDA tensors; enqueue only) ------------------
    # The tensors of a call live on one GPU: an Engine's, or that of pool member `home` (default: pool.home).  A pool
    # computes shard 0 in place there and moves the others to their members and back by grouped RCCL send / receive
    # (or peer copies), in input order (`tfhe_hip_pool_batch_*_dev`, include/tfhe_hip.h).  So Circuit.run_dev,
    # circuit.mux_and_gates_dev and circuit.lut_add_u8_dev take a Pool wherever they take an Engine.
    def _home(self, home):
        """The member a *_dev call names: `home`, or self.home (None on an Engine); refused if there is none such."""
        h = self.home if home is None else int(home)
        self._device(h)
        return h

    def _stream_ptr(self, home, stream):
        """torch's current stream OF THE CALL'S GPU (the torch-current device may be another GPU: a handle from there
        would be an invalid resource here), or the caller's stream, which must live on that GPU."""
        dev = self._device(home)
        if stream is None:
            import torch

            stream = torch.cuda.current_stream(dev)
        elif getattr(stream, "device", None) is not None and stream.device.index != dev:
            raise ValueError(f"stream lives on {stream.device}, the call on cuda:{dev}")
        # torch's default stream is the legacy null stream (handle 0); the C ABI reads NULL as "the
        # context's own stream", so name the null stream explicitly: hipStreamLegacy == (hipStream_t)1
        return C.c_void_p(stream.cuda_stream or 1)

    def _tp(self, home, t):
        """Device pointer of a tensor that must live on the call's GPU (test vectors, outputs, gate codes)."""
        p = _tptr(t)
        if t is not None and t.device.index != self._device(home):
            raise ValueError(f"device tensor lives on {t.device}, the call on cuda:{self._device(home)}")
        return p

    def _dev_batch(self, home, *tensors) -> int:
        """All tensors are [count][n+1] on the call's GPU; returns count."""
        width, dev = self.params.n + 1, self._device(home)
        first = tensors[0]
        for t in tensors:
            if t is None:
                continue
            if t.dim() != 2 or t.shape[1] != width or t.shape[0] != first.shape[0]:
                raise ValueError(f"device tensors must all be [count][{width}]")
            if t.device.index != dev:
                raise ValueError(f"device tensor lives on {t.device}, the call on cuda:{dev}")
        return first.shape[0]

    def batch_gate_dev(self, gate: int, a, b, out, stream=None, home=None) -> None:
        h = self._home(home)
        count = self._dev_batch(h, a, b, out)
        self._call_dev("batch_gate_dev", h, int(gate), self._tp(h, a), self._tp(h, b), self._tp(h, out), count,
                       self._stream_ptr(h, stream))

    def batch_gates_mixed_dev(self, gates, a, b, out, stream=None, keyswitch: bool = True, home=None) -> None:
        """gates: uint8 CUDA tensor [count]; a, b, out: int32 CUDA tensors [count][n+1].  keyswitch=False ends
        in bootstrap_without_key_switch (the first level of Gates::mux, `tfhe_hip_batch_gates_mixed_nks_dev`)."""
        h = self._home(home)
        dev = self._device(h)
        if not gates.is_cuda or gates.element_size() != 1 or not gates.is_contiguous() or gates.device.index != dev:
            raise ValueError(f"gates must be a contiguous uint8 CUDA tensor on cuda:{dev}")
        count = self._dev_batch(h, a, b, out)
        if gates.numel() != count:
            raise ValueError("one gate code per ciphertext")
        self._call_dev("batch_gates_mixed_dev" if keyswitch else "batch_gates_mixed_nks_dev", h,
                       C.c_void_p(gates.data_ptr()), self._tp(h, a), self._tp(h, b), self._tp(h, out), count,
                       self._stream_ptr(h, stream))

    def batch_bootstrap_dev(self, cts, out, testvec=None, per_ct: bool = False, keyswitch: bool = True, stream=None,
                            home=None) -> None:
        h = self._home(home)
        count = self._dev_batch(h, cts, out)
        if testvec is not None and testvec.numel() != (count if per_ct else 1) * 2 * N:
            raise ValueError("test vector must be [2][N], or [count][2][N] with per_ct")
        self._call_dev("batch_bootstrap_dev", h, self._tp(h, cts), self._tp(h, testvec), int(per_ct), int(keyswitch),
                       self._tp(h, out), count, self._stream_ptr(h, stream))

    def batch_tlwe_lincomb_dev(self, ca: int, a, cb: int, b, cconst: int, out, stream=None, home=None) -> None:
        h = self._home(home)
        count = self._dev_batch(h, a, b, out)
        self._call_dev("batch_tlwe_lincomb_dev", h, ca & 0xFFFFFFFF, self._tp(h, a), cb & 0xFFFFFFFF, self._tp(h, b),
                       cconst & 0xFFFFFFFF, self._tp(h, out), count, self._stream_ptr(h, stream))

    def batch_lincomb_bootstrap_dev(self, ca: int, a, cb: int, b, cconst: int, out, testvec=None,
                                    per_ct: bool = False, keyswitch: bool = True, stream=None, home=None) -> None:
        h = self._home(home)
        count = self._dev_batch(h, a, b, out)
        if testvec is not None and testvec.numel() != (count if per_ct else 1) * 2 * N:
            raise ValueError("test vector must be [2][N], or [count][2][N] with per_ct")
        self._call_dev("batch_lincomb_bootstrap_dev", h, ca & 0xFFFFFFFF, self._tp(h, a), cb & 0xFFFFFFFF,
                       self._tp(h, b), cconst & 0xFFFFFFFF, self._tp(h, testvec), int(per_ct), int(keyswitch),
                       self._tp(h, out), count, self._stream_ptr(h, stream))

    def batch_lincomb_bootstrap_many_dev(self, ca: int, a, cb: int, b, cconst: int, out, testvec, n_luts: int = 2,
                                         per_ct: bool = False, keyswitch: bool = True, stream=None, home=None) -> None:
        """Device form of batch_lincomb_bootstrap_many: out is an int32 CUDA tensor [n_luts * count][n+1] (or
        [n_luts][count][n+1]), function-major."""
        h = self._home(home)
        count, width, dev = self._dev_batch(h, a, b), self.params.n + 1, self._device(h)
        if out is None or out.numel() != max(int(n_luts), 1) * count * width or out.device.index != dev:
            raise ValueError(f"out must be [n_luts * count][{width}] on cuda:{dev}")
        if testvec is not None and testvec.numel() != (count if per_ct else 1) * 2 * N:
            raise ValueError("test vector must be [2][N], or [count][2][N] with per_ct")
        self._call_dev("batch_lincomb_bootstrap_many_dev", h, ca & 0xFFFFFFFF, self._tp(h, a), cb & 0xFFFFFFFF,
                       self._tp(h, b), cconst & 0xFFFFFFFF, self._tp(h, testvec), int(per_ct), int(n_luts),
                       int(keyswitch), self._tp(h, out), count, self._stream_ptr(h, stream))

    def batch_blind_rotate_dev(self, cts, out_trlwe, testvec=None, stream=None, home=None) -> None:
        h = self._home(home)
        count = self._dev_batch(h, cts)
        if out_trlwe.numel() != count * 2 * N or (testvec is not None and testvec.numel() != 2 * N):
            raise ValueError("out_trlwe must be [count][2][N], testvec [2][N]")
        self._call_dev("batch_blind_rotate_dev", h, self._tp(h, cts), self._tp(h, testvec), self._tp(h, out_trlwe),
                       count, self._stream_ptr(h, stream))

    def batch_mux_dev(self, a, b, c, out, naive: bool, stream=None, home=None) -> None:
        h = self._home(home)
        count = self._dev_batch(h, a, b, c, out)
        self._call_dev("batch_mux_dev", h, int(naive), self._tp(h, a), self._tp(h, b), self._tp(h, c),
                       self._tp(h, out), count, self._stream_ptr(h, stream))


class Engine(_Handle):
    """Owns a tfhe_hip_ctx.  Host arrays are numpy uint32; *_dev methods take
    torch CUDA tensors (int32 storage of the u32 words) and only enqueue work."""

    home = None  # one GPU: the *_dev calls name no member

    def __init__(self, params: SecurityParams, device: int = 0, _view_of: "Engine" = None):
        self.params = params
        self.device = device
        self._lib = _capi.lib()
        ctx = C.c_void_p()
        if _view_of is not None:  # a key view: another resident cloud key on the parent's context
            rc = self._lib.tfhe_hip_key_create(_view_of._ctx, C.byref(ctx))
            if rc != _capi.OK:
                raise _capi.TfheHipError(rc, "tfhe_hip_key_create failed")
        else:
            cp = _capi.Params(params.n, params.l, params.bgbit, params.basebit, params.iks_t)
            rc = self._lib.tfhe_hip_ctx_create(C.byref(cp), device, C.byref(ctx))
            if rc != _capi.OK:
                msg = self._lib.tfhe_hip_last_error(None)
                raise _capi.TfheHipError(rc, msg.decode() if msg else "")
        self._attach(ctx, None, _view_of)

    def _attach(self, ctx, owner, parent) -> None:
        self._ctx = ctx
        self._owner = owner  # a Pool when the context is borrowed from one (tfhe_hip_pool_ctx): never destroyed here
        self.lock = threading.RLock()  # for callers that want several calls on this handle back to back
        self._last_use = 0
        self._users = 0  # bootstrap.keyed_engine: calls in flight under this view (never evicted while > 0)
        self._link(parent)

    def new_key_view(self) -> "Engine":
        """Another resident cloud key on this context (`tfhe_hip_key_create`): an Engine handle with its own key
        that shares this context's device, streams, scratch buffers and mutex.  Every method works on it; calls
        under different views may come from different threads.  Replaces the reference's `&CloudKey` argument
        (src/bootstrap/mod.rs:23-38): a call names its key by the handle it is made on."""
        base = self._parent if self._parent is not None else self
        return Engine(base.params, base.device, _view_of=base)

    @classmethod
    def from_pool(cls, pool: "Pool", member: int) -> "Engine":
        """The member context of a pool as an Engine (for the device-resident `*_dev` entry points).  The pool keeps
        ownership; do not run pool batch calls while this engine has work in flight (include/tfhe_hip.h)."""
        ctx = pool._lib.tfhe_hip_pool_ctx(pool._h, int(member))
        if not ctx:
            raise ValueError("no such pool member")
        self = cls.__new__(cls)
        self.params, self.device, self._lib = pool.params, pool.devices[member], pool._lib
        self._attach(C.c_void_p(ctx), pool, None)
        self._key = ("pool", object())
        return self

    # -- what a context supplies to the shared calls ---------------------------------------------------------------------
    def _destroy(self) -> None:
        if getattr(self, "_ctx", None) and getattr(self, "_owner", None) is None:
            self._lib.tfhe_hip_ctx_destroy(self._ctx)
        self._ctx = None
        self._owner = None

    def _chk(self, rc: int) -> None:
        _capi.check(self._ctx, rc)

    def _call(self, name: str, *args) -> None:
        self._chk(getattr(self._lib, "tfhe_hip_" + name)(self._ctx, *args))

    def _call_dev(self, name: str, home, *args) -> None:
        self._call(name, *args)  # a context's *_dev entry points take no member: `home` is None

    def _device(self, home) -> int:
        if home is not None:
            raise ValueError("an Engine has no pool members: home must be None")
        return self.device

    def _member_ctx(self, member: int):
        return self._ctx

    @property
    def name(self) -> str:
        return self._lib.tfhe_hip_name().decode()

    # -- seeded (compressed) keys and ciphertexts (include/tfhe_hip.h) ---------------------------------------------
    def gen_compressed_cloud_key(self, key_lv0, key_lv1, rng_key: bytes = None, alpha_ksk=None, alpha_bsk=None):
        """The seeded form of the key (`tfhe_hip_gen_compressed_cloud_key`), returned as a key.CompressedCloudKey;
        this context is left loaded with its expansion.  rng_key=None: the generator key comes from getrandom(2)."""
        from .key import CompressedCloudKey

        p = self.params
        k0, k1 = _u32(key_lv0).reshape(-1), _u32(key_lv1).reshape(-1)
        if len(k0) != p.n or len(k1) != N:
            raise ValueError("secret key has the wrong size for these parameters")
        rk = None
        if rng_key is not None:
            if len(rng_key) != 32:
                raise ValueError("rng_key is 32 bytes")
            rk = (C.c_uint8 * 32).from_buffer_copy(bytes(rng_key))
        seed = (C.c_uint8 * 32)()
        bsk = np.empty((p.n, 2 * p.l, N), np.uint32)
        ksk = np.empty((N, p.iks_t, p.base), np.uint32)
        off = C.c_uint32(0)
        self._chk(self._lib.tfhe_hip_gen_compressed_cloud_key(
            self._ctx, _ptr(k0), _ptr(k1), C.c_double(p.alpha_lv0 if alpha_ksk is None else alpha_ksk),
            C.c_double(p.alpha_lv1 if alpha_bsk is None else alpha_bsk), C.addressof(rk) if rk is not None else None,
            C.addressof(seed), _ptr(bsk), _ptr(ksk), C.byref(off)))
        self._key = ("generated", object())
        return CompressedCloudKey(p, bytes(seed), bsk, ksk, int(off.value))

    def expand_seeded(self, seeded) -> np.ndarray:
        """seeded.SeededCiphertexts -> [count][n+1] u32, expanded on the GPU (`tfhe_hip_expand_seeded_tlwe`)."""
        if seeded.params != self.params:
            raise ValueError(f"seeded ciphertexts of {seeded.params.name} on a {self.params.name} engine")
        bodies = _u32(seeded.bodies).reshape(-1)
        out = np.empty((len(bodies), self.params.n + 1), np.uint32)
        seed = (C.c_uint8 * 32).from_buffer_copy(_seed_bytes(seeded.mask_seed))
        self._chk(self._lib.tfhe_hip_expand_seeded_tlwe(self._ctx, C.addressof(seed), C.c_uint64(int(seeded.first_index)),
                                                        _ptr(bodies), len(bodies), _ptr(out)))
        return out

    def expand_seeded_dev(self, mask_seed: bytes, first_index: int, bodies, out, stream=None) -> None:
        """Device form: bodies [count] and out [count][n+1] torch tensors (32-bit words) on this engine's GPU."""
        if bodies.dim() != 1:
            raise ValueError("bodies must be [count]")
        count = bodies.shape[0]
        if out.dim() != 2 or out.shape[0] != count or out.shape[1] != self.params.n + 1:
            raise ValueError(f"out must be [{count}][{self.params.n + 1}]")
        seed = (C.c_uint8 * 32).from_buffer_copy(_seed_bytes(mask_seed))
        self._chk(self._lib.tfhe_hip_expand_seeded_tlwe_dev(self._ctx, C.addressof(seed), C.c_uint64(int(first_index)),
                                                            self._tp(None, bodies), count, self._tp(None, out),
                                                            self._stream_ptr(None, stream)))

    # -- encrypted linear layers (include/tfhe_hip.h): a plaintext int8 matrix times ciphertexts ------------------------
    @staticmethod
    def _weights(w, bias):
        """(w as C-contiguous [rows][cols] int8, bias as [rows] u32 or None) after the shape checks."""
        w = np.asarray(w)
        if w.ndim != 2 or w.shape[0] < 1 or w.shape[1] < 1:
            raise ValueError("w must be [rows][cols] with rows, cols >= 1")
        if w.dtype != np.int8:
            if not np.issubdtype(w.dtype, np.integer) or w.min() < -128 or w.max() > 127:
                raise ValueError("weights must be integers in [-128, 127]")
        w = np.ascontiguousarray(w, dtype=np.int8)
        if bias is not None:
            bias = _u32(bias).reshape(-1)
            if len(bias) != w.shape[0]:
                raise ValueError("bias must be [rows]")
        return w, bias

    def batch_tlwe_matmul(self, w, cts, bias=None) -> np.ndarray:
        """out[g][r] = sum_j w[r][j] * cts[g][j] + bias[r] on the body (`tfhe_hip_batch_tlwe_matmul`): w [rows][cols]
        int8, cts [groups][cols][n+1] (or [cols][n+1]: one group), bias [rows] torus words or None.  Returns
        [groups][rows][n+1].  Needs no key."""
        from .linear import MAX_COLS

        w, bias = self._weights(w, bias)
        rows, cols = w.shape
        width = self.params.n + 1
        cts = _u32(cts)
        if cols > MAX_COLS or cts.ndim not in (2, 3) or cts.shape[-2:] != (cols, width):
            raise ValueError(f"cts must be [groups][{cols}][{width}] with cols <= {MAX_COLS}")
        groups = cts.shape[0] if cts.ndim == 3 else 1
        out = np.empty((groups, rows, width), np.uint32)
        self._call("batch_tlwe_matmul", _ptr(w), _ptr(bias), rows, cols, _ptr(cts), groups, _ptr(out))
        return out

    def batch_trlwe_matmul(self, w, trlwe, bias=None, keyswitch: bool = True) -> np.ndarray:
        """The same product on slots 0 .. cols-1 of every TRLWE lv1 of trlwe [groups][2][N]
        (`tfhe_hip_batch_trlwe_matmul`).  keyswitch=True: [groups][rows][n+1] lv0 ciphertexts under the cloud key's
        key-switching key; keyswitch=False: [groups][rows][N+1] lv1 ciphertexts, no key needed."""
        w, bias = self._weights(w, bias)
        rows, cols = w.shape
        trlwe = _u32(trlwe)
        if cols > N or trlwe.ndim not in (2, 3) or trlwe.shape[-2:] != (2, N):
            raise ValueError(f"trlwe must be [groups][2][{N}] and cols <= {N}")
        trlwe = trlwe.reshape(-1, 2, N)
        out = np.empty((len(trlwe), rows, (self.params.n if keyswitch else N) + 1), np.uint32)
        self._call("batch_trlwe_matmul", _ptr(w), _ptr(bias), rows, cols, _ptr(trlwe), len(trlwe), int(bool(keyswitch)),
                   _ptr(out))
        return out

    def _dev_weights(self, w, bias):
        """(rows, cols) of a contiguous int8 CUDA tensor w [rows][cols] on this engine's GPU; bias [rows] or None."""
        if w is None or not w.is_cuda or w.dim() != 2 or w.element_size() != 1 or not w.is_contiguous() or \
                w.device.index != self.device or w.shape[0] < 1 or w.shape[1] < 1:
            raise ValueError(f"w must be a contiguous int8 CUDA tensor [rows][cols] on cuda:{self.device}")
        if bias is not None and bias.numel() != w.shape[0]:
            raise ValueError("bias must be [rows]")
        return int(w.shape[0]), int(w.shape[1])

    def batch_tlwe_matmul_dev(self, w, cts, out, bias=None, stream=None) -> None:
        """Device form: w int8 [rows][cols], cts [groups][cols][n+1], out [groups][rows][n+1] and bias [rows] (or None)
        CUDA tensors on this engine's GPU (32-bit words but for w); out must not overlap cts."""
        from .linear import MAX_COLS

        rows, cols = self._dev_weights(w, bias)
        width = self.params.n + 1
        if cols > MAX_COLS or cts is None or cts.dim() != 3 or tuple(cts.shape[1:]) != (cols, width):
            raise ValueError(f"cts must be [groups][{cols}][{width}] with cols <= {MAX_COLS}")
        groups = int(cts.shape[0])
        if out is None or tuple(out.shape) != (groups, rows, width):
            raise ValueError(f"out must be [{groups}][{rows}][{width}]")
        self._call("batch_tlwe_matmul_dev", C.c_void_p(w.data_ptr()), self._tp(None, bias), rows, cols, self._tp(None, cts),
                   groups, self._tp(None, out), self._stream_ptr(None, stream))

    def batch_trlwe_matmul_dev(self, w, trlwe, out, bias=None, keyswitch: bool = True, stream=None) -> None:
        """Device form: trlwe [groups][2][N], out [groups][rows][n+1] (keyswitch) or [groups][rows][N+1]."""
        rows, cols = self._dev_weights(w, bias)
        if cols > N or trlwe is None or trlwe.dim() != 3 or tuple(trlwe.shape[1:]) != (2, N):
            raise ValueError(f"trlwe must be [groups][2][{N}] and cols <= {N}")
        groups = int(trlwe.shape[0])
        width = (self.params.n if keyswitch else N) + 1
        if out is None or tuple(out.shape) != (groups, rows, width):
            raise ValueError(f"out must be [{groups}][{rows}][{width}]")
        self._call("batch_trlwe_matmul_dev", C.c_void_p(w.data_ptr()), self._tp(None, bias), rows, cols,
                   self._tp(None, trlwe), groups, int(bool(keyswitch)), self._tp(None, out), self._stream_ptr(None, stream))

    # -- plaintext polynomial products on packed ciphertexts (include/tfhe_hip.h): TRLWE in, TRLWE out ---------------------
    def batch_trlwe_polymul(self, w, trlwe, bias=None) -> np.ndarray:
        """out[g][r](X) = sum_j w[r][j](X) * trlwe[g][j](X) + bias[r](X) mod X^N + 1 (`tfhe_hip_batch_trlwe_polymul`;
        linear.polymul_model): w [rows][cols][N] int8 (or [N]: one polynomial), trlwe [groups][cols][2][N] (or
        [cols][2][N]: one group; [2][N] with cols == 1), bias [rows][N] torus words or None.  Returns
        [groups][rows][2][N].  Needs no key."""
        from .linear import _packed_inputs, _polys

        w, bias = _polys(w, bias)
        rows, cols = w.shape[:2]
        trlwe = _packed_inputs(trlwe, cols)
        groups = len(trlwe)
        out = np.empty((groups, rows, 2, N), np.uint32)
        self._call("batch_trlwe_polymul", _ptr(w), _ptr(bias), rows, cols, _ptr(trlwe), groups, _ptr(out))
        return out

    def batch_trlwe_polymul_dev(self, w, trlwe, out, bias=None, stream=None) -> None:
        """Device form: w int8 [rows][cols][N], trlwe [groups][cols][2][N], out [groups][rows][2][N] and bias [rows][N]
        (or None) CUDA tensors on this engine's GPU (32-bit words but for w); out must not overlap trlwe."""
        from .linear import MAX_POLY_COLS

        if w is None or not w.is_cuda or w.dim() != 3 or w.element_size() != 1 or not w.is_contiguous() or \
                w.device.index != self.device or w.shape[0] < 1 or not 1 <= w.shape[1] <= MAX_POLY_COLS or w.shape[2] != N:
            raise ValueError(f"w must be a contiguous int8 CUDA tensor [rows][cols][{N}] on cuda:{self.device} "
                             f"with 1 <= cols <= {MAX_POLY_COLS}")
        rows, cols = int(w.shape[0]), int(w.shape[1])
        if bias is not None and tuple(bias.shape) != (rows, N):
            raise ValueError(f"bias must be [rows][{N}]")
        if trlwe is None or trlwe.dim() != 4 or tuple(trlwe.shape[1:]) != (cols, 2, N):
            raise ValueError(f"trlwe must be [groups][{cols}][2][{N}]")
        groups = int(trlwe.shape[0])
        if out is None or tuple(out.shape) != (groups, rows, 2, N):
            raise ValueError(f"out must be [{groups}][{rows}][2][{N}]")
        self._call("batch_trlwe_polymul_dev", C.c_void_p(w.data_ptr()), self._tp(None, bias), rows, cols,
                   self._tp(None, trlwe), groups, self._tp(None, out), self._stream_ptr(None, stream))

    # -- TRLWE key switch (include/tfhe_hip.h): packed re-encryption and slot automorphisms --------------------------------
    def gen_trlwe_switch_key(self, key_from_lv1, key_to_lv1, k: int = 1, basebit: int = 4, t: int = 6,
                             rng_key: bytes = None, alpha=None, download: bool = True):
        """The switching key (k, basebit, t) from ring key `key_from_lv1` to `key_to_lv1`, generated on the GPU
        (`tfhe_hip_gen_trlwe_switch_key`) and left loaded on this handle under k.  rng_key: the 32-byte generator key
        K (one K serves one key per k), None draws it from getrandom(2); alpha: alpha_lv1 of the set by default.
        Returns the packing.TrlweSwitchKey, or None with download=False (the bodies stay on the GPU)."""
        from .packing import TrlweSwitchKey

        k1, k2 = _u32(key_from_lv1).reshape(-1), _u32(key_to_lv1).reshape(-1)
        if len(k1) != N or len(k2) != N:
            raise ValueError(f"ring keys are {N} words")
        rk = None
        if rng_key is not None:
            if len(rng_key) != 32:
                raise ValueError("rng_key is 32 bytes")
            rk = (C.c_uint8 * 32).from_buffer_copy(bytes(rng_key))
        seed = (C.c_uint8 * 32)()
        bodies = np.empty((max(int(t), 0), N), np.uint32) if download else None
        self._call("gen_trlwe_switch_key", _ptr(k1), _ptr(k2), int(k), int(basebit), int(t),
                   C.c_double(self.params.alpha_lv1 if alpha is None else alpha),
                   C.addressof(rk) if rk is not None else None, C.addressof(seed), _ptr(bodies))
        return TrlweSwitchKey(int(k), int(basebit), int(t), bytes(seed), bodies) if download else None

    def load_trlwe_switch_key(self, key) -> None:
        """packing.TrlweSwitchKey (k, basebit, t, mask seed, bodies [t][N]) -> this handle, beside its cloud key, under
        key.k (`tfhe_hip_load_trlwe_switch_key`); up to 16 keys a handle."""
        bodies = _u32(key.bodies).reshape(-1)
        seed = (C.c_uint8 * 32).from_buffer_copy(_seed_bytes(key.mask_seed))
        self._call("load_trlwe_switch_key", int(key.k), int(key.basebit), int(key.t), C.addressof(seed), _ptr(bodies))

    def trlwe_switch_key_is_loaded(self, k: int) -> bool:
        return self._lib.tfhe_hip_trlwe_switch_key_is_loaded(self._ctx, int(k)) == 1

    def drop_trlwe_switch_key(self, k: int) -> None:
        self._call("drop_trlwe_switch_key", int(k))

    def batch_trlwe_keyswitch(self, k: int, trlwe, out=None, stream=None):
        """psi_k of [count][2][N] packed ciphertexts (or [2][N]: one) under the key loaded for k, under that key's target
        secret (`tfhe_hip_batch_trlwe_keyswitch`).  numpy in, numpy out; or a 32-bit CUDA tensor [count][2][N] on this
        engine's GPU in and a tensor out (`out`: where to write, which must not overlap the input; a new tensor by
        default), queued on `stream` (torch's current stream by default)."""
        if _is_tensor(trlwe):
            import torch

            if trlwe.dim() != 3 or tuple(trlwe.shape[1:]) != (2, N):
                raise ValueError(f"trlwe must be [count][2][{N}]")
            if out is None:
                out = torch.empty_like(trlwe)
            elif tuple(out.shape) != tuple(trlwe.shape):
                raise ValueError("out must have the input's shape")
            self._call("batch_trlwe_keyswitch_dev", int(k), self._tp(None, trlwe), int(trlwe.shape[0]), self._tp(None, out),
                       self._stream_ptr(None, stream))
            return out
        trlwe = _u32(trlwe).reshape(-1, 2, N)
        res = np.empty_like(trlwe)
        self._call("batch_trlwe_keyswitch", int(k), _ptr(trlwe), len(trlwe), _ptr(res))
        return res

    def trlwe_switch_times(self) -> dict:
        """Kernel times of the TRLWE key switch's passes since the last call (profiling on)."""
        t = _capi.TrlweSwitchTimes()
        self._chk(self._lib.tfhe_hip_get_trlwe_switch_times(self._ctx, C.byref(t)))
        return {"digits_ms": t.digits_ms, "contraction_ms": t.contraction_ms, "passes": int(t.passes)}

    # -- packed CMUX (include/tfhe_hip.h): caller-held TRGSW selectors --------------------------------------------------
    @staticmethod
    def _trgsw_shape(basebit: int, t: int) -> None:
        from .packing import check_gadget

        check_gadget(basebit, t)

    def batch_trlwe_cmux(self, sel, basebit: int, t: int, d0, d1, reference_digits: bool = False, out=None, stream=None):
        """out = d0 + sel (.) (d1 - d0) over [count][2][N] packed ciphertexts under ONE TRGSW selector `sel` [2t][2][N] of
        gadget (basebit, t); d0=None is the external product sel (.) d1 (`tfhe_hip_batch_trlwe_cmux`).  numpy in, numpy
        out; or 32-bit CUDA tensors on this engine's GPU in and a tensor out (`out`: where to write, which must overlap
        no input; a new tensor by default), queued on `stream` (torch's current stream by default).
        reference_digits: the reference's truncating decomposition (TFHE_HIP_CMUX_REFERENCE_DIGITS)."""
        flags = CMUX_REFERENCE_DIGITS if reference_digits else 0
        if _is_tensor(d1):
            import torch

            if d1.dim() != 3 or tuple(d1.shape[1:]) != (2, N):
                raise ValueError(f"d1 must be [count][2][{N}]")
            if d0 is not None and tuple(d0.shape) != tuple(d1.shape):
                raise ValueError("d0 must have d1's shape")
            if not _is_tensor(sel) or sel.numel() != max(int(t), 0) * 4 * N:
                raise ValueError(f"sel must be a tensor [2t][2][{N}]")
            if out is None:
                out = torch.empty_like(d1)
            elif tuple(out.shape) != tuple(d1.shape):
                raise ValueError("out must have d1's shape")
            self._call("batch_trlwe_cmux_dev", self._tp(None, sel), int(basebit), int(t), flags,
                       self._tp(None, d0) if d0 is not None else None, self._tp(None, d1), int(d1.shape[0]),
                       self._tp(None, out), self._stream_ptr(None, stream))
            return out
        d1 = _u32(d1).reshape(-1, 2, N)
        sel = _u32(sel).reshape(-1)
        if len(sel) != max(int(t), 0) * 4 * N:
            raise ValueError(f"sel must be [2t][2][{N}]")
        if d0 is not None:
            d0 = _u32(d0).reshape(-1, 2, N)
            if d0.shape != d1.shape:
                raise ValueError("d0 must have d1's shape")
        res = np.empty_like(d1)
        self._call("batch_trlwe_cmux", _ptr(sel), int(basebit), int(t), flags, _ptr(d0), _ptr(d1), len(d1), _ptr(res))
        return res

    def batch_encrypt_trgsw(self, key_lv1, mu, basebit: int, t: int, alpha: float = None, rng_key: bytes = None,
                            first_index: int = 0, return_seed: bool = False):
        """mu [count][N] small integers (or [N]: one) -> count TRGSW selectors [count][2t][2][N] under key_lv1, made on
        the GPU (`tfhe_hip_batch_encrypt_trgsw`); row `row` of selector m takes index first_index + m 2t + row of the
        streams.  rng_key: the 32-byte generator key K, None draws it from getrandom(2); a (K, index) pair must never
        encrypt twice.  alpha: alpha_lv1 of the set by default.  return_seed: also the public mask seed S."""
        self._trgsw_shape(basebit, t)
        k1 = self._key_lv1_arg(key_lv1)
        mu = np.ascontiguousarray(mu, dtype=np.int32).reshape(-1, N)
        out = np.empty((len(mu), 2 * int(t), 2, N), np.uint32)
        seed = (C.c_uint8 * 32)()
        rk, rkp = self._rng_key_arg(rng_key)
        self._call("batch_encrypt_trgsw", _ptr(k1), _ptr(mu), len(mu), int(basebit), int(t),
                   C.c_double(self.params.alpha_lv1 if alpha is None else alpha), rkp, C.c_uint64(int(first_index)),
                   C.addressof(seed), _ptr(out))
        return (out, bytes(seed)) if return_seed else out

    def batch_encrypt_trgsw_dev(self, key_lv1, mu, basebit: int, t: int, out, alpha: float = None, rng_key: bytes = None,
                                first_index: int = 0) -> bytes:
        """Device form: mu [count][N] (int32) and out [count][2t][2][N] (32-bit words) torch tensors on this engine's
        GPU; key_lv1 stays a host array.  Runs on the context's stream and has finished on return.  Returns S."""
        self._trgsw_shape(basebit, t)
        k1 = self._key_lv1_arg(key_lv1)
        if mu.dim() != 2 or mu.shape[1] != N:
            raise ValueError(f"mu must be [count][{N}]")
        if tuple(out.shape) != (mu.shape[0], 2 * int(t), 2, N):
            raise ValueError(f"out must be [{mu.shape[0]}][{2 * int(t)}][2][{N}]")
        seed = (C.c_uint8 * 32)()
        rk, rkp = self._rng_key_arg(rng_key)
        self._call("batch_encrypt_trgsw_dev", _ptr(k1), self._tp(None, mu), int(mu.shape[0]), int(basebit), int(t),
                   C.c_double(self.params.alpha_lv1 if alpha is None else alpha), rkp, C.c_uint64(int(first_index)),
                   C.addressof(seed), self._tp(None, out))
        return bytes(seed)

    def cmux_times(self) -> dict:
        """Kernel times of the packed CMUX's passes since the last call (profiling on)."""
        t = _capi.CmuxTimes()
        self._chk(self._lib.tfhe_hip_get_cmux_times(self._ctx, C.byref(t)))
        return {"digits_ms": t.digits_ms, "contraction_ms": t.contraction_ms, "addend_ms": t.addend_ms, "passes": int(t.passes)}

    # -- encrypted 2-D convolution (include/tfhe_hip.h): int8 filters over a feature map of ciphertexts -------------------
    def _conv2d_shape(self, w_shape, cts_shape, bias_len, stride, padding):
        """(struct tfhe_hip_conv2d_shape, groups, (out_h, out_w)) of filters [out_c][k_h][k_w][in_c] over a map
        [groups][in_h][in_w][in_c][n+1] (or without the leading axis: one group), after the header's shape checks."""
        from .linear import MAX_COLS, _pair, conv2d_out_shape

        w_shape, cts_shape = tuple(int(x) for x in w_shape), tuple(int(x) for x in cts_shape)
        if len(w_shape) != 4 or min(w_shape) < 1 or w_shape[1] * w_shape[2] * w_shape[3] > MAX_COLS:
            raise ValueError(f"w must be [out_c][k_h][k_w][in_c] with 1 <= k_h * k_w * in_c <= {MAX_COLS}")
        out_c, k_h, k_w, in_c = w_shape
        if len(cts_shape) not in (4, 5) or cts_shape[-2:] != (in_c, self.params.n + 1) or min(cts_shape[-4:-2]) < 1:
            raise ValueError(f"cts must be [groups][in_h][in_w][{in_c}][{self.params.n + 1}]")
        if bias_len is not None and bias_len != out_c:
            raise ValueError("bias must be [out_c]")
        in_h, in_w = cts_shape[-4:-2]
        (sh, sw), (ph, pw) = _pair(stride, "stride", 1), _pair(padding, "padding", 0)
        out_hw = conv2d_out_shape(in_h, in_w, k_h, k_w, (sh, sw), (ph, pw))
        shape = _capi.Conv2dShape(in_h, in_w, in_c, out_c, k_h, k_w, sh, sw, ph, pw)
        return shape, (cts_shape[0] if len(cts_shape) == 5 else 1), out_hw

    def batch_tlwe_conv2d(self, w, cts, bias=None, stride=1, padding=0) -> np.ndarray:
        """out[g][oy][ox][oc] = sum_{ky,kx,ic} w[oc][ky][kx][ic] * cts[g][oy*s_h + ky - p_h][ox*s_w + kx - p_w][ic] +
        bias[oc] on the body, zero outside the map (`tfhe_hip_batch_tlwe_conv2d`): w [out_c][k_h][k_w][in_c] int8, cts
        [groups][in_h][in_w][in_c][n+1] (or [in_h][in_w][in_c][n+1]: one group), bias [out_c] torus words or None,
        stride and padding an int or a (vertical, horizontal) pair.  Returns [groups][out_h][out_w][out_c][n+1].
        Needs no key."""
        w = np.asarray(w)
        if w.dtype != np.int8:
            if not np.issubdtype(w.dtype, np.integer) or (w.size and (w.min() < -128 or w.max() > 127)):
                raise ValueError("weights must be integers in [-128, 127]")
        w = np.ascontiguousarray(w, dtype=np.int8)
        bias = None if bias is None else _u32(bias).reshape(-1)
        cts = _u32(cts)
        shape, groups, (out_h, out_w) = self._conv2d_shape(w.shape, cts.shape, None if bias is None else len(bias),
                                                           stride, padding)
        out = np.empty((groups, out_h, out_w, w.shape[0], self.params.n + 1), np.uint32)
        self._call("batch_tlwe_conv2d", C.pointer(shape), _ptr(w), _ptr(bias), _ptr(cts), groups, _ptr(out))
        return out

    def batch_tlwe_conv2d_dev(self, w, cts, out, bias=None, stride=1, padding=0, stream=None) -> None:
        """Device form: w int8 [out_c][k_h][k_w][in_c], cts [groups][in_h][in_w][in_c][n+1], out
        [groups][out_h][out_w][out_c][n+1] and bias [out_c] (or None) CUDA tensors on this engine's GPU (32-bit words
        but for w); out must not overlap cts."""
        if w is None or not w.is_cuda or w.element_size() != 1 or not w.is_contiguous() or w.device.index != self.device:
            raise ValueError(f"w must be a contiguous int8 CUDA tensor [out_c][k_h][k_w][in_c] on cuda:{self.device}")
        if cts is None or len(cts.shape) != 5:
            raise ValueError("cts must be [groups][in_h][in_w][in_c][n+1]")
        shape, groups, (out_h, out_w) = self._conv2d_shape(w.shape, cts.shape, None if bias is None else bias.numel(),
                                                           stride, padding)
        want = (groups, out_h, out_w, int(w.shape[0]), self.params.n + 1)
        if out is None or tuple(out.shape) != want:
            raise ValueError("out must be [%d][%d][%d][%d][%d]" % want)
        self._call("batch_tlwe_conv2d_dev", C.pointer(shape), C.c_void_p(w.data_ptr()), self._tp(None, bias),
                   self._tp(None, cts), groups, self._tp(None, out), self._stream_ptr(None, stream))

    # -- encrypted-table key switch and the tree bootstrap's device form (include/tfhe_hip.h) ----------------------------
    def pack_table(self, stage1, m: int) -> np.ndarray:
        """[m][count][n+1] lv0 ciphertexts, function-major (what batch_lincomb_bootstrap_many returns) ->
        [count][2][N] encrypted test vectors under s1 (`tfhe_hip_batch_pack_table`; packing.table_model)."""
        s1 = _u32(stage1)
        width = self.params.n + 1
        if not isinstance(m, int) or m <= 0 or s1.size % (m * width):
            count = 0 if s1.size == 0 else -1
        else:
            count = s1.size // (m * width)
        if count < 0:
            raise ValueError("stage1 must be [m][count][n+1]")
        out = np.empty((count, 2, N), np.uint32)
        self._chk(self._lib.tfhe_hip_batch_pack_table(self._ctx, _ptr(s1), int(m), count, _ptr(out)))
        return out

    def pack_table_dev(self, stage1, m: int, out, stream=None) -> None:
        """Device form: stage1 [m * count][n+1] (or [m][count][n+1]) and out [count][2][N] 32-bit CUDA tensors."""
        width = self.params.n + 1
        if out is None or out.numel() % (2 * N):
            raise ValueError("out must be [count][2][N]")
        count = out.numel() // (2 * N)
        if stage1 is None or stage1.numel() != max(int(m), 0) * count * width:
            raise ValueError("stage1 must be [m][count][n+1]")
        self._chk(self._lib.tfhe_hip_batch_pack_table_dev(self._ctx, self._tp(None, stage1), int(m), count,
                                                          self._tp(None, out), self._stream_ptr(None, stream)))

    def batch_bootstrap_bivariate_dev(self, x, y, testvecs, m: int, out, n_luts: int = 1, keyswitch: bool = True,
                                      stream=None) -> None:
        """Device form of batch_bootstrap_bivariate: x, y, out [count][n+1] and testvecs [m / n_luts][2][N] 32-bit CUDA
        tensors of this engine's GPU; only enqueues."""
        count = self._dev_batch(None, x, y, out)
        self._chk(self._lib.tfhe_hip_batch_bootstrap_bivariate_dev(
            self._ctx, self._tp(None, x), self._tp(None, y), self._tp(None, testvecs), int(m), int(n_luts), int(keyswitch),
            self._tp(None, out), count, self._stream_ptr(None, stream)))

    def cloud_key_device_tensors(self):
        """(bsk, ksk, testvec, decomposition_offset): the context's key buffers in the engine layouts as uint8 torch
        tensors that ALIAS them (no copy), for device-to-device replication (`distributed.broadcast_engine_key`)."""
        import torch

        ptrs = [C.c_void_p() for _ in range(3)]
        sizes = [C.c_size_t() for _ in range(3)]
        off = C.c_uint32(0)
        self._chk(self._lib.tfhe_hip_cloud_key_buffers(self._ctx, C.byref(ptrs[0]), C.byref(sizes[0]), C.byref(ptrs[1]),
                                                       C.byref(sizes[1]), C.byref(ptrs[2]), C.byref(sizes[2]), C.byref(off)))

        class _Alias:  # CUDA array interface: torch wraps the pointer without copying
            def __init__(self, ptr, nbytes):
                self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}

        dev = torch.device("cuda", self.device)
        ts = [torch.as_tensor(_Alias(int(p.value), int(n.value)), device=dev) for p, n in zip(ptrs, sizes)]
        return ts[0], ts[1], ts[2], int(off.value)

    def adopt_cloud_key(self, decomposition_offset: int) -> None:
        """The key buffers were filled from outside (see cloud_key_device_tensors): make them the current key."""
        self._chk(self._lib.tfhe_hip_adopt_cloud_key(self._ctx, C.c_uint32(int(decomposition_offset))))
        self._key = ("adopted", object())

    def ensure_key(self, cloud_key) -> None:
        if self._key is not cloud_key:
            self.load_cloud_key(cloud_key)

    # -- single stages ----------------------------------------------------------
    def batch_external_product(self, trlwe, bsk_index) -> np.ndarray:
        trlwe = _u32(trlwe).reshape(-1, 2, N)
        idx = np.ascontiguousarray(bsk_index, dtype=np.int32).reshape(-1)
        if len(idx) != len(trlwe):
            raise ValueError("one bootstrapping-key index per TRLWE sample")
        out = np.empty_like(trlwe)
        self._chk(self._lib.tfhe_hip_batch_external_product(self._ctx, _ptr(trlwe), _ptr(idx), _ptr(out), len(trlwe)))
        return out

    def batch_sample_extract(self, trlwe, k: int = 0) -> np.ndarray:
        trlwe = _u32(trlwe).reshape(-1, 2, N)
        out = np.empty((len(trlwe), N + 1), np.uint32)
        self._chk(self._lib.tfhe_hip_batch_sample_extract(self._ctx, _ptr(trlwe), int(k), _ptr(out), len(trlwe)))
        return out

    def batch_identity_key_switch(self, lv1) -> np.ndarray:
        lv1 = _u32(lv1).reshape(-1, N + 1)
        out = np.empty((len(lv1), self.params.n + 1), np.uint32)
        self._chk(self._lib.tfhe_hip_batch_identity_key_switch(self._ctx, _ptr(lv1), _ptr(out), len(lv1)))
        return out

    # -- proxy re-encryption (src/proxy_reenc.rs; rs-tfhe_amd/proxy_reenc.py holds the client side) --------
    def load_reenc_key(self, key_encryptions) -> None:
        """ProxyReencryptionKey::key_encryptions [n][t][base][n+1] (proxy_reenc.rs:224-233) -> this handle (a context
        or a key view holds EITHER a cloud key OR a re-encryption key: `tfhe_hip_load_reenc_key`)."""
        p = self.params
        key = _u32(key_encryptions)
        if key.size != p.n * p.iks_t * p.base * (p.n + 1):
            raise ValueError("re-encryption key has the wrong size for these parameters")
        self._chk(self._lib.tfhe_hip_load_reenc_key(self._ctx, _ptr(key)))

    def reenc_key_is_loaded(self) -> bool:
        return self._lib.tfhe_hip_reenc_key_is_loaded(self._ctx) == 1  # 0 / 1; anything else is not "loaded"

    def batch_reencrypt(self, cts) -> np.ndarray:
        """proxy_reenc::reencrypt_tlwe_lv0 (proxy_reenc.rs:468-510) over [count][n+1] host ciphertexts."""
        cts = _u32(cts).reshape(-1, self.params.n + 1)
        out = np.empty_like(cts)
        self._chk(self._lib.tfhe_hip_batch_reencrypt(self._ctx, _ptr(cts), _ptr(out), len(cts)))
        return out

    def batch_reencrypt_dev(self, a, out, stream=None) -> None:
        """The same on int32 CUDA tensors [count][n+1] of this engine's GPU; only enqueues."""
        count = self._dev_batch(None, a, out)
        self._chk(self._lib.tfhe_hip_batch_reencrypt_dev(self._ctx, self._tp(None, a), self._tp(None, out), count,
                                                         self._stream_ptr(None, stream)))

    # -- public-key encryption and the asymmetric re-encryption key (include/tfhe_hip.h; proxy_reenc.py is the client) --
    def load_public_key(self, encryptions) -> None:
        """PublicKeyLv0::encryptions [size][n+1] (proxy_reenc.rs:95-99), 1 <= size <= 8192, -> this handle, beside
        whatever key it holds (`tfhe_hip_load_public_key`); accepts a proxy_reenc.PublicKeyLv0."""
        enc = _u32(getattr(encryptions, "encryptions", encryptions)).reshape(-1, self.params.n + 1)
        self._chk(self._lib.tfhe_hip_load_public_key(self._ctx, _ptr(enc), len(enc)))

    def public_key_is_loaded(self) -> bool:
        return self._lib.tfhe_hip_public_key_is_loaded(self._ctx) == 1  # 0 / 1; anything else is not "loaded"

    @staticmethod
    def _rng_key_arg(rng_key):
        """(keep-alive, pointer) of a 32-byte generator key; None: the library draws it from getrandom(2)"""
        if rng_key is None:
            return None, None
        if len(rng_key) != 32:
            raise ValueError("rng_key is 32 bytes")
        rk = (C.c_uint8 * 32).from_buffer_copy(bytes(rng_key))
        return rk, C.addressof(rk)

    def batch_pk_encrypt(self, plain, alpha: float, rng_key: bytes = None, first_index: int = 0) -> np.ndarray:
        """plain [count] torus words -> [count][n+1] public-key encryptions, row m at index first_index + m of the
        generator key's streams (`tfhe_hip_batch_pk_encrypt`).  A (rng_key, index) pair must encrypt one message only."""
        plain = _u32(plain).reshape(-1)
        out = np.empty((len(plain), self.params.n + 1), np.uint32)
        rk, rkp = self._rng_key_arg(rng_key)
        self._chk(self._lib.tfhe_hip_batch_pk_encrypt(self._ctx, _ptr(plain), len(plain), C.c_double(alpha), rkp,
                                                      C.c_uint64(int(first_index)), _ptr(out)))
        return out

    def batch_pk_encrypt_dev(self, plain, out, alpha: float, rng_key: bytes = None, first_index: int = 0, stream=None) -> None:
        """Device form: plain [count] and out [count][n+1] torch tensors (32-bit words) on this engine's GPU; only enqueues."""
        if plain.dim() != 1:
            raise ValueError("plain must be [count]")
        count = plain.shape[0]
        if out.dim() != 2 or out.shape[0] != count or out.shape[1] != self.params.n + 1:
            raise ValueError(f"out must be [{count}][{self.params.n + 1}]")
        rk, rkp = self._rng_key_arg(rng_key)
        self._chk(self._lib.tfhe_hip_batch_pk_encrypt_dev(self._ctx, self._tp(None, plain), count, C.c_double(alpha), rkp,
                                                          C.c_uint64(int(first_index)), self._tp(None, out),
                                                          self._stream_ptr(None, stream)))

    def gen_reenc_key_asymmetric(self, key_from, alpha=None, rng_key: bytes = None, download: bool = True):
        """ProxyReencryptionKey::new_asymmetric (proxy_reenc.rs:271-326) towards the public key loaded on this handle,
        generated on the GPU and left loaded here (`tfhe_hip_gen_reenc_key_asymmetric`).  key_from: the delegator's
        key_lv0 [n]; alpha: alpha_lv0 of the set by default.  Returns key_encryptions [n t base][n+1], or None with
        download=False (the key stays on the GPU)."""
        p = self.params
        k0 = _u32(key_from).reshape(-1)
        if len(k0) != p.n:
            raise ValueError("secret key has the wrong size for these parameters")
        key = np.empty((p.n * p.iks_t * p.base, p.n + 1), np.uint32) if download else None
        rk, rkp = self._rng_key_arg(rng_key)
        self._chk(self._lib.tfhe_hip_gen_reenc_key_asymmetric(self._ctx, _ptr(k0), C.c_double(p.alpha_lv0 if alpha is None else alpha),
                                                              rkp, _ptr(key)))
        return key

    # -- symmetric encryption: ciphertexts, the public key, the symmetric re-encryption key (include/tfhe_hip.h) --------
    def _key_lv0_arg(self, key_lv0) -> np.ndarray:
        k0 = _u32(getattr(key_lv0, "key_lv0", key_lv0)).reshape(-1)
        if len(k0) != self.params.n:
            raise ValueError("secret key has the wrong size for these parameters")
        return k0

    def batch_encrypt(self, key_lv0, plain, alpha: float = None, rng_key: bytes = None, mask_seed: bytes = None,
                      first_index: int = 0, full: bool = True, bodies: bool = False):
        """plain [count] torus words -> TLWE lv0 encryptions under key_lv0 [n], row m at index first_index + m of the
        streams (`tfhe_hip_batch_encrypt`): masks under the public mask_seed (None: 32 fresh bytes from the OS), noise
        under rng_key (None: the library draws it from getrandom(2)).  full: return [count][n+1]; bodies: return
        seeded.SeededCiphertexts; both: (full, seeded).  Neither a (rng_key, index) nor a (mask_seed, index) pair may
        encrypt twice."""
        from .seeded import SeededCiphertexts

        if not (full or bodies):
            raise ValueError("nothing to return: full and bodies are both off")
        k0 = self._key_lv0_arg(key_lv0)
        plain = _u32(plain).reshape(-1)
        mask_seed = os.urandom(32) if mask_seed is None else _seed_bytes(mask_seed)
        seed = (C.c_uint8 * 32).from_buffer_copy(mask_seed)
        out = np.empty((len(plain), self.params.n + 1), np.uint32) if full else None
        bod = np.empty(len(plain), np.uint32) if bodies else None
        rk, rkp = self._rng_key_arg(rng_key)
        alpha = self.params.alpha_lv0 if alpha is None else alpha
        self._chk(self._lib.tfhe_hip_batch_encrypt(self._ctx, _ptr(k0), _ptr(plain), len(plain), C.c_double(alpha), rkp,
                                                   C.addressof(seed), C.c_uint64(int(first_index)), _ptr(bod), _ptr(out)))
        sc = SeededCiphertexts(self.params, mask_seed, first_index, bod) if bodies else None
        return (out, sc) if full and bodies else (out if full else sc)

    def batch_encrypt_dev(self, key_lv0, plain, alpha: float, mask_seed: bytes, rng_key: bytes = None, first_index: int = 0,
                          bodies=None, out=None, stream=None) -> None:
        """Device form: plain [count], bodies [count] and out [count][n+1] torch tensors (32-bit words) on this engine's
        GPU, bodies or out may be None; key_lv0 stays a host array.  Enqueues on `stream`."""
        k0 = self._key_lv0_arg(key_lv0)
        if plain.dim() != 1:
            raise ValueError("plain must be [count]")
        count = plain.shape[0]
        if bodies is not None and (bodies.dim() != 1 or bodies.shape[0] != count):
            raise ValueError(f"bodies must be [{count}]")
        if out is not None and (out.dim() != 2 or out.shape[0] != count or out.shape[1] != self.params.n + 1):
            raise ValueError(f"out must be [{count}][{self.params.n + 1}]")
        seed = (C.c_uint8 * 32).from_buffer_copy(_seed_bytes(mask_seed))
        rk, rkp = self._rng_key_arg(rng_key)
        self._chk(self._lib.tfhe_hip_batch_encrypt_dev(
            self._ctx, _ptr(k0), self._tp(None, plain), count, C.c_double(alpha), rkp, C.addressof(seed),
            C.c_uint64(int(first_index)), self._tp(None, bodies) if bodies is not None else None,
            self._tp(None, out) if out is not None else None, self._stream_ptr(None, stream)))

    def gen_public_key(self, key_lv0, size: int = None, alpha: float = None, rng_key: bytes = None, download: bool = True):
        """PublicKeyLv0::new (proxy_reenc.rs:125-153) on the GPU, left loaded on this handle (`tfhe_hip_gen_public_key`):
        `size` (2n by default) encryptions of zero under key_lv0 at alpha (alpha_lv0 by default).  Returns the
        encryptions [size][n+1], or None with download=False."""
        p = self.params
        k0 = self._key_lv0_arg(key_lv0)
        size = 2 * p.n if size is None else int(size)
        enc = np.empty((max(size, 0), p.n + 1), np.uint32) if download else None
        rk, rkp = self._rng_key_arg(rng_key)
        self._chk(self._lib.tfhe_hip_gen_public_key(self._ctx, _ptr(k0), size, C.c_double(p.alpha_lv0 if alpha is None else alpha),
                                                    rkp, _ptr(enc)))
        return enc

    def gen_reenc_key_symmetric(self, key_from, key_to, alpha=None, rng_key: bytes = None, download: bool = True):
        """ProxyReencryptionKey::new_symmetric (proxy_reenc.rs:362-425) on the GPU, left loaded on this handle
        (`tfhe_hip_gen_reenc_key_symmetric`), with basebit and t of this engine's set.  Returns key_encryptions
        [n t base][n+1], or None with download=False (the key stays on the GPU)."""
        p = self.params
        kf, kt = self._key_lv0_arg(key_from), self._key_lv0_arg(key_to)
        key = np.empty((p.n * p.iks_t * p.base, p.n + 1), np.uint32) if download else None
        rk, rkp = self._rng_key_arg(rng_key)
        self._chk(self._lib.tfhe_hip_gen_reenc_key_symmetric(self._ctx, _ptr(kf), _ptr(kt),
                                                             C.c_double(p.alpha_lv0 if alpha is None else alpha), rkp, _ptr(key)))
        return key

    # -- decryption: phases, booleans and messages of LWE rows and packed TRLWE slots (include/tfhe_hip.h) --------
    @staticmethod
    def _decrypt_mode(mode, modulus):
        """(TFHE_HIP_DECRYPT_* code, modulus word) of mode "phase" | "bool" | "message" (or the code itself)"""
        code = _capi.DECRYPT_MODES.get(mode, mode) if isinstance(mode, str) else int(mode)
        if isinstance(code, str):
            raise ValueError('mode is "phase", "bool" or "message"')
        if code == _capi.DECRYPT_MODES["message"] and modulus is None:
            raise ValueError("message mode needs the message modulus")
        return code, C.c_uint32(0 if modulus is None else int(modulus) & 0xFFFFFFFF)

    def _decrypt_key(self, key, width: int = None) -> np.ndarray:
        """The key of an LWE-form call: a SecretKey gives key_lv0, or key_lv1 for rows of N + 1 words"""
        if hasattr(key, "key_lv0"):
            key = key.key_lv1 if width == N + 1 and self.params.n != N else key.key_lv0
        return _u32(key).reshape(-1)

    def batch_decrypt(self, key, cts, mode="phase", modulus: int = None) -> np.ndarray:
        """cts [count][len(key)+1] -> [count] u32 (`tfhe_hip_batch_decrypt`): the phases b - <a, key>, or their decodes
        as booleans (1 / 0) or messages mod `modulus`.  key: key_lv0 [n] for lv0 ciphertexts, key_lv1 [N] for lv1 rows
        (or a SecretKey: picked by the row width)."""
        cts = _u32(cts)
        k = self._decrypt_key(key, cts.shape[-1] if cts.ndim else None)
        cts = cts.reshape(-1, len(k) + 1)
        code, m = self._decrypt_mode(mode, modulus)
        out = np.empty(len(cts), np.uint32)
        self._chk(self._lib.tfhe_hip_batch_decrypt(self._ctx, _ptr(k), len(k), _ptr(cts), len(cts), code, m, _ptr(out)))
        return out

    def batch_decrypt_dev(self, key, cts, out, mode="phase", modulus: int = None, stream=None) -> None:
        """Device form: cts [count][len(key)+1] and out [count] torch tensors (32-bit words) on this engine's GPU; the
        key stays a host array.  Enqueues on `stream`."""
        k = self._decrypt_key(key, cts.shape[-1] if cts.dim() else None)
        if cts.dim() != 2 or cts.shape[1] != len(k) + 1:
            raise ValueError(f"cts must be [count][{len(k) + 1}]")
        if out.dim() != 1 or out.shape[0] != cts.shape[0]:
            raise ValueError(f"out must be [{cts.shape[0]}]")
        code, m = self._decrypt_mode(mode, modulus)
        self._chk(self._lib.tfhe_hip_batch_decrypt_dev(self._ctx, _ptr(k), len(k), self._tp(None, cts), cts.shape[0], code, m,
                                                       self._tp(None, out), self._stream_ptr(None, stream)))

    def batch_decrypt_trlwe(self, key_lv1, packed, count: int, mode="phase", modulus: int = None) -> np.ndarray:
        """The first `count` slots of packed [groups][2][N] under key_lv1 -> [count] u32 (`tfhe_hip_batch_decrypt_trlwe`):
        slot i % N of group i / N, as SecretKey.packed_phase orders them."""
        k = _u32(getattr(key_lv1, "key_lv1", key_lv1)).reshape(-1)
        if len(k) != N:
            raise ValueError("key_lv1 has N = 1024 words")
        packed = _u32(packed).reshape(-1, 2, N)
        code, m = self._decrypt_mode(mode, modulus)
        out = np.empty(max(int(count), 0), np.uint32)
        self._chk(self._lib.tfhe_hip_batch_decrypt_trlwe(self._ctx, _ptr(k), _ptr(packed), len(packed), int(count), code, m,
                                                         _ptr(out)))
        return out

    def batch_decrypt_trlwe_dev(self, key_lv1, packed, count: int, out, mode="phase", modulus: int = None, stream=None) -> None:
        """Device form: packed [groups][2][N] and out [count] torch tensors on this engine's GPU.  Enqueues on `stream`."""
        k = _u32(getattr(key_lv1, "key_lv1", key_lv1)).reshape(-1)
        if len(k) != N:
            raise ValueError("key_lv1 has N = 1024 words")
        if packed.dim() != 3 or packed.shape[1] != 2 or packed.shape[2] != N:
            raise ValueError("packed must be [groups][2][1024]")
        if out.dim() != 1 or out.shape[0] != int(count):
            raise ValueError(f"out must be [{int(count)}]")
        code, m = self._decrypt_mode(mode, modulus)
        self._chk(self._lib.tfhe_hip_batch_decrypt_trlwe_dev(self._ctx, _ptr(k), self._tp(None, packed), packed.shape[0], int(count),
                                                             code, m, self._tp(None, out), self._stream_ptr(None, stream)))

    # -- packed encryption: TRLWE lv1 ciphertexts, N values to a ciphertext (include/tfhe_hip.h) ------------------------
    @staticmethod
    def _key_lv1_arg(key_lv1) -> np.ndarray:
        k = _u32(getattr(key_lv1, "key_lv1", key_lv1)).reshape(-1)
        if len(k) != N:
            raise ValueError("key_lv1 has N = 1024 words")
        return k

    def batch_encrypt_trlwe(self, key_lv1, plain, alpha: float = None, rng_key: bytes = None, mask_seed: bytes = None,
                            first_group: int = 0, full: bool = True, bodies: bool = False):
        """plain [count] torus words -> ceil(count / N) packed TRLWE encryptions under key_lv1 [N], group m at index
        first_group + m of the streams (`tfhe_hip_batch_encrypt_trlwe`): masks under the public mask_seed (None: 32 fresh
        bytes from the OS), noise under rng_key (None: the library draws it from getrandom(2)); the unused slots of the
        last group encrypt 0.  full: return [groups][2][N]; bodies: return seeded.SeededPackedCiphertexts; both: (full,
        seeded).  Neither a (rng_key, group) nor a (mask_seed, group) pair may encrypt twice."""
        from .seeded import SeededPackedCiphertexts

        if not (full or bodies):
            raise ValueError("nothing to return: full and bodies are both off")
        k1 = self._key_lv1_arg(key_lv1)
        plain = _u32(plain).reshape(-1)
        groups = -(-len(plain) // N)
        mask_seed = os.urandom(32) if mask_seed is None else _seed_bytes(mask_seed)
        seed = (C.c_uint8 * 32).from_buffer_copy(mask_seed)
        out = np.empty((groups, 2, N), np.uint32) if full else None
        bod = np.empty((groups, N), np.uint32) if bodies else None
        rk, rkp = self._rng_key_arg(rng_key)
        alpha = self.params.alpha_lv1 if alpha is None else alpha
        self._chk(self._lib.tfhe_hip_batch_encrypt_trlwe(self._ctx, _ptr(k1), _ptr(plain), len(plain), C.c_double(alpha), rkp,
                                                         C.addressof(seed), C.c_uint64(int(first_group)), _ptr(bod), _ptr(out)))
        sc = SeededPackedCiphertexts(self.params, mask_seed, first_group, bod, len(plain)) if bodies else None
        return (out, sc) if full and bodies else (out if full else sc)

    def batch_encrypt_trlwe_dev(self, key_lv1, plain, alpha: float, mask_seed: bytes, rng_key: bytes = None,
                                first_group: int = 0, bodies=None, out=None, stream=None) -> None:
        """Device form: plain [count], bodies [groups][N] and out [groups][2][N] torch tensors (32-bit words) on this
        engine's GPU, bodies or out may be None; key_lv1 stays a host array.  Enqueues on `stream`."""
        k1 = self._key_lv1_arg(key_lv1)
        if plain.dim() != 1:
            raise ValueError("plain must be [count]")
        count = plain.shape[0]
        groups = -(-count // N)
        if bodies is not None and (bodies.dim() != 2 or bodies.shape[0] != groups or bodies.shape[1] != N):
            raise ValueError(f"bodies must be [{groups}][{N}]")
        if out is not None and (out.dim() != 3 or out.shape[0] != groups or out.shape[1] != 2 or out.shape[2] != N):
            raise ValueError(f"out must be [{groups}][2][{N}]")
        seed = (C.c_uint8 * 32).from_buffer_copy(_seed_bytes(mask_seed))
        rk, rkp = self._rng_key_arg(rng_key)
        self._chk(self._lib.tfhe_hip_batch_encrypt_trlwe_dev(
            self._ctx, _ptr(k1), self._tp(None, plain), count, C.c_double(alpha), rkp, C.addressof(seed),
            C.c_uint64(int(first_group)), self._tp(None, bodies) if bodies is not None else None,
            self._tp(None, out) if out is not None else None, self._stream_ptr(None, stream)))

    def expand_seeded_trlwe(self, seeded) -> np.ndarray:
        """seeded.SeededPackedCiphertexts -> [groups][2][N] u32, expanded on the GPU (`tfhe_hip_expand_seeded_trlwe`)."""
        bodies = _u32(seeded.bodies).reshape(-1, N)
        out = np.empty((len(bodies), 2, N), np.uint32)
        seed = (C.c_uint8 * 32).from_buffer_copy(_seed_bytes(seeded.mask_seed))
        self._chk(self._lib.tfhe_hip_expand_seeded_trlwe(self._ctx, C.addressof(seed), C.c_uint64(int(seeded.first_group)),
                                                         _ptr(bodies), len(bodies), _ptr(out)))
        return out

    def expand_seeded_trlwe_dev(self, mask_seed: bytes, first_group: int, bodies, out, stream=None) -> None:
        """Device form: bodies [groups][N] and out [groups][2][N] torch tensors (32-bit words) on this engine's GPU."""
        if bodies.dim() != 2 or bodies.shape[1] != N:
            raise ValueError(f"bodies must be [groups][{N}]")
        groups = bodies.shape[0]
        if out.dim() != 3 or out.shape[0] != groups or out.shape[1] != 2 or out.shape[2] != N:
            raise ValueError(f"out must be [{groups}][2][{N}]")
        seed = (C.c_uint8 * 32).from_buffer_copy(_seed_bytes(mask_seed))
        self._chk(self._lib.tfhe_hip_expand_seeded_trlwe_dev(self._ctx, C.addressof(seed), C.c_uint64(int(first_group)),
                                                             self._tp(None, bodies), groups, self._tp(None, out),
                                                             self._stream_ptr(None, stream)))

    def pk_encrypt_times(self) -> dict:
        """Kernel times of the public-key encryption / asymmetric key passes since the last call (profiling on)."""
        t = _capi.PkEncryptTimes()
        self._chk(self._lib.tfhe_hip_get_pk_encrypt_times(self._ctx, C.byref(t)))
        return {"selectors_ms": t.selectors_ms, "contraction_ms": t.contraction_ms, "passes": int(t.passes)}

    def batch_ifft(self, polys) -> np.ndarray:
        polys = _u32(polys).reshape(-1, N)
        out = np.empty((len(polys), N), np.float64)
        self._chk(self._lib.tfhe_hip_batch_ifft(self._ctx, _ptr(out), _ptr(polys), len(polys)))
        return out

    def batch_fft(self, spectra) -> np.ndarray:
        spectra = np.ascontiguousarray(spectra, dtype=np.float64).reshape(-1, N)
        out = np.empty((len(spectra), N), np.uint32)
        self._chk(self._lib.tfhe_hip_batch_fft(self._ctx, _ptr(out), _ptr(spectra), len(spectra)))
        return out

    def batch_poly_mul(self, a, b) -> np.ndarray:
        a, b = _u32(a).reshape(-1, N), _u32(b).reshape(-1, N)
        if b.shape != a.shape:
            raise ValueError("operand batches differ in shape")
        out = np.empty_like(a)
        self._chk(self._lib.tfhe_hip_batch_poly_mul(self._ctx, _ptr(out), _ptr(a), _ptr(b), len(a)))
        return out

    # -- measurement ------------------------------------------------------------
    def set_profiling(self, enabled: bool) -> None:
        self._chk(self._lib.tfhe_hip_set_profiling(self._ctx, int(enabled)))

    def kernel_times(self) -> dict:
        kt = _capi.KernelTimes()
        self._chk(self._lib.tfhe_hip_get_kernel_times(self._ctx, C.byref(kt)))
        return {
            "blind_rotate_ms": kt.blind_rotate_ms,
            "key_switch_ms": kt.key_switch_ms,
            "blind_rotate_launches": int(kt.blind_rotate_launches),
            "key_switch_launches": int(kt.key_switch_launches),
            "bootstraps": int(kt.bootstraps),
        }

    def clock_sample(self) -> dict:
        """Shader clock the blind-rotation kernel actually ran at (sampled while profiling is on)."""
        cs = _capi.ClockSample()
        self._chk(self._lib.tfhe_hip_get_clock_sample(self._ctx, C.byref(cs)))
        return {"shader_mhz": cs.shader_mhz, "rtc_mhz": cs.rtc_mhz, "shader_cycles": int(cs.shader_cycles),
                "rtc_ticks": int(cs.rtc_ticks)}

    def key_switch_clock_sample(self) -> dict:
        """The same sample for the matrix-core key switch (k_key_switch_mfma)."""
        cs = _capi.ClockSample()
        self._chk(self._lib.tfhe_hip_get_key_switch_clock_sample(self._ctx, C.byref(cs)))
        return {"shader_mhz": cs.shader_mhz, "rtc_mhz": cs.rtc_mhz, "shader_cycles": int(cs.shader_cycles),
                "rtc_ticks": int(cs.rtc_ticks)}

    def synchronize(self) -> None:
        self._chk(self._lib.tfhe_hip_synchronize(self._ctx))

    # -- concurrent callers -------------------------------------------------------
    def set_combining(self, max_count: int) -> None:
        """Host-pointer calls of at most `max_count` ciphertexts made by concurrent threads share launches
        (`tfhe_hip_set_combining`; the default is the device's CU count, 0 switches it off)."""
        self._chk(self._lib.tfhe_hip_set_combining(self._ctx, int(max_count)))

    def combine_stats(self) -> dict:
        """Counters of the combining front end since the last call (`tfhe_hip_get_combine_stats`)."""
        st = _capi.CombineStats()
        self._chk(self._lib.tfhe_hip_get_combine_stats(self._ctx, C.byref(st)))
        return {k: (float(getattr(st, k)) if k.endswith("_us") else int(getattr(st, k))) for k, _ in st._fields_}

    @property
    def rounding_mode(self) -> str:
        """"fast" / "general": the blind-rotation kernels' rounding of the external product (`tfhe_hip_rounding_mode`)."""
        return self._lib.tfhe_hip_rounding_mode(self._ctx).decode()

    def describe_dispatch(self, count: int) -> str:
        """Which kernels a batch of `count` runs on (`tfhe_hip_describe_dispatch`), e.g.
        "blind_rotate=batch[0,1024)+single[1024,1100) key_switch=mfma(k=4)".  Needs the key loaded."""
        buf = C.create_string_buffer(256)
        self._chk(self._lib.tfhe_hip_describe_dispatch(self._ctx, int(count), buf, len(buf)))
        return buf.value.decode()


class Pool(_Handle):
    """Several GPUs behind one handle (`tfhe_hip_pool`): the reference's Rayon `par_map` over the ciphertexts of
    a batch (src/parallel/rayon_impl.rs:40-47) as a map over devices.  `devices` may repeat an index (two
    contexts on one GPU).  The cloud key goes to the first device once and is replicated device to device;
    every batch call splits its host arrays contiguously over the members and keeps input order."""

    def __init__(self, params: SecurityParams, devices, _view_of: "Pool" = None):
        self.params = params
        self.devices = [int(d) for d in devices]
        self._lib = _capi.lib()
        h = C.c_void_p()
        if _view_of is not None:  # a key view of a pool: one key view per member context
            rc = self._lib.tfhe_hip_pool_key_create(_view_of._h, C.byref(h))
            if rc != _capi.OK:
                raise _capi.TfheHipError(rc, "tfhe_hip_pool_key_create failed")
        else:
            cp = _capi.Params(params.n, params.l, params.bgbit, params.basebit, params.iks_t)
            arr = (C.c_int * len(self.devices))(*self.devices)
            rc = self._lib.tfhe_hip_pool_create(C.byref(cp), arr, len(self.devices), C.byref(h))
            if rc != _capi.OK:
                msg = self._lib.tfhe_hip_pool_last_error(None)
                raise _capi.TfheHipError(rc, msg.decode() if msg else "")
        self._h = h
        self.home = 0  # member whose GPU holds the operands of the *_dev calls (their `home` argument's default)
        self._link(_view_of)

    def new_key_view(self) -> "Pool":
        """Another resident cloud key on every member of this pool (`tfhe_hip_pool_key_create`)."""
        base = self._parent if self._parent is not None else self
        return Pool(base.params, base.devices, _view_of=base)

    # -- what a pool supplies to the shared calls ------------------------------------------------------------------------
    def _destroy(self) -> None:
        if getattr(self, "_h", None):
            self._lib.tfhe_hip_pool_destroy(self._h)
        self._h = None

    def _chk(self, rc: int) -> None:
        if rc != _capi.OK:
            msg = self._lib.tfhe_hip_pool_last_error(self._h)
            raise _capi.TfheHipError(rc, msg.decode() if msg else "")

    def _call(self, name: str, *args) -> None:
        self._chk(getattr(self._lib, "tfhe_hip_pool_" + name)(self._h, *args))

    def _call_dev(self, name: str, home, *args) -> None:
        self._call(name, home, *args)

    def _device(self, home) -> int:
        if not 0 <= home < len(self.devices):
            raise ValueError("no such pool member")
        return self.devices[home]

    def _member_ctx(self, member: int):
        return C.c_void_p(self._lib.tfhe_hip_pool_ctx(self._h, int(member)))

    @property
    def device(self) -> int:
        return self.devices[self.home]

    def __len__(self) -> int:
        return int(self._lib.tfhe_hip_pool_size(self._h))

    def set_combining(self, max_count: int) -> None:
        """`Engine.set_combining` on every member (small concurrent calls go to the least loaded member's front end)."""
        for i in range(len(self)):
            Engine.from_pool(self, i).set_combining(max_count)

    def combine_stats(self) -> list:
        """`Engine.combine_stats` of every member."""
        return [Engine.from_pool(self, i).combine_stats() for i in range(len(self))]

    @property
    def key_transport(self) -> str:
        """"rccl" / "peer-copy": how the last cloud key reached the members (`tfhe_hip_pool_key_transport`)."""
        return self._lib.tfhe_hip_pool_key_transport(self._h).decode()

    def members_for(self, count: int) -> int:
        """Members a batch of `count` is spread over (`tfhe_hip_pool_members_for`): small batches use fewer."""
        return int(self._lib.tfhe_hip_pool_members_for(self._h, count))

    def shard(self, count: int, member: int) -> tuple:
        """[lo, hi) of the batch that `member` runs -- over the members the call actually uses (members_for),
        so (0, 0) for a member a small batch leaves idle."""
        lo, hi = C.c_size_t(0), C.c_size_t(0)
        self._lib.tfhe_hip_pool_shard(count, member, self.members_for(count), C.byref(lo), C.byref(hi))
        return int(lo.value), int(hi.value)

    def export_cloud_key(self, member: int = 0):
        """The key of pool member `member` back as a CloudKey in the reference layouts."""
        return self._export_cloud_key(member)

    def synchronize(self) -> None:
        """Drain every member's own stream (`tfhe_hip_pool_synchronize`); the home stream is the caller's."""
        self._chk(self._lib.tfhe_hip_pool_synchronize(self._h))

    @property
    def data_transport(self) -> str:
        """"rccl" / "peer-copy" / "none": how the last *_dev call moved its shards."""
        return self._lib.tfhe_hip_pool_data_transport(self._h).decode()

    def set_profiling(self, enabled: bool) -> None:
        self._chk(self._lib.tfhe_hip_pool_set_profiling(self._h, int(enabled)))

    def transfer_times(self) -> dict:
        tt = _capi.PoolTransferTimes()
        self._chk(self._lib.tfhe_hip_pool_get_transfer_times(self._h, C.byref(tt)))
        return {k: getattr(tt, k) for k, _ in _capi.PoolTransferTimes._fields_}
