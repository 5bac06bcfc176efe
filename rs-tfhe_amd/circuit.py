"""Levelised circuits with device-resident ciphertexts.

The reference's real workloads are gate DAGs evaluated one gate at a time on the CPU
(examples/add_two_numbers.rs:11-50: full_adder / add; examples/lut_add_two_numbers.rs:82-158: the LUT nibble adder).
Here a circuit is built once as a DAG over wires -- gates, muxes, programmable bootstraps and linear nodes -- and run
by the native scheduler behind the C ABI (`tfhe_hip_circuit_*`, include/tfhe_hip.h): levelised, every level one
launch per kind whatever its size times the whole batch, operands read out of one device-resident wire store by row
index inside the blind rotation, results written contiguously.  No torch operation sits between levels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _capi
from . import engine as E


@dataclass
class _Gate:
    op: int
    a: int
    b: int
    out: int
    level: int


@dataclass
class Circuit:
    n_inputs: int
    gates: list = field(default_factory=list)
    _level: dict = field(default_factory=dict)
    _n_wires: int = 0
    _plans: dict = field(default_factory=dict)  # (device, n_gates) -> per-level index / gate-code tensors (_run_dev_torch)
    _nodes: list = field(default_factory=list)  # one entry per non-input wire, in wire order
    _luts: list = field(default_factory=list)   # [2][N] uint32 test vectors (lut ids)
    _native: object = field(default=None, repr=False)  # the compiled tfhe_hip_circuit of the nodes so far

    def __post_init__(self):
        self._n_wires = self.n_inputs
        for w in range(self.n_inputs):
            self._level[w] = 0

    def __del__(self):
        try:
            self._drop_native()
        except Exception:
            pass

    # -- construction ----------------------------------------------------------------
    def _wire(self, w) -> int:
        w = int(w)
        if not 0 <= w < self._n_wires:
            raise ValueError(f"no wire {w}")
        return w

    def _add(self, node, level) -> int:
        out = self._n_wires
        self._n_wires += 1
        self._level[out] = level
        self._nodes.append(node)
        self._drop_native()
        return out

    def gate(self, op: int, a: int, b: int) -> int:
        """A bootstrapped two-input gate (one of tfhe_hip_gate); returns its output wire."""
        a, b = self._wire(a), self._wire(b)
        if not 0 <= op <= E.COPY:
            raise ValueError(f"unknown gate code {op}")
        lvl = 1 + max(self._level[a], self._level[b] if op != E.COPY else 0)
        out = self._add(("gate", int(op), a, b), lvl)
        self.gates.append(_Gate(int(op), a, b, out, lvl))
        return out

    def nand(self, a, b): return self.gate(E.NAND, a, b)
    def and_(self, a, b): return self.gate(E.AND, a, b)
    def or_(self, a, b): return self.gate(E.OR, a, b)
    def xor(self, a, b): return self.gate(E.XOR, a, b)
    def xnor(self, a, b): return self.gate(E.XNOR, a, b)
    def nor(self, a, b): return self.gate(E.NOR, a, b)
    def and_ny(self, a, b): return self.gate(E.ANDNY, a, b)
    def and_yn(self, a, b): return self.gate(E.ANDYN, a, b)
    def or_ny(self, a, b): return self.gate(E.ORNY, a, b)
    def or_yn(self, a, b): return self.gate(E.ORYN, a, b)

    def mux_naive(self, a, b, c):
        """Gates::mux_naive (src/gates.rs:189-199): or(and(a, b), and(not(a), c))."""
        return self.or_(self.and_(a, b), self.and_ny(a, c))

    def mux(self, a, b, c):
        """Gates::mux (src/gates.rs:157-183, the reference formula): a ? b : c in one level."""
        a, b, c = self._wire(a), self._wire(b), self._wire(c)
        return self._add(("mux", a, b, c), 1 + max(self._level[a], self._level[b], self._level[c]))

    def lut(self, testvec) -> int:
        """Register a test vector ([2][N] u32, e.g. lut.Generator(...).generate_lookup_table(f).poly); returns its id."""
        tv = np.ascontiguousarray(testvec, dtype=np.uint32).reshape(-1)
        if tv.size != 2 * E.N:
            raise ValueError(f"a test vector is [2][{E.N}]")
        self._luts.append(tv)
        self._drop_native()
        return len(self._luts) - 1

    def pbs(self, ca: int, a: int, cb: int, b, cconst: int, lut: int) -> int:
        """Programmable bootstrap (src/bootstrap/lut.rs:79-99) of ca*a + cb*b (body + cconst) through test vector
        `lut`, key-switched; b is ignored when cb == 0."""
        a = self._wire(a)
        cb &= 0xFFFFFFFF
        b = self._wire(b) if cb else a
        if not 0 <= lut < len(self._luts):
            raise ValueError(f"no lut {lut}")
        lvl = 1 + max(self._level[a], self._level[b] if cb else 0)
        return self._add(("pbs", ca & 0xFFFFFFFF, a, cb, b, cconst & 0xFFFFFFFF, int(lut)), lvl)

    def pbs_many(self, ca: int, a: int, cb: int, b, cconst: int, lut: int, n_luts: int) -> list:
        """Many-LUT bootstrap (tfhe_hip_circuit_add_pbs_many): the n_luts functions packed in `lut`
        (Generator.generate_many_lookup_table) of ca*a + cb*b + cconst from ONE blind rotation; returns the n_luts
        consecutive output wires, function j at [j]."""
        a = self._wire(a)
        cb &= 0xFFFFFFFF
        b = self._wire(b) if cb else a
        if not 0 <= lut < len(self._luts):
            raise ValueError(f"no lut {lut}")
        if n_luts not in (1, 2, 4, 8):
            raise ValueError("n_luts must be 1, 2, 4 or 8")
        lvl = 1 + max(self._level[a], self._level[b] if cb else 0)
        head = self._add(("pbs_many", ca & 0xFFFFFFFF, a, cb, b, cconst & 0xFFFFFFFF, int(lut), int(n_luts)), lvl)
        return [head] + [self._add(("pbs_fn", head, j), lvl) for j in range(1, n_luts)]

    def lincomb(self, terms, cconst: int = 0) -> int:
        """sum coef * wire (+ cconst on the body): TLWE `+` / `-` / scaling, no bootstrap.  terms: [(coef, wire)]."""
        terms = [(int(c) & 0xFFFFFFFF, self._wire(w)) for c, w in terms]
        lvl = max((self._level[w] for _, w in terms), default=0)
        return self._add(("lin", tuple(terms), cconst & 0xFFFFFFFF), lvl)

    def not_(self, a) -> int:
        """Gates::not (src/gates.rs:202-204): -a, no bootstrap."""
        return self.lincomb([(0xFFFFFFFF, a)])

    def constant(self, value: bool) -> int:
        """Gates::constant (src/gates.rs:212-219): body 1/8, or 1 - 1/8 wrapped for false (quirk Q6)."""
        return self.lincomb([], 0x20000000 if value else 0xE0000001)

    def full_adder(self, a, b, c):
        """examples/add_two_numbers.rs:11-29 -> (sum, carry)."""
        a_xor_b = self.xor(a, b)
        a_and_b = self.and_(a, b)
        a_xor_b_and_c = self.and_(a_xor_b, c)
        s = self.xor(a_xor_b, c)
        carry = self.or_(a_and_b, a_xor_b_and_c)
        return s, carry

    def add(self, a_bits, b_bits, cin):
        """examples/add_two_numbers.rs:31-50 -> (sum bits, carry out)."""
        assert len(a_bits) == len(b_bits), "Cannot add two numbers with different number of bits!"
        result, carry = [], cin
        for x, y in zip(a_bits, b_bits):
            s, carry = self.full_adder(x, y, carry)
            result.append(s)
        return result, carry

    # -- schedule ----------------------------------------------------------------------
    @property
    def n_wires(self) -> int:
        return self._n_wires

    def levels(self):
        """Gates grouped by level (all operands of level L come from levels < L)."""
        depth = max((g.level for g in self.gates), default=0)
        out = [[] for _ in range(depth)]
        for g in self.gates:
            out[g.level - 1].append(g)
        return out

    # -- the native circuit ----------------------------------------------------------------
    def _drop_native(self):
        if self._native is not None:
            _capi.lib().tfhe_hip_circuit_destroy(self._native)
            self._native = None

    def _native_handle(self):
        """The nodes so far as a compiled tfhe_hip_circuit (built on first use, rebuilt after further additions)."""
        if self._native is not None:
            return self._native
        lib = _capi.lib()
        h = C.c_void_p()
        _chk_circ(lib.tfhe_hip_circuit_create(self.n_inputs, C.byref(h)), "create")
        try:
            w, lid = C.c_uint32(), C.c_uint32()
            for tv in self._luts:
                _chk_circ(lib.tfhe_hip_circuit_add_lut(h, tv.ctypes.data_as(C.c_void_p), C.byref(lid)), "add_lut")
            for node in self._nodes:
                kind = node[0]
                if kind == "gate":
                    rc = lib.tfhe_hip_circuit_add_gate(h, node[1], node[2], node[3], C.byref(w))
                elif kind == "mux":
                    rc = lib.tfhe_hip_circuit_add_mux(h, node[1], node[2], node[3], C.byref(w))
                elif kind == "pbs":
                    rc = lib.tfhe_hip_circuit_add_pbs(h, *node[1:], C.byref(w))
                elif kind == "pbs_many":
                    ws = (C.c_uint32 * node[7])()
                    rc = lib.tfhe_hip_circuit_add_pbs_many(h, *node[1:], ws)
                elif kind == "pbs_fn":  # added with its head
                    continue
                else:
                    coefs = np.array([c for c, _ in node[1]], np.uint32)
                    wires = np.array([x for _, x in node[1]], np.uint32)
                    rc = lib.tfhe_hip_circuit_add_lincomb(h, coefs.ctypes.data_as(C.c_void_p), wires.ctypes.data_as(C.c_void_p),
                                                          len(node[1]), node[2], C.byref(w))
                _chk_circ(rc, f"add_{kind}")
            _chk_circ(lib.tfhe_hip_circuit_compile(h), "compile")
        except Exception:
            lib.tfhe_hip_circuit_destroy(h)
            raise
        self._native = h
        self._all_wires = np.arange(self._n_wires, dtype=np.uint32)
        return h

    def describe(self) -> list:
        """The native schedule, one dict per level (level 0 = the inputs): slot range and (launches, nodes) per kind."""
        lib, h = _capi.lib(), self._native_handle()
        n = C.c_size_t()
        _chk_circ(lib.tfhe_hip_circuit_describe(h, None, 0, C.byref(n)), "describe")
        buf = np.zeros((n.value, _capi.CIRCUIT_LEVEL_WORDS), np.uint32)
        _chk_circ(lib.tfhe_hip_circuit_describe(h, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n)), "describe")
        keys = ("begin", "end", "lincomb_launches", "lincomb_nodes", "nks_launches", "nks_nodes", "gate_launches",
                "gate_nodes", "lut_launches", "lut_nodes")
        return [dict(zip(keys, (int(x) for x in row))) for row in buf]

    @property
    def slots(self) -> int:
        v = C.c_uint32()
        _chk_circ(_capi.lib().tfhe_hip_circuit_slots(self._native_handle(), C.byref(v)), "slots")
        return v.value

    def wire_slot(self, wire: int) -> int:
        """The store slot of `wire` (_capi.NO_SLOT for a linear node, formed where it is read)."""
        v = C.c_uint32()
        _chk_circ(_capi.lib().tfhe_hip_circuit_wire_slot(self._native_handle(), int(wire), C.byref(v)), "wire_slot")
        return v.value

    def operand_slots(self, wire: int) -> list:
        """The store slots the launch of bootstrap node `wire` reads."""
        buf, n = np.zeros(3, np.uint32), C.c_uint32()
        _chk_circ(_capi.lib().tfhe_hip_circuit_operand_slots(self._native_handle(), int(wire), buf.ctypes.data_as(C.c_void_p),
                                                             C.byref(n)), "operand_slots")
        return [int(x) for x in buf[: n.value]]

    # -- execution -----------------------------------------------------------------------
    def run_dev(self, eng, inputs, stream=None):
        """inputs: int32 CUDA tensor [n_inputs][B][n+1]; returns every wire [n_wires][B][n+1] (int32 CUDA tensor) in
        this circuit's wire numbering.  The native scheduler runs the whole circuit (`tfhe_hip_circuit_run_dev`) in a
        store of its own slots, then `tfhe_hip_circuit_gather_dev` hands the wires back.
        `eng`: an Engine, or a Pool -- then the store lives on the pool's home member (`pool.home`) and every level's
        launches are pool calls cut over the members (`tfhe_hip_circuit_run_pool_dev`)."""
        import torch

        n_in, B, w = inputs.shape
        assert n_in == self.n_inputs
        inputs = inputs.contiguous()
        # allocations and kernels on ONE stream (the caching allocator hands a block back to that stream's later work)
        with _on_stream(stream):
            store = torch.empty((self.slots, B, w), dtype=torch.int32, device=inputs.device)
            out = torch.empty((self.n_wires, B, w), dtype=torch.int32, device=inputs.device)
            self.run_store_dev(eng, inputs, store, stream)
            self.gather_dev(eng, store, out, stream=stream)
        return out

    def _dev_entry(self, eng, name: str):
        """(C function, leading arguments) of a circuit `_dev` call on an Engine or a Pool"""
        lib = _capi.lib()
        if isinstance(eng, E.Pool):
            return getattr(lib, f"tfhe_hip_circuit_{name}_pool_dev"), (eng._h, eng.home)
        return getattr(lib, f"tfhe_hip_circuit_{name}_dev"), (eng._ctx,)

    def run_store_dev(self, eng, inputs, store, stream=None) -> None:
        """`tfhe_hip_circuit_run_dev` alone: inputs [n_inputs][B][n+1] into the caller's store [slots][B][n+1] (32-bit
        CUDA tensors on the call's GPU), every level enqueued on `stream`.  Slot s of the store holds the wire with
        wire_slot(w) == s; materialised linear nodes and the mux's first level take the remaining slots."""
        B = inputs.shape[1]
        if tuple(inputs.shape) != (self.n_inputs, B, eng.params.n + 1) or tuple(store.shape) != (self.slots, B, eng.params.n + 1):
            raise ValueError("inputs must be [n_inputs][B][n+1] and store [slots][B][n+1]")
        fn, lead = self._dev_entry(eng, "run")
        home = eng.home
        eng._chk(fn(*lead, self._native_handle(), eng._tp(home, inputs), eng._tp(home, store), B, eng._stream_ptr(home, stream)))

    def gather_dev(self, eng, store, out, wires=None, stream=None) -> None:
        """`tfhe_hip_circuit_gather_dev` alone: the wires `wires` (every wire by default) of a store [slots][B][n+1]
        that run_store_dev filled, into out [len(wires)][B][n+1]; linear nodes are formed from the store here."""
        h = self._native_handle()
        ow = self._all_wires if wires is None else np.ascontiguousarray(wires, dtype=np.uint32).reshape(-1)
        B = store.shape[1]
        if tuple(store.shape) != (self.slots, B, eng.params.n + 1) or tuple(out.shape) != (len(ow), B, eng.params.n + 1):
            raise ValueError("store must be [slots][B][n+1] and out [len(wires)][B][n+1]")
        fn, lead = self._dev_entry(eng, "gather")
        home = eng.home
        eng._chk(fn(*lead, h, eng._tp(home, store), B, ow.ctypes.data_as(C.c_void_p), len(ow), eng._tp(home, out),
                    eng._stream_ptr(home, stream)))

    def _run_dev_torch(self, eng, inputs, stream=None):
        """The torch-scheduled path this module had before the native scheduler (gate-only circuits): per level two
        index_select gathers, one batch_gates_mixed_dev launch and one index_copy_.  Kept for comparisons only."""
        import torch

        if len(self.gates) != len(self._nodes):
            raise ValueError("_run_dev_torch runs gate-only circuits")
        n_in, B, w = inputs.shape
        assert n_in == self.n_inputs
        with _on_stream(stream):
            wires = torch.empty((self.n_wires, B, w), dtype=torch.int32, device=inputs.device)
            wires[:n_in] = inputs
            for ia, ib, io, codes in self._plan(inputs.device):
                a = wires.index_select(0, ia).reshape(-1, w)
                b = wires.index_select(0, ib).reshape(-1, w)
                gc = codes.repeat_interleave(B).contiguous()
                out = torch.empty_like(a)
                eng.batch_gates_mixed_dev(gc, a, b, out)  # torch's current stream = `stream`
                wires.index_copy_(0, io, out.reshape(len(io), B, w))
        return wires

    def _plan(self, device):
        """Per-level operand / result wire indices and gate codes as device tensors (_run_dev_torch)."""
        import torch

        key = (str(device), len(self.gates))
        plan = self._plans.get(key)
        if plan is None:
            plan = []
            for lvl in self.levels():
                plan.append((torch.tensor([g.a for g in lvl], device=device),
                             torch.tensor([g.b for g in lvl], device=device),
                             torch.tensor([g.out for g in lvl], device=device),
                             torch.tensor([g.op for g in lvl], dtype=torch.uint8, device=device)))
            self._plans[key] = plan
        return plan

    def run(self, eng, inputs) -> np.ndarray:
        """Host convenience: inputs uint32 [n_inputs][B][n+1] -> all wires uint32 [n_wires][B][n+1].  `eng`: Engine or
        Pool (`tfhe_hip_circuit_run` / `tfhe_hip_circuit_run_pool`: the store on the device, one copy in, one out)."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint32)
        n_in, B, w = inputs.shape
        assert n_in == self.n_inputs
        h = self._native_handle()
        lib = _capi.lib()
        out = np.empty((self.n_wires, B, w), np.uint32)
        args = (h, inputs.ctypes.data_as(C.c_void_p), B, self._all_wires.ctypes.data_as(C.c_void_p), self.n_wires,
                out.ctypes.data_as(C.c_void_p))
        if isinstance(eng, E.Pool):
            eng._chk(lib.tfhe_hip_circuit_run_pool(eng._h, *args))
        else:
            eng._chk(lib.tfhe_hip_circuit_run(eng._ctx, *args))
        return out

    def run_reference(self, gate_fn, inputs, mux_fn=None, pbs_fn=None, many_fn=None) -> np.ndarray:
        """Evaluate node by node in the order they were added (the order the reference's examples execute them; the
        tests plug their CPU checker in here): `gate_fn(op, a[B][n+1], b[B][n+1]) -> [B][n+1]`,
        `mux_fn(a, b, c) -> [B][n+1]`, `pbs_fn(testvec [2][N], prepared [B][n+1]) -> [B][n+1]`,
        `many_fn(testvec, prepared, k) -> [k][B][n+1]`; linear nodes in numpy (wrapping u32)."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint32)
        wires = np.zeros((self.n_wires,) + inputs.shape[1:], np.uint32)
        wires[: self.n_inputs] = inputs
        for i, node in enumerate(self._nodes):
            out, kind = self.n_inputs + i, node[0]
            if kind == "gate":
                wires[out] = gate_fn(node[1], wires[node[2]], wires[node[3]])
            elif kind == "mux":
                wires[out] = mux_fn(wires[node[1]], wires[node[2]], wires[node[3]])
            elif kind == "pbs":
                _, ca, a, cb, b, cc, lut = node
                prep = _lin([(ca, wires[a])] + ([(cb, wires[b])] if cb else []), cc, wires.shape[1:])
                wires[out] = pbs_fn(self._luts[lut].reshape(2, -1), prep)
            elif kind == "pbs_many":
                _, ca, a, cb, b, cc, lut, k = node
                prep = _lin([(ca, wires[a])] + ([(cb, wires[b])] if cb else []), cc, wires.shape[1:])
                wires[out:out + k] = many_fn(self._luts[lut].reshape(2, -1), prep, k)
            elif kind == "pbs_fn":
                pass  # written with its head
            else:
                wires[out] = _lin([(c, wires[w]) for c, w in node[1]], node[2], wires.shape[1:])
        return wires


def _lin(terms, cconst, shape) -> np.ndarray:
    """sum coef * x (+ cconst on the body), wrapping u32."""
    acc = np.zeros(shape, np.uint32)
    for c, x in terms:
        acc += np.uint32(c) * x
    acc[..., -1] += np.uint32(cconst)
    return acc


def _chk_circ(rc: int, what: str) -> None:
    if rc != _capi.OK:
        raise _capi.TfheHipError(rc, f"tfhe_hip_circuit_{what}")


def _on_stream(stream):
    """torch.cuda.stream(stream) when a stream is given, a no-op context otherwise."""
    import contextlib

    import torch

    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


# ---- LUT arithmetic: the nibble adder of examples/lut_add_two_numbers.rs, batched ---------------
def lut_add_u8_dev(eng, a_low, a_high, b_low, b_high, stream=None):
    """8-bit addition with three programmable bootstraps per byte pair instead of eight gate
    bootstraps per bit pair (examples/lut_add_two_numbers.rs:82-158), for a whole batch, on the device.

    Inputs: int32 CUDA tensors [count][n+1], encryptions of the low / high nibbles of a and b under
    message modulus 32 (`encrypt_lwe_message(nibble, 32, ...)`, :99-122).  Returns
    (sum_low, sum_high, carry) as device tensors, each decrypting (modulus 32) to the nibble / bit.

    Every TLWE addition the example performs with `&x + &y` is folded into the prologue of the
    bootstrap that consumes it (tfhe_hip_batch_lincomb_bootstrap_dev), or is one streaming kernel
    (tfhe_hip_batch_tlwe_lincomb_dev) for the three-operand high sum; nothing leaves HBM."""
    import torch

    from .lut import Generator

    gen = Generator(32)  # message modulus 32 covers every possible nibble sum 0..30 (:86-87)
    dev = a_low.device
    with _on_stream(stream):  # uploads, allocations and kernels on one stream (see Circuit.run_dev)
        lut_mod16 = torch.from_numpy(gen.generate_lookup_table(lambda x: x % 16).poly.view(np.int32)).to(dev)
        lut_carry = torch.from_numpy(gen.generate_lookup_table(lambda x: 1 if x >= 16 else 0).poly.view(np.int32)).to(dev)
        sum_low, carry = torch.empty_like(a_low), torch.empty_like(a_low)
        high, sum_high = torch.empty_like(a_low), torch.empty_like(a_low)
        # bootstraps 1 and 2: low sum mod 16 and its carry, both from a_low + b_low (:124-150)
        eng.batch_lincomb_bootstrap_dev(1, a_low, 1, b_low, 0, sum_low, testvec=lut_mod16)
        eng.batch_lincomb_bootstrap_dev(1, a_low, 1, b_low, 0, carry, testvec=lut_carry)
        # a_high + b_high (:152-153), then bootstrap 3 on (a_high + b_high) + carry (:155-158)
        eng.batch_tlwe_lincomb_dev(1, a_high, 1, b_high, 0, high)
        eng.batch_lincomb_bootstrap_dev(1, high, 1, carry, 0, sum_high, testvec=lut_mod16)
    return sum_low, sum_high, carry


def mux_and_gates_dev(eng, a, b, c, codes, xa, xb, stream=None):
    """One circuit level holding `M` Gates::mux (the reference's formula, src/gates.rs:157-183) beside `X` two-input
    gates (`codes`: uint8 device tensor [X]) -- BASELINE configs[4] is M hom_mux + X hom_xor -- in TWO blind-rotation
    launches and ONE key switch whatever M and X:
      launch 1  [and(a, b) | and(not(a), c)] for all M, bootstrap_without_key_switch      (gates.rs:165-177)
      launch 2  [or(u1, u2) for all M | the X other gates], full bootstrap                   (gates.rs:179-182)
    a, b, c: int32 CUDA tensors [M][n+1]; xa, xb: [X][n+1].  Returns (mux_out [M][n+1], gate_out [X][n+1]).
    `eng`: an Engine, or a Pool (tensors on its home member's GPU): each of the two launches is then a pool call cut
    over the members -- configs[4]'s level through ONE handle."""
    import torch

    M, X = a.shape[0], xa.shape[0]
    with _on_stream(stream):
        g1 = torch.empty(2 * M, dtype=torch.uint8, device=a.device)
        g1[:M] = E.AND
        g1[M:] = E.ANDNY
        u = torch.empty((2 * M, a.shape[1]), dtype=torch.int32, device=a.device)
        eng.batch_gates_mixed_dev(g1, torch.cat([a, a]), torch.cat([b, c]), u, keyswitch=False)
        g2 = torch.cat([torch.full((M,), E.OR, dtype=torch.uint8, device=a.device), codes])
        out = torch.empty((M + X, a.shape[1]), dtype=torch.int32, device=a.device)
        eng.batch_gates_mixed_dev(g2, torch.cat([u[:M], xa]), torch.cat([u[M:], xb]), out)
    return out[:M], out[M:]


def lut_add_u8(eng, a_low, a_high, b_low, b_high):
    """Host-array form of lut_add_u8_dev: numpy [count][n+1] in, (sum_low, sum_high, carry) out."""
    from .lut import Generator

    gen = Generator(32)
    lut_mod16 = gen.generate_lookup_table(lambda x: x % 16).poly
    lut_carry = gen.generate_lookup_table(lambda x: 1 if x >= 16 else 0).poly
    sum_low = eng.batch_lincomb_bootstrap(1, a_low, 1, b_low, testvec=lut_mod16)
    carry = eng.batch_lincomb_bootstrap(1, a_low, 1, b_low, testvec=lut_carry)
    high = eng.batch_tlwe_lincomb(1, a_high, 1, b_high)
    sum_high = eng.batch_lincomb_bootstrap(1, high, 1, carry, testvec=lut_mod16)
    return sum_low, sum_high, carry


def lut_add_u8_digits(c: "Circuit", a_digits, b_digits, n_luts: int = 2):
    """An 8-bit adder over base-4 digits: a_digits / b_digits are 4 wires each (least significant first), encryptions
    of 2-bit digits under message modulus 8 (`encrypt_lwe_message(d, 8, ...)`).  Digit i bootstraps a_i + b_i + carry
    (at most 7) once through a 2-LUT table (x mod 4, x div 4): 4 blind rotations for the byte where single LUTs take 8
    (m * k = 16, the SECURITY_UINT4 precision bound; Generator.generate_many_lookup_table).  n_luts=1 builds the same
    adder from two single-LUT bootstraps per digit, for comparison.  Returns (sum digit wires, carry wires); the byte
    is sum(s_i * 4^i) & 0xFF, each wire decrypting under modulus 8."""
    from .lut import Generator

    assert len(a_digits) == len(b_digits) == 4
    gen = Generator(8)
    fs = [lambda x: x % 4, lambda x: x // 4]
    if n_luts == 2:
        lut2 = c.lut(gen.generate_many_lookup_table(fs).poly)
    else:
        lut_s, lut_c = (c.lut(gen.generate_lookup_table(f).poly) for f in fs)
    sums, carries, carry = [], [], None
    for a, b in zip(a_digits, b_digits):
        if carry is None:
            ca, x, cb, y = 1, a, 1, b
        else:
            ca, x, cb, y = 1, c.lincomb([(1, a), (1, b)]), 1, carry
        if n_luts == 2:
            s, carry = c.pbs_many(ca, x, cb, y, 0, lut2, 2)
        else:
            s, carry = c.pbs(ca, x, cb, y, 0, lut_s), c.pbs(ca, x, cb, y, 0, lut_c)
        sums.append(s)
        carries.append(carry)
    return sums, carries
