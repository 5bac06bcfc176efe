"""Every device-pointer entry point of a context on FRAMED operands (tests/dev_buffers.py): each operand `o` words into
a 16-byte chunk (o = 0 .. 3, one mixed run, int8 operands at odd bytes), inputs between pads of 0xFFFFFFFF / 0x80000000,
the output -- itself prefilled with the sentinel -- between pads of the sentinel.  For every (call, shape, offset plan)

  * the output view equals the CPU's words (np.array_equal: the family's own model or the oracle);
  * every pad word of the output frame is still the sentinel (no store outside the output);
  * every pad word of every input frame is still the poison, and the inputs themselves are unchanged;
  * a read outside an input that is USED would have moved the result by 2^31 times a coefficient.

The calls the header demands 16-byte alignment for (packed CMUX d0 / d1 / out, packed encryption and expansion bodies /
out) run framed at offset 0 and must refuse every other offset with TFHE_HIP_EINVAL, nothing touched.

Shapes.  The row width decides the alignment of every row after the first: the LWE dimension takes n = 63, 64, 65, 66
((n + 1) % 4 = 0, 1, 2, 3).  Calls with a blind rotation run on custom sets in the exact-product regime (l = 1,
bgbit = 10: bgbit + log2(2 l) = 11 < 12), where the oracle's words are the one right answer -- its f64 rotation is held
equal to its exact-integer one on a row of every shape before the device runs -- with a base-4 key switch (2, 8) (mfma,
b4, generic, split) and a base-32 one (5, 3) (sliced, generic, split).  Counts 1, 17, 65: one row; a ragged group of the
G-ciphertext key-switch workgroups; one row into a second 64-row tile.  CALLS says what each entry runs on.

DESIGN.md section 4.0a classifies every kernel's accesses to caller memory; what this file runs was judged legal there
first."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import dev_buffers as DB
import ks_shapes as S
import lockstep as LS

pytestmark = pytest.mark.gpu

N = 1024
COUNTS = (1, 17, 65)
WIDTH_NS = (63, 64, 65, 66)           # (n + 1) % 4 = 0, 1, 2, 3
KS_BASES = ((2, 8), (5, 3))           # (basebit, t) of the key switch: base 4 and base 32
ROW_NS = WIDTH_NS + (700, 33)         # keyless row calls: also SECURITY_128_BIT's width 701 and a toy width
GEMM_SHAPES = ((1, 1, 1), (33, 31, 2), (65, 100, 3))  # (rows, cols, groups)
CONV_GEOMS = ((5, 5, 3, 3, 3, 3, (1, 1), (1, 1)),     # padding on every side, in_c % 16 != 0 (taps cross inside a fetch)
              (5, 5, 16, 3, 3, 3, (1, 1), (1, 1)))    # in_c % 16 == 0: one tap per fetch, the aligned weight loads at plan all0
POLYMUL_SHAPE = (2, 3, 2)             # (rows, cols, groups)
GADGETS = ((4, 8), (6, 3))            # TRLWE switch / CMUX: basebit t == 32, and below it
SEED = bytes((29 * i + 3) & 0xFF for i in range(32))  # a public mask seed
HIGH = (1 << 32) - 3                  # a first index whose rows cross a carry of the low nonce word

Case = namedtuple("Case", "label inputs out_like expected run")
Entry = namedtuple("Entry", "groups cases shapes")


def _words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def _plans(case):
    """every plan; the bytes-only one where an int8 operand exists"""
    has8 = any(v is not None and np.asarray(v).dtype.itemsize == 1 for v in case.inputs.values())
    return DB.PLANS if has8 else DB.WORD_PLANS


RAN = {"framed": 0}  # framed calls checked so far: the sweeps assert that theirs ran


def run_case(eng, case, plans=None, at=None):
    import torch

    for plan in plans or _plans(case):
        f = DB.Framed(case.inputs, case.out_like, plan, at=at)
        assert all(v is None or v.is_cuda for v in f.views.values()) and all(o.is_cuda for o in f.outs.values())
        case.run(eng, f.views, f.out if f.single else f.outs)
        torch.cuda.synchronize()
        f.check(case.expected, case.label)
        RAN["framed"] += 1


def run_refused(eng, case, plan, at):
    """the call must return TFHE_HIP_EINVAL and leave the output (all sentinel) and every frame as they were"""
    import torch

    from rs_tfhe_amd import _capi

    f = DB.Framed(case.inputs, case.out_like, plan, at=at)
    with pytest.raises(_capi.TfheHipError) as err:
        case.run(eng, f.views, f.out if f.single else f.outs)
    assert err.value.code == _capi.EINVAL, (case.label, plan.name, at, str(err.value))
    torch.cuda.synchronize()
    f.check_untouched(f"{case.label} at {at}")


# ---- calls with a blind rotation or a key switch: custom sets, the oracle's words ------------------------------------------
_BOOT = {}


class Boot:
    """One (n, basebit, t): the oracle's keys, the product's CloudKey, 65 rows of every operand, the expected words of
    every call (made when first asked for, kept: every kernel of the sweep shares them)."""

    def __init__(self, O, n, basebit, t):
        import rs_tfhe_amd as R
        from rs_tfhe_amd import packing as PK
        from rs_tfhe_amd.params import SecurityParams

        self.O, self.n, self.basebit, self.t = O, n, basebit, t
        l, bgbit = 1, 10
        assert bgbit + np.log2(2 * l) < 12  # the exact-product regime
        self.op = O.Params(f"DEVBUF_n{n}_b{basebit}_t{t}", n, l, bgbit, basebit, t, 2.0e-5, 2.0e-8)
        self.sk, self.ck = O.keygen(self.op, 7000 + 8 * n + basebit, with_time_domain=True)
        self.pp = SecurityParams(self.op.name, 0, n, l, bgbit, basebit, t, self.op.alpha_lv0, self.op.alpha_lv1)
        ck = self.ck
        self.cloud_key = R.CloudKey(self.pp, ck.bootstrapping_key, ck.key_switching_key, ck.decomposition_offset,
                                    ck.blind_rotate_testvec)
        rng = np.random.default_rng(100 * n + basebit)
        m = max(COUNTS)
        self.a, self.b, self.c = (_words(rng, (m, n + 1)) for _ in range(3))
        self.tv = _words(rng, (2, N))
        self.tv_per_ct = _words(rng, (m, 2, N))
        self.codes = np.concatenate([np.arange(11), rng.integers(0, 11, m - 11)]).astype(np.uint8)
        rng.shuffle(self.codes[1:])  # (a batch of one runs NAND)
        self.biv_tabs = _words(rng, (2, 2, N))  # m = 2, one function a table
        self.packing_key = PK.PackingKey(self.pp, S.MASK_SEED, _words(rng, (n, t, N)))
        self.reenc_key = _words(rng, (n * t * (1 << basebit), n + 1))
        self.reenc_key[::1 << basebit] = 0  # the k = 0 rows
        self.trlwe = _words(rng, (2, 2, N))
        self.slots = np.concatenate([[0, 1, N - 1, N, 2 * N - 1], rng.integers(0, 2 * N, m - 5)]).astype(np.uint32)
        self._want = {}
        # the oracle itself is exact here: its f64 blind rotation is the exact-integer one
        assert np.array_equal(O.batch_blind_rotate(ck, self.a[:1], self.tv)[0], O.blind_rotate(ck, self.a[0], self.tv, exact=True))

    def want(self, key, make):
        if key not in self._want:
            self._want[key] = make()
        return self._want[key]

    def prep(self, ca, cb, cc):
        p = (np.uint32(ca) * self.a + np.uint32(cb) * self.b).astype(np.uint32)
        p[:, -1] += np.uint32(cc)
        return p


def boot(O, n, basebit, t):
    key = (n, basebit, t)
    if key not in _BOOT:
        _BOOT[key] = Boot(O, n, basebit, t)
    return _BOOT[key]


LIN = (1, 3, 0x12345678)  # (ca, cb, cconst) of the lincomb forms


def _gate(B, count, group):
    O = B.O
    want = B.want("gate", lambda: O.batch_gate(B.ck, O.GATE_XOR, B.a, B.b))
    return [Case("batch_gate_dev", {"a": B.a[:count], "b": B.b[:count]}, want[:count], want[:count],
                 lambda e, v, out: e.batch_gate_dev(O.GATE_XOR, v["a"], v["b"], out))]


def _by_code(B, one):
    """rows of a per-ciphertext gate call: `one(code, rows)` over the rows of every code"""
    out = np.empty_like(B.a)
    for g in np.unique(B.codes):
        idx = np.flatnonzero(B.codes == g)
        out[idx] = one(int(g), idx)
    return out


def _gates_mixed(B, count, group):
    O = B.O
    want = B.want("mixed", lambda: _by_code(B, lambda g, i: O.batch_gate(B.ck, g, B.a[i], None if g == O.GATE_COPY else B.b[i])))
    return [Case("batch_gates_mixed_dev", {"gates": B.codes[:count], "a": B.a[:count], "b": B.b[:count]}, want[:count],
                 want[:count], lambda e, v, out: e.batch_gates_mixed_dev(v["gates"], v["a"], v["b"], out))]


def _gates_mixed_nks(B, count, group):
    O = B.O

    def make():
        prep = np.stack([O.gate_prep(int(g), B.a[i], None if g == O.GATE_COPY else B.b[i], B.n) for i, g in enumerate(B.codes)])
        return O.batch_bootstrap(B.ck, prep, keyswitch=False)

    want = B.want("mixed_nks", make)
    return [Case("batch_gates_mixed_nks_dev", {"gates": B.codes[:count], "a": B.a[:count], "b": B.b[:count]}, want[:count],
                 want[:count], lambda e, v, out: e.batch_gates_mixed_dev(v["gates"], v["a"], v["b"], out, keyswitch=False))]


def _bootstrap(B, count, group):
    O = B.O
    if group == "ks":  # one table for the batch, the key switch writes the output
        want = B.want("boot_ks", lambda: O.batch_bootstrap(B.ck, B.a, testvec=B.tv))
        return [Case("batch_bootstrap_dev", {"in": B.a[:count], "testvec": B.tv}, want[:count], want[:count],
                     lambda e, v, out: e.batch_bootstrap_dev(v["in"], out, v["testvec"]))]
    want = B.want("boot_nks", lambda: O.batch_bootstrap(B.ck, B.a, testvec=B.tv_per_ct, keyswitch=False))
    return [Case("batch_bootstrap_dev(per-ct table, no key switch)", {"in": B.a[:count], "testvec": B.tv_per_ct[:count]},
                 want[:count], want[:count],
                 lambda e, v, out: e.batch_bootstrap_dev(v["in"], out, v["testvec"], per_ct=True, keyswitch=False))]


def _lincomb_bootstrap(B, count, group):
    O, ks = B.O, group == "ks"
    want = B.want(("lin", ks), lambda: O.batch_bootstrap(B.ck, B.prep(*LIN), testvec=B.tv, keyswitch=ks))
    return [Case(f"batch_lincomb_bootstrap_dev(keyswitch={ks})", {"a": B.a[:count], "b": B.b[:count], "testvec": B.tv},
                 want[:count], want[:count],
                 lambda e, v, out: e.batch_lincomb_bootstrap_dev(LIN[0], v["a"], LIN[1], v["b"], LIN[2], out, v["testvec"], keyswitch=ks))]


def _lincomb_bootstrap_many(B, count, group):
    from test_gpu_many_lut import many_model

    ks = group == "ks"
    both = B.want("many", lambda: many_model(B.O, B.ck, B.prep(*LIN), B.tv, 2, both=True))  # ([2][65][n+1] with, without)
    want = np.ascontiguousarray(both[0 if ks else 1][:, :count])
    return [Case(f"batch_lincomb_bootstrap_many_dev(k=2, keyswitch={ks})", {"a": B.a[:count], "b": B.b[:count], "testvec": B.tv},
                 want, want,
                 lambda e, v, out: e.batch_lincomb_bootstrap_many_dev(LIN[0], v["a"], LIN[1], v["b"], LIN[2], out, v["testvec"],
                                                                     n_luts=2, keyswitch=ks))]


def _blind_rotate(B, count, group):
    want = B.want("rot", lambda: B.O.batch_blind_rotate(B.ck, B.a, B.tv))
    return [Case("batch_blind_rotate_dev", {"in": B.a[:count], "testvec": B.tv}, want[:count], want[:count],
                 lambda e, v, out: e.batch_blind_rotate_dev(v["in"], out, v["testvec"]))]


def _mux(B, count, group):
    cases = []
    for naive in (True, False):
        want = B.want(("mux", naive), lambda: B.O.batch_mux(B.ck, B.a, B.b, B.c, naive=naive))
        cases.append(Case(f"batch_mux_dev(naive={naive})", {"a": B.a[:count], "b": B.b[:count], "c": B.c[:count]}, want[:count],
                          want[:count], lambda e, v, out, naive=naive: e.batch_mux_dev(v["a"], v["b"], v["c"], out, naive)))
    return cases


def _bivariate(B, count, group):
    """m = 2, one function a table: stage 1 on the oracle, packing.table_model, the oracle's per-ciphertext bootstrap"""
    from rs_tfhe_amd import packing as PK

    O, ks, pk = B.O, group == "ks", B.packing_key

    def tables():
        stage1 = np.stack([O.batch_bootstrap(B.ck, B.b, testvec=B.biv_tabs[x]) for x in range(2)])
        return PK.table_model(B.pp, pk.mask_seed, pk.bodies, stage1, 2)

    want = B.want(("biv", ks), lambda: O.batch_bootstrap(B.ck, B.a, testvec=B.want("biv_tv", tables), keyswitch=ks))
    return [Case(f"batch_bootstrap_bivariate_dev(keyswitch={ks})", {"x": B.a[:count], "y": B.b[:count], "testvecs": B.biv_tabs},
                 want[:count], want[:count],
                 lambda e, v, out: e.batch_bootstrap_bivariate_dev(v["x"], v["y"], v["testvecs"], 2, out, keyswitch=ks))]


def _reencrypt(B, count, group):
    want = B.want("reenc", lambda: B.O.reencrypt_tlwe_lv0(B.op, B.reenc_key, B.a))
    return [Case("batch_reencrypt_dev", {"in": B.a[:count]}, want[:count], want[:count],
                 lambda e, v, out: B.reenc_view.batch_reencrypt_dev(v["in"], out))]


def _unpack(B, count, group):
    from rs_tfhe_amd import packing as PK

    ksk = B.ck.key_switching_key
    by_slot = B.want("unpack_slots", lambda: PK.unpack_model(B.pp, ksk, B.trlwe, slots=B.slots))
    in_order = B.want("unpack_order", lambda: PK.unpack_model(B.pp, ksk, B.trlwe, count=max(COUNTS)))
    return [Case("batch_unpack_trlwe_dev(slots)", {"trlwe": B.trlwe, "slots": B.slots[:count]}, by_slot[:count], by_slot[:count],
                 lambda e, v, out: e.unpack_dev(v["trlwe"], out, count, v["slots"])),
            Case("batch_unpack_trlwe_dev(slots=NULL)", {"trlwe": B.trlwe}, in_order[:count], in_order[:count],
                 lambda e, v, out: e.unpack_dev(v["trlwe"], out, count))]


def _trlwe_matmul_ks(B, count, group):
    """the packed linear layer through the key switch: the GEMM shapes, at the sweep's middle count alone (its own
    counts are rows x groups = 1, 66, 195)"""
    from rs_tfhe_amd import linear as L
    from test_gpu_matmul import packed_case

    if count != COUNTS[1]:
        return []
    cases = []
    for i, (rows, cols, groups) in enumerate(GEMM_SHAPES):
        w, bias, trlwe = packed_case(rows, cols, groups, 400 + i)

        def make(w=w, bias=bias, trlwe=trlwe, rows=rows, groups=groups):
            lv1 = L.matmul_packed_model(B.pp, w, trlwe, bias)
            return B.O.batch_identity_key_switching(B.ck, lv1.reshape(-1, N + 1)).reshape(groups, rows, B.n + 1)

        want = B.want(("pmm", i), make)
        cases.append(Case(f"batch_trlwe_matmul_dev(keyswitch, {rows}x{cols}x{groups})", {"w": w, "bias": bias, "trlwe": trlwe},
                          want, want, lambda e, v, out: e.batch_trlwe_matmul_dev(v["w"], v["trlwe"], out, v["bias"])))
    return cases


# ---- the circuit: a store of the caller's ----------------------------------------------------------------------------------
def _circuit():
    """gates, a NOT folded into a gate, a programmable bootstrap, one linear node formed where it is read and one
    materialised (three source wires): every launch kind but the mux's, whose scratch slots hold no wire"""
    import rs_tfhe_amd as R

    c = R.Circuit(3)
    g1 = c.nand(0, 1)
    g2 = c.xor(c.not_(g1), 2)
    lin = c.lincomb([(1, 0), (3, g2)], 5)
    lid = c.lut(R.lut.Generator(2).generate_lookup_table(lambda x: 1 - x).poly)
    p = c.pbs(1, g2, 1, 0, 0, lid)
    c.or_(lin, p)
    return c, lin


def circuit_cases(B, batch):
    """(run case, gather case): tfhe_hip_circuit_run_dev writes the whole store [slots][batch][n+1] from framed inputs,
    tfhe_hip_circuit_gather_dev every wire [n_wires][batch][n+1] from a framed store"""
    from rs_tfhe_amd import _capi

    O = B.O
    c, lin = _circuit()
    inputs = np.stack([B.a[:batch], B.b[:batch], B.c[:batch]])
    ref = B.want(("circuit", batch), lambda: c.run_reference(
        lambda op, x, y: O.batch_gate(B.ck, op, x, y), inputs, pbs_fn=lambda tv, x: O.batch_bootstrap(B.ck, x, testvec=tv)))
    slot_of = [c.wire_slot(w) for w in range(c.n_wires)]
    store = np.zeros((c.slots, batch, B.n + 1), np.uint32)
    filled = set()
    for w, s in enumerate(slot_of):
        if s != _capi.NO_SLOT:
            store[s] = ref[w]
            filled.add(s)
    spare = sorted(set(range(c.slots)) - filled)
    assert len(spare) == 1, (slot_of, c.slots)  # the materialised linear node's slot
    store[spare[0]] = ref[lin]
    return (Case(f"circuit_run_dev(batch={batch})", {"inputs": inputs}, store, store,
                 lambda e, v, out: c.run_store_dev(e, v["inputs"], out)),
            Case(f"circuit_gather_dev(batch={batch})", {"wires": store}, ref, ref, lambda e, v, out: c.gather_dev(e, v["wires"], out)))


def _circuit_run(B, count, group):
    return [circuit_cases(B, count)[0]]


def _circuit_gather(B, count, group):
    return [circuit_cases(B, count)[1]]


# ---- keyless calls on rows of n + 1 words -----------------------------------------------------------------------------------
_ROWS = {}


class Rows:
    """One n: the parameter set of tests/pk_encrypt_model.py at that n, its secret key, and what the calls need"""

    def __init__(self, n):
        import pk_encrypt_model as PM
        import keygen_model as KM

        self.n = n
        self.pp = PM.params(n)
        self.sk = KM.secret_key(self.pp)
        self._want = {}

    want = Boot.want


def rows_of(n):
    if n not in _ROWS:
        _ROWS[n] = Rows(n)
    return _ROWS[n]


def _tlwe_matmul(R_, count, group):
    from rs_tfhe_amd import linear as L
    from test_gpu_matmul import dense_case

    if count != COUNTS[0]:  # (the GEMM shapes are the counts)
        return []
    cases = []
    for i, (rows, cols, groups) in enumerate(GEMM_SHAPES):
        w, bias, cts = dense_case(R_.pp, rows, cols, groups, 500 + i)
        want = R_.want(("mm", i), lambda: L.matmul_model(R_.pp, w, cts, bias))
        cases.append(Case(f"batch_tlwe_matmul_dev({rows}x{cols}x{groups}, n={R_.n})", {"w": w, "bias": bias, "cts": cts}, want, want,
                          lambda e, v, out: e.batch_tlwe_matmul_dev(v["w"], v["cts"], out, v["bias"])))
    return cases


def _conv2d(R_, count, group):
    from test_gpu_conv2d import case as conv_case

    if count != COUNTS[0]:
        return []
    cases = []
    for i, geom in enumerate(CONV_GEOMS):
        w, bias, cts, stride, padding, want = conv_case(R_.pp, geom, 2, 600 + i)
        cases.append(Case(f"batch_tlwe_conv2d_dev(in_c={geom[2]}, n={R_.n})", {"w": w, "bias": bias, "cts": cts}, want, want,
                          lambda e, v, out, s=stride, p=padding: e.batch_tlwe_conv2d_dev(v["w"], v["cts"], out, v["bias"], s, p)))
    return cases


def _decrypt(R_, count, group):
    cts = R_.want("dec_in", lambda: _words(np.random.default_rng(70 + R_.n), (max(COUNTS), R_.n + 1)))[:count]
    phase = R_.sk.phase(cts)
    return [Case(f"batch_decrypt_dev(phase, n={R_.n})", {"in": cts}, phase, phase,
                 lambda e, v, out: e.batch_decrypt_dev(R_.sk, v["in"], out, "phase")),
            Case(f"batch_decrypt_dev(bool, n={R_.n})", {"in": cts}, phase, (phase.view(np.int32) >= 0).astype(np.uint32),
                 lambda e, v, out: e.batch_decrypt_dev(R_.sk, v["in"], out, "bool"))]


def _encrypt(R_, count, group):
    """alpha = 0: no noise sample is borderline, the words are the model's"""
    import sym_encrypt_model as SM

    plain = SM.plaintexts(count, R_.n)
    want, border = SM.bulk(R_.sk.key_lv0, plain, HIGH, 0.0, SEED, SM.K)
    assert not border.any()
    enc = lambda e, v, **kw: e.batch_encrypt_dev(R_.sk.key_lv0, v["plain"], 0.0, SEED, SM.K, HIGH, **kw)  # noqa: E731
    bodies = np.ascontiguousarray(want[:, -1])
    return [Case(f"batch_encrypt_dev(out, n={R_.n})", {"plain": plain}, want, want, lambda e, v, out: enc(e, v, out=out)),
            Case(f"batch_encrypt_dev(bodies, n={R_.n})", {"plain": plain}, bodies, bodies, lambda e, v, out: enc(e, v, bodies=out)),
            Case(f"batch_encrypt_dev(bodies and out, n={R_.n})", {"plain": plain}, {"out": want, "bodies": bodies},
                 {"out": want, "bodies": bodies}, lambda e, v, outs: enc(e, v, out=outs["out"], bodies=outs["bodies"]))]


def _expand_seeded_tlwe(R_, count, group):
    from rs_tfhe_amd.seeded import SeededCiphertexts

    bodies = _words(np.random.default_rng(80 + R_.n + count), (count,))
    want = SeededCiphertexts(R_.pp, SEED, HIGH, bodies).expand()
    return [Case(f"expand_seeded_tlwe_dev(n={R_.n})", {"bodies": bodies}, want, want,
                 lambda e, v, out: e.expand_seeded_dev(SEED, HIGH, v["bodies"], out))]


PK_SIZE = 66


def _pk_encrypt(R_, count, group):
    import pk_encrypt_model as PM

    enc = R_.want("pk", lambda: PM.public_key(R_.n, PK_SIZE))
    plain = _words(np.random.default_rng(90 + R_.n), (count,))
    want, border = PM.encrypt(enc, PM.K, PM.row_indices(HIGH, count), plain, 0.0)
    assert not border.any()
    return [Case(f"batch_pk_encrypt_dev(n={R_.n})", {"plain": plain}, want, want,
                 lambda e, v, out: e.batch_pk_encrypt_dev(v["plain"], out, 0.0, PM.K, HIGH))]


def _pack_key(R_):
    from rs_tfhe_amd import packing as PK

    def make():
        pk = PK.PackingKey(R_.pp, S.MASK_SEED, S.build_pack_bodies(R_.n, R_.pp.basebit, R_.pp.iks_t))
        return pk, PK.key_rows(R_.pp, pk.mask_seed, pk.bodies)

    return R_.want("pack_key", make)


def _pack_tlwe(R_, count, group):
    from rs_tfhe_amd import packing as PK

    pk, rows = _pack_key(R_)
    cts = S.build_tlwe(R_.n, R_.pp.basebit, R_.pp.iks_t, max(COUNTS), 0)[:count]
    want = PK.pack_model(R_.pp, pk.mask_seed, pk.bodies, cts, rows=rows)  # [1][2][N]: the one, partial, group
    return [Case(f"batch_pack_tlwe_dev(n={R_.n})", {"in": cts}, want, want, lambda e, v, out: e.pack_dev(v["in"], out))]


def _pack_table(R_, count, group):
    """m = 2 (W = 512) at every count, m = 64 (W = 16: a ciphertext's rows span two 32-row blocks) at count 1"""
    from rs_tfhe_amd import packing as PK

    pk, rows = _pack_key(R_)
    cases = []
    for m in (2, 64) if count == COUNTS[0] else (2,):
        stage1 = S.build_tlwe(R_.n, R_.pp.basebit, R_.pp.iks_t, m * count, m).reshape(m, count, R_.n + 1)
        want = PK.table_model(R_.pp, pk.mask_seed, pk.bodies, stage1, m, rows=rows)
        cases.append(Case(f"batch_pack_table_dev(m={m}, n={R_.n})", {"in": stage1}, want, want,
                          lambda e, v, out, m=m: e.pack_table_dev(v["in"], m, out)))
    return cases


def _tlwe_lincomb(R_, count, group):
    rng = np.random.default_rng(60 + R_.n)
    a, b = _words(rng, (count, R_.n + 1)), _words(rng, (count, R_.n + 1))
    want = lincomb_model(3, a, 0xFFFFFFFE, b, 0x40000000)
    return [Case(f"batch_tlwe_lincomb_dev(n={R_.n})", {"a": a, "b": b}, want, want,
                 lambda e, v, out: e.batch_tlwe_lincomb_dev(3, v["a"], 0xFFFFFFFE, v["b"], 0x40000000, out))]


def lincomb_model(ca, a, cb, b, cc):
    out = (np.uint32(ca) * a + np.uint32(cb) * b).astype(np.uint32)
    out[:, -1] += np.uint32(cc)
    return out


# ---- calls on packed ciphertexts: rows of N or 2N words, the base offset alone moves -------------------------------------------
def _secret(seed):
    return np.random.default_rng(seed).integers(0, 2, N).astype(np.uint32)


def _trlwe_matmul_nks(_, count, group):
    """no key switch: lv1 rows of N + 1 = 1025 words, so rows start at every word of a chunk"""
    from rs_tfhe_amd import linear as L
    from rs_tfhe_amd.params import SECURITY_128_BIT as p
    from test_gpu_matmul import packed_case

    if count != 1:  # (the GEMM shapes are the counts)
        return []
    cases = []
    for i, (rows, cols, groups) in enumerate(GEMM_SHAPES):
        w, bias, trlwe = packed_case(rows, cols, groups, 410 + i)
        want = L.matmul_packed_model(p, w, trlwe, bias)
        cases.append(Case(f"batch_trlwe_matmul_dev(no key switch, {rows}x{cols}x{groups})", {"w": w, "bias": bias, "trlwe": trlwe},
                          want, want, lambda e, v, out: e.batch_trlwe_matmul_dev(v["w"], v["trlwe"], out, v["bias"], keyswitch=False)))
    return cases


def _polymul(_, count, group):
    from rs_tfhe_amd import linear as L

    if count != 1:
        return []
    rows, cols, groups = POLYMUL_SHAPE
    rng = np.random.default_rng(20)
    w = rng.integers(-128, 128, (rows, cols, N)).astype(np.int8)
    w[0, 0], w[0, 1] = -128, 127
    bias, trlwe = _words(rng, (rows, N)), _words(rng, (groups, cols, 2, N))
    want = L.polymul_model(w, trlwe, bias)
    return [Case("batch_trlwe_polymul_dev", {"w": w, "bias": bias, "trlwe": trlwe}, want, want,
                 lambda e, v, out: e.batch_trlwe_polymul_dev(v["w"], v["trlwe"], out, v["bias"]))]


def _trlwe_keyswitch(_, count, group):
    import trlwe_switch_model as TM
    from rs_tfhe_amd.packing import TrlweSwitchKey

    cases = []
    for basebit, t in GADGETS:
        k = 3
        rng = np.random.default_rng(30 + basebit)
        bodies, ct = _words(rng, (t, N)), _words(rng, (count, 2, N))
        key = TrlweSwitchKey(k, basebit, t, SEED, bodies)
        want = TM.switch(TM.key_rows(SEED, k, t, bodies), k, basebit, t, ct)

        def run(e, v, out, key=key):
            e.load_trlwe_switch_key(key)
            try:
                e.batch_trlwe_keyswitch(key.k, v["in"], out=out)
            finally:
                import torch

                torch.cuda.synchronize()
                e.drop_trlwe_switch_key(key.k)

        cases.append(Case(f"batch_trlwe_keyswitch_dev({basebit}, {t})", {"in": ct}, want, want, run))
    return cases


def _cmux_operands(basebit, t, count):
    import cmux_model as CM

    rng = np.random.default_rng(40 + basebit)
    sel, d0, d1 = _words(rng, (2 * t, 2, N)), _words(rng, (count, 2, N)), _words(rng, (count, 2, N))
    return sel, d0, d1, CM.cmux(sel, basebit, t, d0, d1), CM.external_product(sel, basebit, t, d1)


def _cmux(_, count, group):
    """d0 / d1 / out are demanded 16-byte aligned: here at offset 0, the selector (which is not) at the plan's"""
    cases = []
    for basebit, t in GADGETS:
        sel, d0, d1, want, want_ep = _cmux_operands(basebit, t, count)
        cases.append(Case(f"batch_trlwe_cmux_dev({basebit}, {t})", {"sel": sel, "d0": d0, "d1": d1}, want, want,
                          lambda e, v, out, b=basebit, t=t: e.batch_trlwe_cmux(v["sel"], b, t, v["d0"], v["d1"], out=out)))
        cases.append(Case(f"batch_trlwe_cmux_dev({basebit}, {t}, d0 = NULL)", {"sel": sel, "d1": d1}, want_ep, want_ep,
                          lambda e, v, out, b=basebit, t=t: e.batch_trlwe_cmux(v["sel"], b, t, None, v["d1"], out=out)))
    return cases


def _encrypt_trgsw(_, count, group):
    import cmux_model as CM

    basebit, t = GADGETS[1]
    s = _secret(51)
    mu = np.random.default_rng(52).integers(-3, 4, (count, N)).astype(np.int32)
    want, border, _seed = CM.encrypt_trgsw(s, mu, basebit, t, 0.0, SEED, HIGH)
    assert not border.any()
    return [Case(f"batch_encrypt_trgsw_dev({basebit}, {t})", {"mu": mu}, want, want,
                 lambda e, v, out: e.batch_encrypt_trgsw_dev(s, v["mu"], basebit, t, out, alpha=0.0, rng_key=SEED, first_index=HIGH))]


def _decrypt_trlwe(_, count, group):
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    sk = SecretKey(p, np.zeros(p.n, np.uint32), _secret(53))
    packed = _words(np.random.default_rng(54), (2, 2, N))
    cases = []
    for slots in (count, N + count):  # inside the first group; a partial second group
        want = sk.packed_phase(packed, slots)
        cases.append(Case(f"batch_decrypt_trlwe_dev(count={slots})", {"trlwe": packed}, want, want,
                          lambda e, v, out, c=slots: e.batch_decrypt_trlwe_dev(sk, v["trlwe"], c, out)))
    return cases


def _encrypt_trlwe(_, count, group):
    """bodies / out are demanded 16-byte aligned (offset 0 here); plain is not"""
    import packed_encrypt_model as PE

    s1 = _secret(55)
    slots = N + count  # a whole group and a partial one
    plain = PE.plaintexts(slots, 5)
    want, border = PE.encrypt(s1, plain, slots, HIGH, 0.0, SEED, PE.K)
    assert not border.any()
    bodies = np.ascontiguousarray(want[:, 1])
    enc = lambda e, v, **kw: e.batch_encrypt_trlwe_dev(s1, v["plain"], 0.0, SEED, PE.K, HIGH, **kw)  # noqa: E731
    return [Case("batch_encrypt_trlwe_dev(out)", {"plain": plain}, want, want, lambda e, v, out: enc(e, v, out=out)),
            Case("batch_encrypt_trlwe_dev(bodies and out)", {"plain": plain}, {"out": want, "bodies": bodies},
                 {"out": want, "bodies": bodies}, lambda e, v, outs: enc(e, v, out=outs["out"], bodies=outs["bodies"]))]


def _expand_seeded_trlwe(_, count, group):
    import packed_encrypt_model as PE

    groups = 2
    bodies = _words(np.random.default_rng(56), (groups, N))
    want = np.stack([PE.masks(SEED, PE.group_indices(HIGH, groups)), bodies], axis=1)
    return [Case("expand_seeded_trlwe_dev", {"bodies": bodies}, want, want,
                 lambda e, v, out: e.expand_seeded_trlwe_dev(SEED, HIGH, v["bodies"], out))]


# ---- the table: one entry per device-pointer entry point ---------------------------------------------------------------------
# groups: "ks"     the output is written by a key-switch kernel: every TFHE_HIP_KS_KERNEL of the shape, n = 63 .. 66 x both bases
#         "br"     the output is written by a blind-rotation epilogue: every TFHE_HIP_BR_KERNEL, n = 63 .. 66 (base 4: the
#                  key switch does not run)
#         "rows"   keyless, rows of n + 1 words: n = 63 .. 66, 700, 33
#         "packed" rows of N, N + 1 or 2N words: one engine, the base offset alone moves
#         "aligned" as "packed", and the header demands 16-byte alignment of some operands: see test_alignment_refusals
CALLS = {
    "tfhe_hip_batch_gate_dev": Entry(("ks",), _gate, "counts 1, 17, 65; XOR"),
    "tfhe_hip_batch_gates_mixed_dev": Entry(("ks",), _gates_mixed, "counts 1, 17, 65; all eleven codes, byte offsets"),
    "tfhe_hip_batch_gates_mixed_nks_dev": Entry(("br",), _gates_mixed_nks, "counts 1, 17, 65; all eleven codes"),
    "tfhe_hip_batch_bootstrap_dev": Entry(("ks", "br"), _bootstrap, "counts 1, 17, 65; one table / per-ciphertext tables"),
    "tfhe_hip_batch_lincomb_bootstrap_dev": Entry(("ks", "br"), _lincomb_bootstrap, "counts 1, 17, 65"),
    "tfhe_hip_batch_lincomb_bootstrap_many_dev": Entry(("ks", "br"), _lincomb_bootstrap_many, "counts 1, 17, 65; k = 2"),
    "tfhe_hip_batch_blind_rotate_dev": Entry(("br",), _blind_rotate, "counts 1, 17, 65"),
    "tfhe_hip_batch_mux_dev": Entry(("ks",), _mux, "counts 1, 17, 65; both forms"),
    "tfhe_hip_batch_bootstrap_bivariate_dev": Entry(("ks", "br"), _bivariate, "counts 1, 17, 65; m = 2"),
    "tfhe_hip_batch_reencrypt_dev": Entry(("ks",), _reencrypt, "counts 1, 17, 65; a key view holds the key"),
    "tfhe_hip_batch_unpack_trlwe_dev": Entry(("ks",), _unpack, "counts 1, 17, 65 of two groups; slots given and NULL"),
    "tfhe_hip_batch_trlwe_matmul_dev": Entry(("ks", "packed"), lambda x, c, g: (_trlwe_matmul_ks if g == "ks" else _trlwe_matmul_nks)(x, c, g),
                                             "the GEMM shapes; through the key switch, and lv1 rows of 1025 words without"),
    "tfhe_hip_circuit_run_dev": Entry(("ks",), _circuit_run, "batches 1, 17, 65: the whole store is the output"),
    "tfhe_hip_circuit_gather_dev": Entry(("ks",), _circuit_gather, "batches 1, 17, 65: every wire out of a framed store"),
    "tfhe_hip_batch_tlwe_matmul_dev": Entry(("rows",), _tlwe_matmul, "the GEMM shapes"),
    "tfhe_hip_batch_tlwe_conv2d_dev": Entry(("rows",), _conv2d, "5 x 5 maps, 3 x 3 filters, padding 1: in_c = 3 and in_c = 16"),
    "tfhe_hip_batch_decrypt_dev": Entry(("rows",), _decrypt, "counts 1, 17, 65 (four rows a workgroup); phase and bool"),
    "tfhe_hip_batch_encrypt_dev": Entry(("rows",), _encrypt, "counts 1, 17, 65 (sixteen rows a workgroup); out, bodies, both"),
    "tfhe_hip_expand_seeded_tlwe_dev": Entry(("rows",), _expand_seeded_tlwe, "counts 1, 17, 65"),
    "tfhe_hip_batch_pk_encrypt_dev": Entry(("rows",), _pk_encrypt, "counts 1, 17, 65 (32-row blocks); key of 66 rows"),
    "tfhe_hip_batch_pack_tlwe_dev": Entry(("rows",), _pack_tlwe, "counts 1, 17, 65 (32-row blocks): one partial group"),
    "tfhe_hip_batch_pack_table_dev": Entry(("rows",), _pack_table, "m = 2 and 64"),
    "tfhe_hip_batch_tlwe_lincomb_dev": Entry(("rows",), _tlwe_lincomb, "counts 1, 17, 65; aliasing: test_lincomb_out_may_alias"),
    "tfhe_hip_batch_trlwe_polymul_dev": Entry(("packed",), _polymul, "(2, 3, 2), with a bias"),
    "tfhe_hip_batch_trlwe_keyswitch_dev": Entry(("packed",), _trlwe_keyswitch, "(4, 8) and (6, 3), k = 3; counts 1, 65: one wave a ciphertext, then the 64-row tile of the contraction -- no G-ciphertext group for 17 to be ragged in"),
    "tfhe_hip_batch_encrypt_trgsw_dev": Entry(("packed",), _encrypt_trgsw, "counts 1, 3: one wave a row of a selector (6 rows each), no tile over rows"),
    "tfhe_hip_batch_decrypt_trlwe_dev": Entry(("packed",), _decrypt_trlwe, "two groups; counts inside the first and in the second"),
    "tfhe_hip_batch_trlwe_cmux_dev": Entry(("aligned",), _cmux, "(4, 8) and (6, 3), with and without d0; counts 1, 65 as for the TRLWE switch (the same digit and contraction tiling)"),
    "tfhe_hip_batch_encrypt_trlwe_dev": Entry(("aligned",), _encrypt_trlwe, "a whole group and a partial one"),
    "tfhe_hip_expand_seeded_trlwe_dev": Entry(("aligned",), _expand_seeded_trlwe, "two groups"),
}
# what `at` pins to offset 0 for the calls that demand alignment (the other operands follow the plan)
DEMANDED = {
    "tfhe_hip_batch_trlwe_cmux_dev": ("d0", "d1", "out"),
    "tfhe_hip_batch_encrypt_trlwe_dev": ("bodies", "out"),
    "tfhe_hip_expand_seeded_trlwe_dev": ("bodies", "out"),
}


def _in(group):
    return [name for name, e in CALLS.items() if group in e.groups]


# ---- the sweeps ---------------------------------------------------------------------------------------------------------------
KS_CASES = [(n, b, t, k) for n in WIDTH_NS for b, t in KS_BASES for k in S.KERNELS if k in S.available(n, b, t)]
BR_CASES = [(n, k) for n in WIDTH_NS for k in LS.BR_KERNEL_ENVS]


def _boot_engine(B):
    """An engine under the environment's forced kernels with B's cloud key and packing key; B.reenc_view is a key view
    of it that holds B's re-encryption key (closed with the engine)."""
    import rs_tfhe_amd as R

    eng = R.Engine(B.pp, 0)
    eng.load_cloud_key(B.cloud_key)
    eng.load_packing_key(B.packing_key)
    B.reenc_view = eng.new_key_view()
    B.reenc_view.load_reenc_key(B.reenc_key)
    return eng


@pytest.mark.parametrize("n,basebit,t,kernel", KS_CASES, ids=[f"n{n}_b{b}_t{t}-{k}" for n, b, t, k in KS_CASES])
def test_outputs_written_by_a_key_switch_kernel(O, monkeypatch, n, basebit, t, kernel):
    """every call whose output a key-switch kernel writes, under each TFHE_HIP_KS_KERNEL the shape admits, at the default
    blind-rotation dispatch"""
    assert {(2, 8): {"mfma", "b4", "generic", "split"}, (5, 3): {"sliced", "generic", "split"}}[(basebit, t)] == S.available(n, basebit, t)
    B = boot(O, n, basebit, t)
    monkeypatch.setenv("TFHE_HIP_KS_KERNEL", kernel)
    monkeypatch.delenv("TFHE_HIP_BR_KERNEL", raising=False)
    eng, before = _boot_engine(B), RAN["framed"]
    try:
        for count in COUNTS:
            assert f"key_switch={kernel}" in eng.describe_dispatch(count), eng.describe_dispatch(count)
            for name in _in("ks"):
                for case in CALLS[name].cases(B, count, "ks"):
                    run_case(eng, case)
    finally:
        eng.close()
    # a count: ten cases and the circuit's run and gather under five plans, the mixed gates under six; the three GEMM
    # shapes under six at one count
    assert RAN["framed"] - before == 3 * (12 * 5 + 6) + 3 * 6


@pytest.mark.parametrize("n,kernel", BR_CASES, ids=[f"n{n}-{k}" for n, k in BR_CASES])
def test_outputs_written_by_a_blind_rotation_epilogue(O, monkeypatch, n, kernel):
    """the forms without a key switch, tfhe_hip_batch_blind_rotate_dev and the many-LUT form at k = 2, under each
    TFHE_HIP_BR_KERNEL, at the default key switch"""
    B = boot(O, n, *KS_BASES[0])
    monkeypatch.delenv("TFHE_HIP_KS_KERNEL", raising=False)
    LS.with_br_kernel(monkeypatch, kernel)
    eng, before = _boot_engine(B), RAN["framed"]
    try:
        for count in COUNTS:
            assert f"blind_rotate={kernel}[0,{count})" in eng.describe_dispatch(count), eng.describe_dispatch(count)
            for name in _in("br"):
                for case in CALLS[name].cases(B, count, "br"):
                    run_case(eng, case)
    finally:
        eng.close()
    assert RAN["framed"] - before == 3 * (5 * 5 + 6)  # a count: five cases under five plans, the mixed gates under six


ROW_CASES = [(name, n) for name in _in("rows") for n in ROW_NS]


@pytest.mark.parametrize("name,n", ROW_CASES, ids=[f"{s[len('tfhe_hip_'):]}-n{n}" for s, n in ROW_CASES])
def test_keyless_calls_on_rows_of_every_alignment(monkeypatch, name, n):
    import pk_encrypt_model as PM
    import rs_tfhe_amd as R

    for var in ("TFHE_HIP_KS_KERNEL", "TFHE_HIP_BR_KERNEL"):
        monkeypatch.delenv(var, raising=False)
    R_ = rows_of(n)
    eng = R.Engine(R_.pp, 0)
    try:
        if "pack" in name:
            eng.load_packing_key(_pack_key(R_)[0])
        if "pk_encrypt" in name:
            eng.load_public_key(R_.want("pk", lambda: PM.public_key(n, PK_SIZE)))
        ran = 0
        for count in COUNTS:
            for case in CALLS[name].cases(R_, count, "rows"):
                run_case(eng, case)
                ran += 1
        assert ran
    finally:
        eng.close()


@pytest.fixture(scope="module")
def engine():
    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    e = R.Engine(p, 0)  # no key: none of the packed calls needs the cloud key
    yield e
    e.close()


@pytest.mark.parametrize("name", _in("packed"), ids=lambda s: s[len("tfhe_hip_"):])
def test_calls_on_packed_ciphertexts(engine, name):
    counts = (1, 3) if "trgsw" in name else (1, 65)
    for count in counts:
        for case in CALLS[name].cases(None, count, "packed"):
            run_case(engine, case)


@pytest.mark.parametrize("name", sorted(DEMANDED), ids=lambda s: s[len("tfhe_hip_"):])
def test_alignment_refusals(engine, name):
    """The operands the header demands 16-byte aligned: framed at offset 0 the call computes the model's words whatever
    word the other operands start at; with every operand at word 1, 2 or 3, and with any ONE demanded operand a word
    off, it returns TFHE_HIP_EINVAL and touches nothing."""
    demanded = DEMANDED[name]
    aligned = {k: 0 for k in demanded}
    for count in (1, 65):
        for case in CALLS[name].cases(None, count, "aligned"):
            present = [k for k in demanded if k in case.inputs or k == "out" or (isinstance(case.out_like, dict) and k in case.out_like)]
            run_case(engine, case, DB.WORD_PLANS, at=aligned)
            for plan in DB.WORD_PLANS[1:4]:  # every operand at the same word 1 .. 3
                run_refused(engine, case, plan, None)
            for k in present:
                run_refused(engine, case, DB.PLANS[0], {k: 1})
                run_refused(engine, case, DB.PLANS[0], {k: 2})


# ---- smaller things -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect,said", [("past_end", "AFTER the end touched, the nearest 1 past"),
                                         ("before_start", "BEFORE the start touched, the nearest 1 before"),
                                         ("unwritten", "1 still hold the sentinel"), ("neighbour", "output words differ")])
def test_the_harness_catches_planted_defects_on_the_device(defect, said):
    """tests/test_dev_buffers_host.py's stand-in kernel and its four defects on frames that live on the GPU: what run_case
    does with a device frame (the copy back, the spans, the fills) tells a defect there too.  Plain torch operations
    inside the frame: nothing is written outside an allocation."""
    from test_dev_buffers_host import _operands, standin

    inputs, want = _operands()
    f = DB.Framed(inputs, want, DB.PLANS[4])
    assert f.out.is_cuda
    standin(f)
    f.check(want, "stand-in")
    f = DB.Framed(inputs, want, DB.PLANS[4])
    standin(f, defect)
    with pytest.raises(AssertionError, match=said):
        f.check(want, "stand-in")


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [64, 65])
def test_lincomb_out_may_alias(n, offset):
    """tfhe_hip_batch_tlwe_lincomb_dev: "out may alias a or b" -- out is a, out is b, a is b is out, against the model;
    the pads around the operands stay, and the operand that is not the output is unchanged."""
    import torch

    import rs_tfhe_amd as R

    count, (ca, cb, cc) = 17, (3, 0xFFFFFFFE, 0x40000000)
    rng = np.random.default_rng(n + offset)
    a, b = _words(rng, (count, n + 1)), _words(rng, (count, n + 1))
    eng = R.Engine(rows_of(n).pp, 0)
    try:
        for form, want in (("a", lincomb_model(ca, a, cb, b, cc)), ("b", lincomb_model(ca, a, cb, b, cc)),
                           ("ab", lincomb_model(ca, a, cb, a, cc))):
            (big_a, va), (big_b, vb) = DB.frame(a, offset), DB.frame(b, offset)
            if form == "ab":
                vb, big_b = va, big_a
            out = va if form in ("a", "ab") else vb
            eng.batch_tlwe_lincomb_dev(ca, va, cb, vb, cc, out)
            torch.cuda.synchronize()
            big_out = big_a if out is va else big_b
            sp = DB.span(big_out, out)
            assert np.array_equal(DB.view_words(big_out, sp).reshape(count, n + 1), want), form
            said = [DB.check_frame(big_a, DB.span(big_a, va), "poison", "a"), DB.check_frame(big_b, DB.span(big_b, vb), "poison", "b")]
            assert not any(said), (form, said)
            if form == "a":
                assert np.array_equal(DB.view_words(big_b, DB.span(big_b, vb)).reshape(count, n + 1), b)
            if form == "b":
                assert np.array_equal(DB.view_words(big_a, DB.span(big_a, va)).reshape(count, n + 1), a)
    finally:
        eng.close()


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_pinned_host_views_run_in_place(O, monkeypatch, offset):
    """The other way caller memory reaches the kernels: pinned operands of the host forms are read and written in place.
    One gate call and one bootstrap call on views `offset` words into pinned buffers, inputs between poison pads, the
    output (prefilled) between sentinel pads: the oracle's words, and nothing else touched."""
    from rs_tfhe_amd.engine import pinned_empty

    for var in ("TFHE_HIP_KS_KERNEL", "TFHE_HIP_BR_KERNEL"):
        monkeypatch.delenv(var, raising=False)
    n, count = 65, 17
    B = boot(O, n, *KS_BASES[0])
    eng = _boot_engine(B)

    def pinned(words, fill):
        size, start = words.size, DB.PAD + offset
        big = pinned_empty(DB.PAD + offset + size + DB.PAD)
        big[...] = DB.fill_pattern(len(big), fill, 4).view(np.uint32)
        if fill == "poison":
            big[start:start + size] = words.reshape(-1)
        return big, (start, size), C.c_void_p(big.ctypes.data + 4 * start)

    try:
        a, b = B.a[:count], B.b[:count]
        gate = B.want("gate", lambda: O.batch_gate(B.ck, O.GATE_XOR, B.a, B.b))[:count]
        boot_own = B.want("boot_own", lambda: O.batch_bootstrap(B.ck, B.a))[:count]  # the key's own test vector
        calls = (("gate", gate, lambda pa, pb, po: eng._lib.tfhe_hip_batch_gate(eng._ctx, O.GATE_XOR, pa, pb, po, count)),
                 ("bootstrap", boot_own, lambda pa, pb, po: eng._lib.tfhe_hip_batch_bootstrap(eng._ctx, pa, None, 0, 1, po, count)))
        for label, want, call in calls:
            (big_a, sa, pa), (big_b, sb, pb), (big_o, so, po) = pinned(a, "poison"), pinned(b, "poison"), pinned(gate, "sentinel")
            assert call(pa, pb, po) == 0, eng._lib.tfhe_hip_last_error(eng._ctx)
            assert np.array_equal(DB.view_words(big_o, so).reshape(count, n + 1), want), label
            said = [DB.check_frame(big_o, so, "sentinel", "output"), DB.check_frame(big_a, sa, "poison", "a"),
                    DB.check_frame(big_b, sb, "poison", "b")]
            assert not any(said), (label, said)
            assert np.array_equal(DB.view_words(big_a, sa), a.reshape(-1)) and np.array_equal(DB.view_words(big_b, sb), b.reshape(-1))
    finally:
        eng.close()
