"""Call sequences on one context (tfhe_hip_ctx and its key views): a seeded generator of sequences of calls, forms,
streams and state changes, an executor that issues them back to back with no synchronisation of its own, the model of
every step's words (the CPU oracle plus packing.pack_model / unpack_model / table_model), and the comparison.  The
axis under test is ORDER: what a call leaves behind on the context (scratch, scratch ownership, staging, key binding,
profiling events) and what the next call, on another stream or another key view, does to work still in flight.

A plain module (no tests in it; nothing it imports opens the device), like circuit_fuzz.py and lockstep.py.  The
executor talks to the device through a small backend (upload / empty / download / synchronize / pinned memory): `TorchBackend` on the GPU,
`FakeBackend` with the stand-in handles of test_sequence_fuzz_host.py.

Rows.  A step's rows are drawn with repetition from ROWS_PER_STEP rows of pools of at most POOL distinct ciphertexts,
so the oracle evaluates a handful of rows per step and EVERY row of every step is compared with the tiled result
(`Model._rowwise` finds the distinct rows again from the operands themselves, chained operands included, and memoises
by key, op signature and row bytes).  The generator asserts that a sequence costs at most MAX_ORACLE_BOOTSTRAPS.

Encryption, decryption and the linear layers.  These steps stage secrets in the context's one `sym_sec`, selectors
in `pke_sel`, lv1 rows in the bootstrap's scratch, or claim nothing at all, and each names the secret key of its own
handle.  Encrypting steps draw real noise (alpha of the set) under a generator key, a mask seed and a first index of
their own; the generator draws the key again while a sample of the step lies within 2^-20 of a torus step, where two
correct f64 implementations may round apart, so the comparison stays word for word.  Their models are the
term-by-term ones of sym_encrypt_model / packed_encrypt_model / pk_encrypt_model, client.SecretKey's phases and
decodes, and linear's definitions; the shapes are the table TABLE.  A step's count is its output ciphertexts (the
groups of encrypt_trlwe, whose plaintext words are args["words"]) or, for the decrypting steps, its output words.
Chains C (encrypt -> tlwe_matmul -> decrypt) and D (encrypt_trlwe -> polymul -> trlwe_matmul -> decrypt) run on one
handle and one stream like A and B.

The ring steps: the TRLWE key switch (`trlwe_keyswitch`, args {"k"}), the packed CMUX (`cmux`, args {"d0", "reference"},
a gadget and one selector a step) and TRGSW encryption (`encrypt_trgsw`, a bit times a monomial under real noise), all on
[.][2][N] words.  Each of E and V2 holds a switching key per k of SWITCH_KS whose gadgets differ between the views
(SWITCH_START), so a call that read the other view's table gives other words; `switch_key_change` replaces one by a key
of another (basebit, t) from a pre-made book, by generation under the book's generator key (the same words expected), by
a load, or by a drop and a load, and drains nothing itself: the library's device-wide drain is under test.  `ring_times`
asks tfhe_hip_get_trlwe_switch_times / _cmux_times for the chunk passes issued while profiling was on (ring_passes reads
them off the sequence).  The ring items of the generator (switch_change, trgsw_pair, ring_mix, ring_grow, cm_t_grow)
place these calls in the orders ring_orders() names: under a running key switch and the reverse, the two families on two
streams, the same k on the two views, a digit scratch that grows through t alone (the first (1, 32) key or selector of a
sequence, at the family's largest count so far, under a running call of that family), RING_BIG = 2,049 ciphertexts (a
second chunk pass) at twice any earlier ring count, a key change under a running switch of the same k on the other view
(and one of the changed view itself), TRGSW encryption as the second call of a secret pair.  Chains E (encrypt_trlwe ->
trlwe_keyswitch k = 3 -> decrypt_trlwe) and F (encrypt_trgsw -> cmux on genuine encryptions -> trlwe_keyswitch k = 2047 ->
decrypt_trlwe) end in plaintext (chains_decrypt_to_their_plaintext_products).  Their models are trlwe_switch_model and
cmux_model as they stand, through Model._rowwise; these cost 37 ms per key row per evaluation whatever the count, so the
ring steps of a sequence share the three rows of the "ring" pool and one selector per gadget (a row seen under a key
costs nothing again), the ring variants are dealt in turn by the ring items and not by the deck, and t = 32 is kept to
what the orders need: the (1, 32) key of a sequence's first switch_key_change and the (1, 32) selector of cm_t_grow (the
deck of CMUX gadgets is (6, 3), (4, 6)); a ring count is one of RING_COUNTS or RING_BIG; a step that needs a row of the
"ring" pool under a key or selector evaluates the pool's other rows with it, so a sequence pays for a key's matrices once.
STEPS is 102 against 66 before these steps: the ring items and chains E and F take 36 steps of a sequence, and the deck
keeps its 32 draws -- six sequences deal each of the 64 variants of the deck three times, which the corpus condition wants.
What the ring orders leave uncovered: the six sequences of a shape run on one context whose scratch never shrinks, and a
ring family's digit scratch cannot grow from seed to seed as the grow step does (1.5 x the seed before): it is capped at
RING_CHUNK ciphertexts of the largest t, 2,048 x 36 N bytes of ts_dig and 2,048 x 64 N of cm_dig.  So ts_dig and cm_dig are
reallocated under running calls in the first sequences of a shape only, until a count above RING_CHUNK has met t = 32 (on
SECURITY_128_BIT cm_dig is at its largest from seed 1 on and ts_dig from seed 2 on, on SECURITY_UINT4 from seeds 0 and
1); the "grown through t alone" and ring grow steps of the later sequences find the scratch large enough and hold the
ORDER of calls only (the claim, the stream waits), not a reallocation.
The directed pair of test_gpu_sequence_fuzz.py for these calls (a host switch on V2 under an un-synchronised
trlwe_keyswitch_dev of the same k on E) measured 16,384 ciphertexts at 2.31 ms alone against 0.09 ms to issue, the first
call still running in all four rounds when the second was entered.

What is narrower than the full cross product: TRGSW encryption's device form has no stream argument (it runs on the
context's own and has finished on return, so what is chained from it may run on any stream); VR runs no ring step and
holds no switching key; switching keys keep s_from = s_to = the handle's own ring key, so that a chain decrypts; the
pinned form (every operand and the output from pinned_empty, the
zero-copy path of host_call) exists for `gate` only -- the one host method of Engine that takes `out=`; the stage ops
(identity_key_switch, sample_extract, external_product) exist as host forms only; `reencrypt` runs on VR only and VR
runs nothing else; a key change on V2 first drains the streams that still carry V2's own work (the header makes a key
change under in-flight calls of the SAME key the caller's job), never the work of the sibling views."""
import hashlib
import time

import numpy as np

N = 1024
M32 = 0xFFFFFFFF
POOL = 24  # distinct ciphertexts per (sequence, key)
ROWS_PER_STEP = 3  # distinct rows of one step
MAX_ORACLE_BOOTSTRAPS = 400
FILL = 0x5A5A5A5A  # what a device output holds before its step runs

BASE_COUNTS = (1, 2, 5, 33, 64, 65, 300, 520, 1300)
HANDLES = ("E", "V2", "VR")
FORMS = ("host", "pinned", "dev0", "dev1", "dev2")  # dev0: torch's default stream; dev1 / dev2: side streams
ROUTES = ("load", "compressed", "gen")
STAGE_OPS = ("identity_key_switch", "sample_extract", "external_product")
STATE_OPS = ("profiling_on", "profiling_off", "kernel_times", "combining_off", "combining_default", "synchronize",
             "load_packing_key", "key_change", "switch_key_change", "ring_times")
COEFS = (1, 2, 3, M32, M32 - 1)
ENC_OUTS = ("full", "bodies", "both")
DECRYPT_MODES = ("phase", "bool", "message")
MESSAGE_MODULUS = 16
# the calls that stage a secret in ctx->sym_sec
SECRET_OPS = ("encrypt", "encrypt_trlwe", "decrypt", "decrypt_trlwe", "encrypt_trgsw")
RING_OPS = ("trlwe_keyswitch", "cmux")  # the calls whose digit scratch (ts_dig, cm_dig) is the context's
RING_CHUNK = 2048  # kTsChunk = kCmuxChunk: ciphertexts of one pass through the digit scratch
RING_COUNTS = (1, 2, 5, 33, 64, 65, 300, 520)  # what a ring step draws from, besides ...
RING_BIG = 2049  # ... one ciphertext into a second chunk pass
SWITCH_KS = (1, 3, 2047)  # the automorphisms each of E and V2 holds a switching key for
SWITCH_ROUTES = ("gen", "load", "drop_load")
# (basebit, t) of the key each view starts with, per k: never the same on the two views
SWITCH_START = {"E": {1: (4, 6), 3: (7, 4), 2047: (2, 16)}, "V2": {1: (2, 16), 3: (4, 6), 2047: (7, 3)}}
CMUX_GADGETS = ((6, 3), (4, 6), (1, 32))
TRGSW_GADGETS = ((6, 3), (1, 32))
GEN_POOL = 4  # genuine packed encryptions of known words per handle (chain F's d0 / d1)
UNCLAIMED_OPS = ("tlwe_matmul", "conv2d", "polymul", "expand_seeded_trlwe")  # no context scratch, no claim
HIGH_FIRST = (1 << 33) - 1  # a first index above 2^32 whose second row (or group) carries out of the low nonce word
PK_SIZE = 48  # the public keys: the "whole blocks" shape of sym_encrypt_model.SHAPES
PK_GEN_KEY = bytes((29 * i + 5) & 0xFF for i in range(32))  # their generator key
# (rows, cols, groups), the smallest that reach each code path: a row tail, a K tail, weight rows off 16-byte boundaries,
# a column tail at n + 1
TABLE = {
    "tlwe_matmul": ((1, 1, 1), (33, 31, 2), (65, 100, 3)),
    "trlwe_matmul": ((33, 1, 2), (7, 1023, 1), (40, 1024, 3)),
    "polymul": ((1, 1, 1), (2, 3, 2)),
    # (in_h, in_w, in_c, k, out_c, stride, padding, groups): in_c % 16 != 0 is the tap-walking loader; the other the
    # one-tap loader, with padding taps
    "conv2d": ((5, 4, 3, 3, 5, (1, 1), (1, 1), 2), (4, 4, 16, 3, 33, (2, 1), (1, 0), 1)),
}
CHAIN_D_MATMUL = (7, 1023, 4)  # chain D: the four TRLWEs of polymul (2, 3, 2) as four groups


class Shape:
    """A parameter shape of the fuzz: its name, n, the counts, whether the oracle gives words (`exact`), and whether
    the tree bootstrap runs (UINT4 only), and the noise parameters of the set."""

    def __init__(self, name, n, counts, exact, bivariate, alpha_lv0, alpha_lv1):
        self.name, self.n, self.counts, self.exact, self.bivariate = name, n, tuple(counts), exact, bivariate
        self.alpha_lv0, self.alpha_lv1 = alpha_lv0, alpha_lv1  # of the parameter set: what the encrypting steps draw

    def __repr__(self):
        return f"Shape({self.name})"


SHAPES = {
    "SECURITY_128_BIT": Shape("SECURITY_128_BIT", 700, BASE_COUNTS, True, False, 2.0e-5, 2.0e-8),
    # l = 1, general rounding, base 32: the column-sliced key switch from ks_sl_chunk_min = 384 rows on
    "SECURITY_UINT4": Shape("SECURITY_UINT4", 820, BASE_COUNTS + (383, 384, 400), False, True, 0.0000025167616095979554,
                            2.220446049250313e-16),
}
STEPS = 102
SEEDS = {"SECURITY_128_BIT": (0, 1, 2, 3, 4, 5), "SECURITY_UINT4": (0, 1, 2, 3, 4, 5)}


def variants(shape):
    """Every (op, fixed arguments) the generator deals out, in a fixed order."""
    v = [("gate", {"code": c}) for c in range(11)]
    v += [("gates_mixed", {"ks": True}), ("gates_mixed", {"ks": False})]
    v += [("bootstrap", {"tv": tv, "ks": ks}) for tv in (None, "one", "per") for ks in (True, False)]
    v += [("tlwe_lincomb", {}), ("lincomb_bootstrap", {})]
    v += [("lincomb_bootstrap_many", {"k": k}) for k in (2, 4, 8)]
    v += [("mux", {"naive": False}), ("mux", {"naive": True}), ("blind_rotate", {})]
    v += [(op, {}) for op in STAGE_OPS]
    v += [("pack", {}), ("unpack", {"slots": False}), ("unpack", {"slots": True}), ("pack_table", {"m": 4})]
    if shape.bivariate:
        v += [("bootstrap_bivariate", {"m": 4, "k": 1}), ("bootstrap_bivariate", {"m": 4, "k": 4})]
    v += [("reencrypt", {}), ("expand_seeded", {})]
    v += [("encrypt", {"out": o}) for o in ENC_OUTS] + [("encrypt_trlwe", {"out": o}) for o in ENC_OUTS]
    v += [("expand_seeded_trlwe", {}), ("pk_encrypt", {})]
    v += [("decrypt", {"mode": m, "width": w}) for m in DECRYPT_MODES for w in ("lv0", "lv1")]
    v += [("decrypt_trlwe", {"mode": m}) for m in DECRYPT_MODES]
    v += [("tlwe_matmul", {"bias": b}) for b in (True, False)] + [("trlwe_matmul", {"ks": k}) for k in (True, False)]
    v += [("polymul", {"bias": b}) for b in (True, False)] + [("conv2d", {"case": c}) for c in range(len(TABLE["conv2d"]))]
    return v + ring_variants()


def ring_variants():
    """The TRLWE key switch, the packed CMUX and TRGSW encryption: dealt in turn by the ring items of the generator
    (every one of them sits in an order that names its neighbours), not by the deck."""
    v = [("trlwe_keyswitch", {"k": k}) for k in SWITCH_KS]
    v += [("cmux", {"d0": d0, "reference": ref}) for d0 in (True, False) for ref in (False, True)]
    return v + [("encrypt_trgsw", {"gadget": g}) for g in TRGSW_GADGETS]


def switch_key_name(handle, k, gadget):
    return f"{handle}:{k}:{gadget[0]}x{gadget[1]}"


def switch_gadgets(handle, k):
    """The gadgets of the switching keys made for (handle, k): the one the view starts with, then the two a
    switch_key_change brings in turn -- (1, 32) first: the largest digit scratch a count can ask for."""
    start = SWITCH_START[handle][k]
    return (start,) + tuple(g for g in ((1, 32), (7, 3), (4, 6)) if g != start)[:2]


def switch_key_gadget(name):
    basebit, t = name.rsplit(":", 1)[1].split("x")
    return int(basebit), int(t)


def switch_book_names():
    return [switch_key_name(h, k, g) for h in ("E", "V2") for k in SWITCH_KS for g in switch_gadgets(h, k)]


def switch_gen_key(name):
    """The generator key a switching key of the book is made under."""
    return hashlib.blake2b(b"switching key " + name.encode(), digest_size=32).digest()


def ring_scratch_bytes(op, t, count):
    """ts_dig / cm_dig of one call: chunk (t N + 4 N) digits and bodies, chunk 2t N digits."""
    chunk = min(count, RING_CHUNK)
    return chunk * (t * N + 4 * N) if op == "trlwe_keyswitch" else chunk * 2 * t * N


def variant_name(op, args):
    """The name the corpus condition counts an op under."""
    if op == "gate":
        return f"gate:{args['code']}"
    if op == "gates_mixed":
        return "gates_mixed" if args["ks"] else "gates_mixed_nks"
    if op == "bootstrap":
        return f"bootstrap:{args['tv']}:{'ks' if args['ks'] else 'nks'}"
    if op == "lincomb_bootstrap_many":
        return f"many:{args['k']}"
    if op == "mux":
        return "mux_naive" if args["naive"] else "mux"
    if op == "unpack":
        return "unpack_slots" if args["slots"] else "unpack"
    if op == "bootstrap_bivariate":
        return f"bivariate:{args['k']}"
    if op in ("encrypt", "encrypt_trlwe"):
        return f"{op}:{args['out']}"
    if op == "decrypt":
        return f"decrypt:{args['mode']}:{args['width']}"
    if op == "decrypt_trlwe":
        return f"decrypt_trlwe:{args['mode']}"
    if op in ("tlwe_matmul", "polymul"):
        return op + ":bias" if args["bias"] else op
    if op == "trlwe_matmul":
        return "trlwe_matmul:ks" if args["ks"] else "trlwe_matmul:nks"
    if op == "conv2d":
        return f"conv2d:{args['case']}"
    if op == "trlwe_keyswitch":
        return f"trlwe_keyswitch:{args['k']}"
    if op == "cmux":
        return ("cmux" if args["d0"] else "external_product_sel") + (":reference" if args["reference"] else "")
    if op == "encrypt_trgsw":
        return f"encrypt_trgsw:{args['gadget'][0]}x{args['gadget'][1]}"
    return op


def forms_of(op):
    if op in STAGE_OPS:
        return ("host",)
    if op == "encrypt_trgsw":  # its device form has no stream argument: it runs on the context's own and drains it
        return ("host", "dev0")
    if op == "gate":
        return FORMS
    return ("host", "dev0", "dev1", "dev2")


class Step:
    """One step.  kind "call": `op` on `handle` in `form` over `count` ciphertexts with operands `ins` (specs, see
    `materialise`) and scalar arguments `args`; kind "state": `op` of STATE_OPS on `handle`."""

    def __init__(self, kind, handle, op, form=None, count=0, ins=(), args=None):
        self.i = -1
        self.kind, self.handle, self.op, self.form, self.count = kind, handle, op, form, count
        self.ins, self.args = list(ins), dict(args or {})

    @property
    def dev(self):
        return self.kind == "call" and self.form.startswith("dev")

    @property
    def queued(self):
        """A _dev step whose work may still run when the next step is entered (TRGSW encryption's device form has
        finished on return)."""
        return self.dev and self.op != "encrypt_trgsw"

    @property
    def ring(self):
        return self.kind == "call" and self.op in RING_OPS

    @property
    def passes(self):
        """Chunk passes of a ring step through its digit scratch."""
        return -(-self.count // RING_CHUNK) if self.ring else 0

    @property
    def stream(self):
        return int(self.form[3:]) if self.dev else None

    @property
    def sources(self):
        return [s[1] for s in self.ins if s is not None and s[0] == "out"]

    @property
    def ks_rows(self):
        """Rows of the step's largest key switch (0: none)."""
        a, c = self.args, self.count
        if self.kind != "call":
            return 0
        if self.op in ("gate", "mux", "unpack", "reencrypt", "identity_key_switch"):
            return c
        if self.op in ("gates_mixed", "bootstrap", "lincomb_bootstrap"):
            return c if a["ks"] else 0
        if self.op == "lincomb_bootstrap_many":
            return c * a["k"] if a["ks"] else 0
        if self.op == "bootstrap_bivariate":
            return c * a["k"]  # the many-LUT stage; the last bootstrap's is `c` (with ks)
        if self.op == "trlwe_matmul":
            return c if a["ks"] else 0  # groups x rows
        return 0

    @property
    def claims(self):
        """Whether the call takes the context's scratch (claim_scratch): a key switch, a blind rotation, a staged secret,
        the selectors of pk_encrypt, the packing and unpacking key switches."""
        return self.kind == "call" and (self.ks_rows > 0 or self.oracle_bootstraps > 0 or
                                        self.op in SECRET_OPS + RING_OPS + ("pk_encrypt", "pack", "pack_table", "unpack", "bootstrap_bivariate"))

    @property
    def oracle_bootstraps(self):
        """Blind rotations the oracle runs for ONE distinct row of this step."""
        if self.kind != "call":
            return 0
        return {"gate": 1, "gates_mixed": 1, "bootstrap": 1, "lincomb_bootstrap": 1, "lincomb_bootstrap_many": 1, "mux": 3,
                "blind_rotate": 1}.get(self.op, 0)

    def key(self):
        def norm(x):
            if isinstance(x, np.ndarray):
                return (x.dtype.str, x.shape, x.tobytes())
            if isinstance(x, (tuple, list)):
                return tuple(norm(y) for y in x)
            return x

        return (self.i, self.kind, self.handle, self.op, self.form, self.count, norm(self.ins), norm(sorted(self.args.items())))

    def __repr__(self):
        if self.kind == "state":
            return f"<{self.i} {self.handle}.{self.op} {self.args if self.op in ('key_change', 'switch_key_change') else ''}>"
        return f"<{self.i} {self.handle}.{variant_name(self.op, self.args)} {self.form} x{self.count} from {self.sources}>"


# ---- the generator ----------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, seed, shape, steps):
        self.seed, self.shape, self.steps = seed, shape, steps
        self.rng = np.random.default_rng([0x5E9F, seed, shape.n])
        self.seq = []
        self.changes = 0
        self.v2_pending = set()  # streams that carry V2 work no step has drained yet
        self.dealt = {}  # shape-table op -> how many of its steps were dealt
        self.switch = {h: dict(SWITCH_START[h]) for h in SWITCH_START}  # the gadget of the key each view holds per k
        self.ring_max = {op: 0 for op in RING_OPS}  # the largest count of each ring family so far

    # -- operands
    def _sel(self, count):
        d = min(count, ROWS_PER_STEP)
        sel = self.rng.integers(0, d, count)
        sel[:d] = np.arange(d)
        return sel

    def _rows(self, pool, sel, size=POOL):
        pick = self.rng.choice(size, int(sel.max()) + 1, replace=False)
        return ("rows", pool, pick[sel])

    def _u32(self, sel, hi=1 << 32):
        vals = self.rng.integers(0, hi, int(sel.max()) + 1, dtype=np.uint64)
        return vals[sel]

    def _table(self, kind, sel):
        if kind is None:
            return None
        return self._rows("tv", sel, 8) if kind == "per" else ("rows", "tv", np.array([self.rng.integers(0, 8)]))

    def add(self, st):
        st.i = len(self.seq)
        self.seq.append(st)
        if st.handle == "V2" and st.dev:
            self.v2_pending.add(st.stream)
        if st.ring:
            self.ring_max[st.op] = max(self.ring_max[st.op], st.count)
        return st

    def call(self, handle, op, args, form, count, src=None):
        """A call step with fresh operands (operand 0 chained from step `src` when given)."""
        args = dict(args)
        lv0 = f"lv0:{handle}"
        sel = self._sel(count)
        first = ("out", src) if src is not None else self._rows(lv0, sel)
        if op == "gate":
            ins = [first, self._rows(lv0, sel)]
        elif op == "gates_mixed":
            ins = [("u8", self._u32(sel, 11).astype(np.uint8)), first, self._rows(lv0, sel)]
        elif op == "bootstrap":
            ins = [first, self._table(args["tv"], sel)]
        elif op in ("tlwe_lincomb", "lincomb_bootstrap", "lincomb_bootstrap_many"):
            args.update(ca=int(self.rng.choice(COEFS)), cb=int(self.rng.choice(COEFS)), cc=int(self.rng.integers(0, 1 << 32)))
            ins = [first, self._rows(lv0, sel)]
            if op == "lincomb_bootstrap":
                args.update(tv=(None, "one", "per")[int(self.rng.integers(0, 3))], ks=bool(self.rng.integers(0, 2)))
                ins.append(self._table(args["tv"], sel))
            elif op == "lincomb_bootstrap_many":
                args.update(ks=bool(self.rng.integers(0, 4)))
                ins.append(self._table("one", sel))
        elif op == "mux":
            ins = [first, self._rows(lv0, sel), self._rows(lv0, sel)]
        elif op == "blind_rotate":
            args.update(tv=(None, "one")[int(self.rng.integers(0, 2))])
            ins = [first, self._table(args["tv"], sel)]
        elif op == "identity_key_switch":
            ins = [self._rows("lv1", sel)]
        elif op == "sample_extract":
            args.update(k=int(self.rng.integers(0, N)))
            ins = [self._rows("trlwe", sel, 8)]
        elif op == "external_product":
            ins = [self._rows("trlwe", sel, 8), ("i32", self._u32(sel, self.shape.n).astype(np.int32))]
        elif op == "pack":
            ins = [first]
        elif op == "unpack":
            groups = -(-count // N) if not args["slots"] else 2
            trlwe = ("out", src) if src is not None else ("rows", "trlwe", self.rng.choice(8, groups, replace=False))
            slots = ("u32", self._u32(sel, groups * N).astype(np.uint32)) if args["slots"] else None
            ins = [trlwe, slots]
        elif op == "pack_table":
            s1 = self._sel(args["m"] * count)
            ins = [self._rows(lv0, s1)]
        elif op == "bootstrap_bivariate":
            args.update(ks=bool(self.rng.integers(0, 4)))
            ins = [first, self._rows(lv0, sel), ("rows", "tv", self.rng.choice(8, args["m"] // args["k"], replace=False))]
        elif op == "reencrypt":
            ins = [first]
        elif op == "expand_seeded":
            args.update(seed=self.rng.integers(0, 256, 32).astype(np.uint8).tobytes(), first=int(self.rng.integers(0, 1 << 40)))
            ins = [("u32", self._u32(sel).astype(np.uint32))]
        elif op in ("encrypt", "pk_encrypt"):
            if op == "pk_encrypt" and count > 520:
                count = self.pick_count(at_most=520)
                sel = self._sel(count)
            self._encrypting(op, args, count, self.shape.alpha_lv0)
            ins = [("u32", self._u32(sel).astype(np.uint32))]
        elif op == "encrypt_trlwe":  # `count` plaintext words; the step's count is its groups
            args["words"] = count
            count = -(-count // N)
            self._encrypting(op, args, count, self.shape.alpha_lv1)
            ins = [("u32", self._u32(self._sel(args["words"])).astype(np.uint32))]
        elif op == "expand_seeded_trlwe":
            count = 1 + int(self.rng.integers(0, 2))
            args.update(seed=self._bytes32(), first=self._first())
            ins = [("u32", words(self.rng, (count, N)))]
        elif op == "decrypt":
            ins = [first if src is not None or args["width"] == "lv0" else self._rows("lv1", sel)]
        elif op == "trlwe_keyswitch":
            # (the ring steps of a sequence share the ROWS_PER_STEP rows of the "ring" pool, in any order and tiling: the
            # numpy models cost 37 ms per key row whatever the count, and a row already seen under a key costs nothing)
            ins = [first if src is not None else self._rows("ring", sel, ROWS_PER_STEP)]
        elif op == "cmux":
            if "gadget" not in args:  # in turn; (1, 32) -- 2.4 s of model a step -- is the step that grows cm_dig through t
                args["gadget"] = CMUX_GADGETS[(self.seed + self.dealt.get(op, 0)) % 2]
                self.dealt[op] = self.dealt.get(op, 0) + 1
            t = args["gadget"][1]
            # one selector a step: the [2t][2][N] random words of its gadget (the operation is exact on any words), or the
            # first selector a TRGSW encryption returned
            sel_in = ("out", src) if src is not None else ("rows", f"sel:{t}", np.array([0]))
            pool, size = args.pop("pool", ("ring", ROWS_PER_STEP))
            d1 = self._rows(pool, sel, size)
            ins = [sel_in, ("rows", pool, (d1[2] + 1) % size) if args["d0"] else None, d1]
        elif op == "encrypt_trgsw":  # mu: a bit times a monomial
            args.setdefault("mu", [(int(b), int(j)) for b, j in zip(self.rng.integers(0, 2, count), self.rng.integers(0, N, count))])
            mu = np.zeros((count, N), np.int32)
            for m, (b, j) in enumerate(args["mu"]):
                mu[m, j] = b
            args["mu"] = tuple(args["mu"])
            self._encrypting(op, args, count, self.shape.alpha_lv1)
            ins = [("i32", mu)]
        elif op == "decrypt_trlwe" and src is not None:  # the last link of chains E and F: every slot of the groups
            ins = [first]
        elif op == "decrypt_trlwe":
            groups = 1 + int(self.rng.integers(0, 2))  # one group, or a second one partly read; below the largest count
            count = (groups - 1) * N + 1 + int(self.rng.integers(0, (N if groups == 1 else max(self.shape.counts) - N) - 1))
            ins = [("rows", "trlwe", self.rng.integers(0, 8, groups))]
        elif op in TABLE:
            if op == "conv2d":
                args["shape"] = TABLE[op][args["case"]]
            elif "shape" not in args:  # each shape of the table in turn
                args["shape"] = TABLE[op][(self.seed + self.dealt.get(op, 0)) % len(TABLE[op])]
                self.dealt[op] = self.dealt.get(op, 0) + 1
            if op == "conv2d":
                in_h, in_w, in_c, k, out_c, stride, pad, groups = args["shape"]
                args["bias"] = bool(self.rng.integers(0, 2))
                out_h, out_w = (in_h + 2 * pad[0] - k) // stride[0] + 1, (in_w + 2 * pad[1] - k) // stride[1] + 1
                wshape, n_in, n_bias, count = (out_c, k, k, in_c), groups * in_h * in_w * in_c, out_c, groups * out_h * out_w * out_c
                pool, size = lv0, POOL
            else:
                rows, cols, groups = args["shape"]
                if op == "trlwe_matmul":
                    args.setdefault("bias", bool(self.rng.integers(0, 2)))
                wshape, n_bias, count = (rows, cols), rows, groups * rows
                pool, size, n_in = (lv0, POOL, groups * cols) if op == "tlwe_matmul" else ("trlwe", 8, groups)
                if op == "polymul":
                    wshape, n_bias, n_in = (rows, cols, N), (rows, N), groups * cols
            w = self.rng.integers(-128, 128, wshape).astype(np.int8)  # -128 and 127 occur (one of them in a single weight)
            w.reshape(-1)[0] = -128
            w.reshape(-1)[-1] = 127
            operand = ("out", src) if src is not None else ("rows", pool, self.rng.integers(0, size, n_in))
            ins = [("i8", w), operand, ("u32", words(self.rng, n_bias)) if args["bias"] else None]
        else:
            raise ValueError(op)
        return self.add(Step("call", handle, op, form, count, ins, args))

    def _bytes32(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8).tobytes()

    def _first(self):
        """first_index / first_group: small, or above 2^32"""
        return int(self.rng.integers(0, 1000)) if self.rng.integers(0, 2) else HIGH_FIRST - int(self.rng.integers(0, 2))

    def _encrypting(self, op, args, count, alpha):
        """The keys and indices of an encrypting step.  Its noise is real (alpha of the set); a sample within 2^-20 of a
        torus step may round apart in two correct f64 implementations, so the generator key is drawn again until the
        step has none (about one 1300-row step in 400 needs a second draw)."""
        args.update(alpha=alpha, first=self._first())
        if op not in ("pk_encrypt", "encrypt_trgsw"):  # (those derive their public seed from the generator key)
            args["mask_seed"] = self._bytes32()
        for _ in range(4):
            args["rng_key"] = self._bytes32()
            if not encrypt_border(op, args["rng_key"], args["first"], count, alpha, args.get("gadget")).any():
                return
        raise AssertionError(("four generator keys with a borderline sample", self.seed, op, count))

    def pick_handle(self, op):
        if op == "reencrypt":
            return "VR"
        last = self.seq[-1].handle if self.seq else "V2"
        # the other of E / V2 two times in three: steps on V2 directly after steps on the engine, and the reverse
        other = {"E": "V2", "V2": "E"}.get(last, "E")
        return other if self.rng.integers(0, 3) else {"E": "V2", "V2": "E"}[other]

    def pick_form(self, op):
        forms = forms_of(op)
        prev = self.seq[-1] if self.seq else None
        if prev is not None and prev.dev and len(forms) > 1 and self.rng.integers(0, 2):
            # after a _dev step: the host form, or another stream, half of the time each
            if self.rng.integers(0, 2):
                return "host"
            return f"dev{(prev.stream + 1 + int(self.rng.integers(0, 2))) % 3}"
        return forms[int(self.rng.integers(0, len(forms)))]

    def pick_count(self, at_most=None):
        cs = [c for c in self.shape.counts if at_most is None or c <= at_most]
        return int(cs[int(self.rng.integers(0, len(cs)))])

    def dev_before(self, min_ks_rows=0):
        """Make the last step a _dev step (with a key switch of at least `min_ks_rows` rows, when asked)."""
        prev = self.seq[-1] if self.seq else None
        if prev is not None and prev.queued and (not min_ks_rows or prev.ks_rows >= min_ks_rows):
            return prev
        count = self.pick_count()
        while count < min_ks_rows:
            count = self.pick_count()
        handle = self.pick_handle("gate")
        code = int(self.rng.integers(0, 11))
        return self.call(handle, "gate", {"code": code}, f"dev{int(self.rng.integers(0, 3))}", count)

    def state(self, op):
        self.dev_before()
        handle = "V2" if op in ("key_change", "load_packing_key") and self.rng.integers(0, 2) or op == "key_change" else "E"
        args = {}
        if op == "key_change":
            args = {"route": ROUTES[(self.seed + self.changes) % 3], "target": ("K3", "K2")[self.changes % 2],
                    "wait": tuple(sorted(self.v2_pending))}
            self.changes += 1
            self.v2_pending = set()
        self.add(Step("state", handle, op, args=args))
        if op == "key_change":  # the public key sits beside the cloud key: a key change leaves it in place
            self.call("V2", "pk_encrypt", {}, ("host", "dev0", "dev1", "dev2")[int(self.rng.integers(0, 4))], self.pick_count(at_most=520))

    def grow(self):
        """A call of at least twice any earlier count, directly after un-synchronised device work."""
        self.dev_before()
        # 1.5 x the grow step of the seed before (ensure() keeps a quarter of headroom): a context that runs the corpus
        # seed after seed reallocates at every grow step, not only at the first
        # (twice the ring steps' largest count too: a step's count is whatever it has most of)
        count = max(2 * max(s.count for s in self.seq), int(np.ceil(2 * max(self.shape.counts + (RING_BIG,)) * 1.5 ** self.seed)))
        op, args, form = [("gate", {"code": 0}, "dev1"), ("gate", {"code": 3}, "host"), ("bootstrap", {"tv": None, "ks": True}, "dev2"),
                          ("identity_key_switch", {}, "host"), ("lincomb_bootstrap_many", {"k": 2}, "dev0")][self.seed % 5]
        st = self.call(self.pick_handle(op), op, args, form, count)
        st.args["grow"] = True

    def pair(self):
        """The pair of the scratch-claim finding: a _dev step whose key switch runs on >= 520 rows, then at once a host
        identity_key_switch of 384 rows or more (on a base >= 16 set both take the column-sliced kernel, whose digit
        scratch is the context's), no larger than the first."""
        prev = self.dev_before(min_ks_rows=520)
        cs = [c for c in self.shape.counts if 384 <= c <= min(prev.ks_rows, 520)]
        self.call(self.pick_handle("identity_key_switch"), "identity_key_switch", {}, "host", int(cs[int(self.rng.integers(0, len(cs)))]))

    def chain(self, which):
        handle = self.pick_handle("gate")
        stream = f"dev{int(self.rng.integers(0, 3))}"
        count = self.pick_count()
        if which == "A":  # gate_dev -> pack_dev -> unpack_dev
            links = [("gate", {"code": int(self.rng.integers(0, 11))}), ("pack", {}), ("unpack", {"slots": False})]
        elif which == "B":  # lincomb_dev -> bootstrap_dev
            links = [("tlwe_lincomb", {}), ("bootstrap", {"tv": "one", "ks": True})]
        elif which == "C":  # encrypt_dev -> tlwe_matmul_dev (the first 62 of 65 rows as two groups) -> decrypt_dev
            links = [("encrypt", {"out": "full"}, 65), ("tlwe_matmul", {"bias": True, "shape": TABLE["tlwe_matmul"][1]}),
                     ("decrypt", {"mode": "phase", "width": "lv0"}, 2 * 33)]
        elif which == "D":  # encrypt_trlwe_dev (six groups) -> polymul_dev -> trlwe_matmul_dev (no key switch) -> decrypt_dev
            links = [("encrypt_trlwe", {"out": "full"}, 5 * N + 300), ("polymul", {"bias": True, "shape": TABLE["polymul"][1]}),
                     ("trlwe_matmul", {"ks": False, "bias": True, "shape": CHAIN_D_MATMUL}),
                     ("decrypt", {"mode": "phase", "width": "lv1"}, 4 * 7)]
        elif which == "E":  # encrypt_trlwe_dev (two groups) -> trlwe_keyswitch_dev (k = 3) -> decrypt_trlwe_dev
            links = [("encrypt_trlwe", {"out": "full"}, N + 300), ("trlwe_keyswitch", {"k": 3}, 2),
                     ("decrypt_trlwe", {"mode": "phase"}, 2 * N)]
        else:  # F: encrypt_trgsw_dev (a bit) -> cmux_dev (genuine d0, d1) -> trlwe_keyswitch_dev (k = 2047) -> decrypt_trlwe_dev
            links = [("encrypt_trgsw", {"gadget": TRGSW_GADGETS[0], "mu": [(int(self.rng.integers(0, 2)), 0)]}, 1),
                     ("cmux", {"d0": True, "reference": False, "gadget": TRGSW_GADGETS[0], "pool": ("gen:" + handle, GEN_POOL)}, 2),
                     ("trlwe_keyswitch", {"k": 2047}, 2), ("decrypt_trlwe", {"mode": "phase"}, 2 * N)]
        src = None
        for op, args, *own in links:
            # (TRGSW encryption's device form names no stream: it runs on the context's own and has finished on return)
            st = self.call(handle, op, args, "dev0" if op == "encrypt_trgsw" else stream, own[0] if own else count, src)
            st.args["chain"] = which
            src = st.i
            yield

    def other_stream(self, *not_these):
        free = [k for k in range(3) if k not in not_these]
        return int(free[int(self.rng.integers(0, len(free)))])

    def secret_pair(self, k):
        """A secret-staging _dev call, then at once a secret-staging call on the other of E / V2 (another key in the same
        ctx->sym_sec), by its host form or on another stream.  The twelve pairs of a shape go through the four ordered
        kinds of {encrypting, decrypting} three times."""
        q = 2 * self.seed + k
        kinds = [("enc", "enc"), ("enc", "dec"), ("dec", "enc"), ("dec", "dec")][q % 4]
        first_on = ("E", "V2")[(q // 4 + q) % 2]
        prev = None
        for j, kind in enumerate(kinds):
            pick = [v for v in variants(self.shape) if v[0] in SECRET_OPS[:4] and v[0].startswith(kind)]
            op, args = pick[int(self.rng.integers(0, len(pick)))]
            if j == 0:
                form, handle = f"dev{int(self.rng.integers(0, 3))}", first_on
            else:
                form = "host" if (q // 2) % 2 else f"dev{self.other_stream(prev.stream)}"
                handle = {"E": "V2", "V2": "E"}[first_on]
            prev = self.call(handle, op, args, form, self.pick_count())

    def sandwich(self):
        """A call that claims nothing, on a stream of its own between two claiming _dev calls on other streams."""
        prev = self.dev_before(min_ks_rows=1)
        pick = [v for v in variants(self.shape) if v[0] in UNCLAIMED_OPS]
        op, args = pick[int(self.rng.integers(0, len(pick)))]
        mid = self.call(self.pick_handle(op), op, args, f"dev{self.other_stream(prev.stream)}", self.pick_count())
        self.call(self.pick_handle("gate"), "gate", {"code": int(self.rng.integers(0, 11))}, f"dev{self.other_stream(mid.stream)}",
                  self.pick_count())

    def ks_matmul(self):
        """trlwe_matmul with its key switch (the lv1 scratch of every bootstrap, then launch_key_switch) entered under a
        running key switch, and a key switch entered while it runs."""
        prev = self.dev_before(min_ks_rows=1)
        mm = self.call(self.pick_handle("gate"), "trlwe_matmul", {"ks": True}, f"dev{self.other_stream(prev.stream)}", 1)
        form = "host" if self.rng.integers(0, 2) else f"dev{self.other_stream(mm.stream)}"
        self.call(self.pick_handle("gate"), "gate", {"code": int(self.rng.integers(0, 11))}, form, self.pick_count())

    # -- the ring items: the TRLWE key switch, the packed CMUX, TRGSW encryption and the switching keys
    def ring(self, op, form, count=None, handle=None, src=None, **fixed):
        """A ring step: the variants of `op` in turn, a count of RING_COUNTS, `fixed` over the variant's arguments."""
        pick = [v for v in ring_variants() if v[0] == op]
        j = self.dealt.get("ring:" + op, 0)
        self.dealt["ring:" + op] = j + 1
        args = dict(pick[(self.seed + j) % len(pick)][1], **fixed)
        if count is None and op == "encrypt_trgsw":
            # 1, 2 or 5 selectors of 2t = 6 rows; one of 64 rows (65,536 noise samples: one draw in eight has a borderline
            # one and is drawn again)
            count = 1 if args["gadget"][1] == 32 else int(RING_COUNTS[int(self.rng.integers(0, 3))])
        elif count is None:
            count = int(RING_COUNTS[int(self.rng.integers(0, len(RING_COUNTS)))])
        return self.call(handle or self.pick_handle(op), op, args, form, count, src)

    def dev(self, *not_these):
        return f"dev{self.other_stream(*not_these)}"

    def elsewhere(self, prev):
        """The host form (the context's own stream), or another stream than the step before."""
        return "host" if self.rng.integers(0, 2) else self.dev(prev.stream)

    def switch_change(self, j):
        """An un-synchronised trlwe_keyswitch_dev of k on each view (the other view's last), AT ONCE a switch_key_change
        of the same k on the first (to a key of another (basebit, t); the step drains nothing: the library's device-wide drain is under
        test), at once a switch of that k on the changed view.  The first change of a sequence brings the view's first
        (1, 32) key: after a one- or two-row switch under it, a switch of the largest count so far finds ts_dig too small
        through t alone, under a running switch of the same k on the other view.  The second is followed by the same k
        on the two views in the other order."""
        q = 2 * self.seed + j
        h = ("E", "V2")[self.seed % 2]
        o = {"E": "V2", "V2": "E"}[h]
        k = SWITCH_KS[q % 3]
        prev = self.dev_before(min_ks_rows=1)
        own = self.ring("trlwe_keyswitch", self.dev(prev.stream), handle=h, k=k)  # (the changed view's own, still queued too)
        first = self.ring("trlwe_keyswitch", self.dev(own.stream), own.count, o, k=k)  # (the same ts_dig, the same size)
        new = switch_gadgets(h, k)[1 + j]
        assert new != self.switch[h][k] and (new[1] == 32) == (j == 0)
        self.add(Step("state", h, "switch_key_change", args={"k": k, "route": SWITCH_ROUTES[(q // 3 + q) % 3],
                                                             "to": switch_key_name(h, k, new)}))
        self.switch[h][k] = new
        if j == 0:
            self.ring("trlwe_keyswitch", self.elsewhere(first), 1 + int(self.rng.integers(0, 2)), h, k=k)
            count = max(33, self.ring_max["trlwe_keyswitch"])
            under = self.ring("trlwe_keyswitch", self.dev(), count, o, k=k)
            self.ring("trlwe_keyswitch", self.elsewhere(under), count, h, k=k, t_grow=True)
        else:
            follow = self.ring("trlwe_keyswitch", self.dev(first.stream), handle=h, k=k)
            self.ring("trlwe_keyswitch", self.elsewhere(follow), handle=o, k=k)

    def trgsw_pair(self, j):
        """A secret-staging _dev call, then at once a TRGSW encryption on the other of E / V2 (a third layout of the same
        ctx->sym_sec): by its host form and its device form, after an encrypting and after a decrypting call."""
        q = 2 * self.seed + j
        kind, form = ("enc", "dec")[(q // 2) % 2], ("host", "dev0")[q % 2]
        first_on = ("E", "V2")[(q // 4 + q) % 2]
        pick = [v for v in variants(self.shape) if v[0] in SECRET_OPS[:4] and v[0].startswith(kind)]
        op, args = pick[int(self.rng.integers(0, len(pick)))]
        self.call(first_on, op, args, self.dev(), self.pick_count())
        self.ring("encrypt_trgsw", form, handle={"E": "V2", "V2": "E"}[first_on])

    def ring_mix(self):
        """A _dev key switch, a ring _dev call on another stream, an unclaimed call on a third, the other ring family's
        _dev call, a key switch by the host form or on another stream."""
        a, b = (("cmux", "trlwe_keyswitch"), ("trlwe_keyswitch", "cmux"))[self.seed % 2]
        prev = self.dev_before(min_ks_rows=1)
        first = self.ring(a, self.dev(prev.stream))
        pick = [v for v in variants(self.shape) if v[0] in UNCLAIMED_OPS]
        op, args = pick[int(self.rng.integers(0, len(pick)))]
        mid = self.call(self.pick_handle(op), op, args, self.dev(first.stream), self.pick_count())
        last = self.ring(b, self.dev(mid.stream))
        self.call(self.pick_handle("gate"), "gate", {"code": int(self.rng.integers(0, 11))}, self.elsewhere(last), self.pick_count())

    def ring_grow(self):
        """RING_BIG ciphertexts (a second chunk pass; at least twice any earlier ring count) of one family directly after
        un-synchronised device work, of the other family at once on another stream (each family's digit scratch is its
        own: both are grow steps of their family, each under running device work), a small call of the first again."""
        a, b = (("trlwe_keyswitch", "cmux"), ("cmux", "trlwe_keyswitch"))[self.seed % 2]
        prev = self.dev_before()
        assert 2 * max(self.ring_max.values()) <= RING_BIG
        first = self.ring(a, self.dev(prev.stream), RING_BIG, ring_grow=True)
        second = self.ring(b, self.dev(first.stream), RING_BIG, ring_grow=True)
        self.ring(a, self.elsewhere(second))

    def cm_t_grow(self):
        """The sequence's first (1, 32) selector, at the largest CMUX count so far: cm_dig is too small through t alone,
        under a running CMUX of that count on another stream."""
        prev = self.dev_before(min_ks_rows=1)
        count = max(33, self.ring_max["cmux"])
        under = self.ring("cmux", self.dev(prev.stream), count)
        assert under.args["gadget"][1] < 32
        self.ring("cmux", self.elsewhere(under), count, gadget=CMUX_GADGETS[2], t_grow=True)

    def run(self):
        vs = [v for v in variants(self.shape) if v not in ring_variants()]
        order = np.random.default_rng([0xDEC4, self.shape.n]).permutation(len(vs))
        fixed = ["profiling_on", "kernel_times", "ring_times", "profiling_off", "kernel_times", "ring_times", "combining_off",
                 "combining_default",
                 "synchronize", "load_packing_key", "key_change", "key_change", "grow", "pair", "A", "B", "C", "D",
                 "secret_pair0", "secret_pair1", "sandwich", "ks_matmul", "E", "F", "switch_change0", "switch_change1",
                 "trgsw_pair0", "trgsw_pair1", "ring_mix", "ring_grow", "cm_t_grow"]
        budget = {"A": 3, "B": 2, "C": 3, "D": 4, "key_change": 2, "secret_pair0": 2, "secret_pair1": 2, "sandwich": 2, "ks_matmul": 2,
                  "E": 3, "F": 4, "switch_change0": 6, "switch_change1": 5, "trgsw_pair0": 2, "trgsw_pair1": 2, "ring_mix": 5,
                  "ring_grow": 4, "cm_t_grow": 3}
        n_deck = self.steps - sum(budget.get(f, 1) for f in fixed)
        # where the fixed items go among the deck's draws: the profiling and combining steps keep their order, the
        # others go anywhere, the grow step into the second half
        plan = dict()
        for pos, item in zip(np.sort(self.rng.integers(1, n_deck, 8)), fixed[:8]):
            plan.setdefault(int(pos), []).append(item)
        for item in fixed[8:]:
            pos = self.rng.integers(n_deck // 2 if item == "grow" else 1, n_deck)
            plan.setdefault(int(pos), []).append(item)
        open_chains = []
        for j in range(n_deck):
            for item in plan.get(j, []):
                if item in ("A", "B", "C", "D", "E", "F"):
                    ch = self.chain(item)
                    next(ch)
                    open_chains.append(ch)
                elif item == "grow":
                    self.grow()
                elif item == "pair":
                    self.pair()
                elif item.startswith("secret_pair"):
                    self.secret_pair(int(item[-1]))
                elif item == "sandwich":
                    self.sandwich()
                elif item == "ks_matmul":
                    self.ks_matmul()
                elif item.startswith(("switch_change", "trgsw_pair")):
                    getattr(self, item[:-1])(int(item[-1]))
                elif item in ("ring_mix", "ring_grow", "cm_t_grow"):
                    getattr(self, item)()
                else:
                    self.state(item)
            for ch in list(open_chains):  # a chain's next link: at once, or after one unrelated step
                if self.rng.integers(0, 2):
                    try:
                        next(ch)
                    except StopIteration:
                        open_chains.remove(ch)
            op, args = vs[order[(self.seed * n_deck + j) % len(vs)]]
            if op in STAGE_OPS and self.rng.integers(0, 4):
                # a stage op directly after a _dev step whose own key switch runs on at least as many rows
                prev = self.dev_before(min_ks_rows=1)
                self.call(self.pick_handle(op), op, args, "host", self.pick_count(at_most=prev.ks_rows))
            elif op == "pk_encrypt":  # under un-synchronised work on another stream (the host form runs on the context's own)
                prev = self.dev_before()
                form = "host" if self.rng.integers(0, 2) else f"dev{self.other_stream(prev.stream)}"
                self.call(self.pick_handle(op), op, args, form, self.pick_count(at_most=520))
            else:
                self.call(self.pick_handle(op), op, args, self.pick_form(op), self.pick_count())
        for ch in open_chains:
            for _ in ch:
                pass
        cost = sum(min(s.count, ROWS_PER_STEP) * s.oracle_bootstraps for s in self.seq)
        assert cost <= MAX_ORACLE_BOOTSTRAPS, (self.seed, cost)
        return self.seq


def random_sequence(seed, shape, steps=STEPS):
    """The sequence of `seed` on `shape` (a Shape or the name of one): a list of Steps, a few more than `steps` where a
    condition of the corpus (a _dev step before every state step, before a grow step and before most stage ops) needed
    one put in.  A pure function of its arguments."""
    shape = SHAPES[shape] if isinstance(shape, str) else shape
    return _Gen(seed, shape, steps).run()


def corpus(shape):
    name = shape if isinstance(shape, str) else shape.name
    return [random_sequence(seed, shape) for seed in SEEDS[name]]


def cone(sequence, i):
    """Step i and the steps chained from it."""
    hit = {i}
    for st in sequence:
        if st.kind == "call" and hit & set(st.sources):
            hit.add(st.i)
    return hit


def as_host(sequence):
    """The same steps made alone: every call by its host form, followed by synchronize()."""
    out = []
    for st in sequence:
        c = Step(st.kind, st.handle, st.op, "host" if st.kind == "call" else None, st.count, st.ins, st.args)
        c.i = st.i
        c.args["alone"] = True
        out.append(c)
    return out


def adjacency(sequence):
    """What the corpus condition counts, for one sequence: a dict name -> occurrences."""
    c = {}

    def hit(name):
        c[name] = c.get(name, 0) + 1

    grown = 0
    switch = {h: dict(SWITCH_START[h]) for h in SWITCH_START}  # the gadget of the key each view holds per k
    ring_bytes, ring_count = {op: 0 for op in RING_OPS}, {op: 0 for op in RING_OPS}  # the largest so far, per family
    for prev, st, nxt in zip([None] + sequence[:-1], sequence, sequence[1:] + [None]):
        if st.kind == "state" and st.op == "key_change" and nxt is not None and nxt.kind == "call" and \
                nxt.op == "pk_encrypt" and nxt.handle == "V2":
            hit("pk_encrypt on V2 after key_change")
        if prev is not None and nxt is not None and st.dev and st.op in UNCLAIMED_OPS and prev.queued and nxt.queued and \
                prev.claims and nxt.claims and prev.stream != st.stream != nxt.stream:
            hit("unclaimed call between two claiming dev calls on other streams")
            if prev.ring and nxt.ring:
                hit("unclaimed call between two ring dev calls on other streams")
        # (the host form, and TRGSW encryption's device form, run on the context's own stream, never a _dev step's)
        apart = prev is not None and prev.queued and st.kind == "call" and (not st.queued or st.stream != prev.stream)
        if st.kind == "state" and st.op == "switch_key_change":
            k, new = st.args["k"], switch_key_gadget(st.args["to"])
            assert new != switch[st.handle][k] and st.args["to"] == switch_key_name(st.handle, k, new), st
            hit("switch route " + st.args["route"])
            if prev is not None and prev.queued and prev.op == "trlwe_keyswitch" and prev.args["k"] == k and prev.handle != st.handle:
                hit("switch_key_change under a running switch of the same k on the other view")
                if nxt is not None and nxt.kind == "call" and nxt.op == "trlwe_keyswitch" and nxt.args["k"] == k and \
                        nxt.handle == st.handle and (not nxt.dev or nxt.stream != prev.stream):
                    hit("switch under the new key directly after switch_key_change")
            switch[st.handle][k] = new
        if st.ring:
            t = switch[st.handle][st.args["k"]][1] if st.op == "trlwe_keyswitch" else st.args["gadget"][1]
            size = ring_scratch_bytes(st.op, t, st.count)
            through_t = apart and prev.ring and size > ring_bytes[st.op] and st.count <= ring_count[st.op]
            if apart and prev.ks_rows > 0:
                hit(f"{st.op} after a dev key switch")
            if apart and prev.ring and prev.op != st.op:
                hit(f"{st.op} after {prev.op} dev on another stream")
            if through_t:
                hit(f"{st.op} scratch grown through t alone under a running ring dev call")
            if apart and st.op == prev.op == "trlwe_keyswitch" and st.args["k"] == prev.args["k"] and st.handle != prev.handle:
                hit(f"trlwe_keyswitch on {st.handle} after trlwe_keyswitch_dev on {prev.handle} with the same k")
            if st.args.get("t_grow"):
                assert through_t and t == 32, st
            if st.args.get("ring_grow"):
                # (at least twice any earlier ring count but the other family's grow step directly before it: a family's
                # digit scratch is its own)
                assert prev.queued and st.count == RING_BIG >= 2 * ring_count[st.op] and st.passes == 2, st
                assert st.count >= 2 * max(ring_count.values()) or (prev.args.get("ring_grow") and prev.op != st.op), st
                hit(f"dev then {st.op} ring grow")
            ring_bytes[st.op], ring_count[st.op] = max(ring_bytes[st.op], size), max(ring_count[st.op], st.count)
        if apart and prev.ring and st.ks_rows > 0:
            hit(f"key switch after a {prev.op} dev")
        if apart:
            if prev.op in SECRET_OPS and st.op in SECRET_OPS:
                if st.dev:
                    hit("secret-staging call after a secret-staging dev call on another stream")
                else:
                    hit("secret-staging host call after a secret-staging dev call")
                hit(f"secret-staging {st.op[:3]} after {prev.op[:3]}")
                if prev.handle != st.handle:
                    hit(f"secret-staging call on {st.handle} after a secret-staging dev call on {prev.handle}")
                    if st.op == "encrypt_trgsw":
                        hit(f"encrypt_trgsw ({'device' if st.dev else 'host'} form) after a secret-staging dev call of the other view")
                        hit(f"encrypt_trgsw after a secret-staging {prev.op[:3]} dev call of the other view")
            if st.op == "trlwe_matmul" and st.ks_rows and prev.ks_rows:
                hit("trlwe_matmul:ks under a running key switch")
            if prev.op == "trlwe_matmul" and prev.ks_rows and st.ks_rows:
                hit("key switch after a running trlwe_matmul:ks dev")
            if st.op == "pk_encrypt":
                hit("pk_encrypt after a dev call on another stream")
        if st.kind == "call":
            hit("op " + variant_name(st.op, st.args))
            hit("form " + st.form)
            if st.sources:
                hit("chained " + st.op)
            if st.args.get("grow"):
                assert st.count >= 2 * grown, st
            grown = max(grown, st.count)
        else:
            hit("state " + st.op)
            if st.op == "key_change":
                hit("route " + st.args["route"])
        if prev is None:
            continue
        if prev.handle == "E" and st.handle == "V2":
            hit("V2 after E")
        if prev.handle == "V2" and st.handle == "E":
            hit("E after V2")
        if not prev.queued:
            continue
        if st.kind == "state":
            hit("dev then " + st.op)
        elif st.args.get("grow"):
            hit("dev then grow")
        if st.kind == "call" and not st.dev:
            hit("dev then host")
        if st.dev and st.stream != prev.stream:
            hit("dev then dev on another stream")
        if st.kind == "call" and st.op in STAGE_OPS and prev.ks_rows >= st.count:
            hit("stage op under a running key switch")  # (a _dev step's stream is never the context's own)
            if st.op == "identity_key_switch" and st.count >= 384:
                hit("key switch of 384 rows or more under a running key switch")
    return c


def ring_orders():
    """The orders of adjacency() the ring items exist for: the corpus condition wants each three times over a shape."""
    need = ["unclaimed call between two ring dev calls on other streams",
            "switch_key_change under a running switch of the same k on the other view",
            "switch under the new key directly after switch_key_change",
            "trlwe_keyswitch on V2 after trlwe_keyswitch_dev on E with the same k",
            "trlwe_keyswitch on E after trlwe_keyswitch_dev on V2 with the same k",
            "cmux after trlwe_keyswitch dev on another stream", "trlwe_keyswitch after cmux dev on another stream",
            "chained trlwe_keyswitch", "chained cmux", "chained decrypt_trlwe"]
    for op in RING_OPS:
        need += [f"{op} after a dev key switch", f"key switch after a {op} dev", f"dev then {op} ring grow",
                 f"{op} scratch grown through t alone under a running ring dev call"]
    need += ["switch route " + r for r in SWITCH_ROUTES]
    need += [f"encrypt_trgsw ({f} form) after a secret-staging dev call of the other view" for f in ("host", "device")]
    need += [f"encrypt_trgsw after a secret-staging {k} dev call of the other view" for k in ("enc", "dec")]
    return need


def ring_passes(sequence):
    """What each ring_times step must report: {step: (passes of the TRLWE key switch, passes of the CMUX)}, the chunk
    passes issued on the context (E and V2) since the ring_times step before while profiling was on (it is off at the
    start).  Read off the sequence."""
    out, on, n = {}, False, {op: 0 for op in RING_OPS}
    for st in sequence:
        if st.kind == "state" and st.op in ("profiling_on", "profiling_off"):
            on = st.op == "profiling_on"
        elif st.kind == "state" and st.op == "ring_times":
            out[st.i] = (n["trlwe_keyswitch"], n["cmux"])
            n = {op: 0 for op in RING_OPS}
        elif st.ring and on:
            n[st.op] += st.passes
    return out


def switch_keys_after(sequence, upto=None):
    """The switching key each view holds for each k after step `upto` (the last by default): {handle: {k: name}}."""
    held = {h: {k: switch_key_name(h, k, g) for k, g in SWITCH_START[h].items()} for h in SWITCH_START}
    for st in sequence[:None if upto is None else upto + 1]:
        if st.kind == "state" and st.op == "switch_key_change":
            held[st.handle][st.args["k"]] = st.args["to"]
    return held


def ring_clobbered_steps(sequence):
    """What a device whose ring families each share their digit scratch WITHOUT a claim would get wrong: {step: donor
    step}, every ring _dev step that a call of the same family of at least its size follows while it is pending -- its
    stream (or the device) not synchronised and no later call queued on that stream -- with the last such call, whose
    digits it reads.  Read off the sequence alone, as unclaimed_secret_steps."""
    donor, pending = {}, []
    for st in sequence:
        if st.kind == "state":
            if st.op in ("synchronize", "switch_key_change"):
                pending = []
            elif st.op == "key_change":
                pending = [p for p in pending if p.stream not in st.args["wait"]]
            continue
        if st.queued:
            pending = [p for p in pending if p.stream != st.stream]
        if st.ring:
            for p in pending:
                if p.op == st.op and p.count <= st.count:
                    donor[p.i] = st.i
            if st.dev:
                pending.append(st)
    return donor


def undrained_switch_steps(sequence):
    """What a device whose switch_key_change does NOT drain would get wrong: {step: key name}, every trlwe_keyswitch_dev
    of the changed k on the changed view that nothing has synchronised (its stream, or the device) when the key is
    replaced, with the key that replaced its own."""
    wrong, queued = {}, []
    for st in sequence:
        if st.kind == "state":
            if st.op == "synchronize":
                queued = []
            elif st.op == "key_change":
                queued = [p for p in queued if p.stream not in st.args["wait"]]
            elif st.op == "switch_key_change":
                for p in queued:
                    if p.handle == st.handle and p.args["k"] == st.args["k"]:
                        wrong[p.i] = st.args["to"]
            continue
        if st.op == "trlwe_keyswitch" and st.dev:
            queued.append(st)
    return wrong


def unclaimed_secret_steps(sequence):
    """What a device whose one secret-staging buffer is shared WITHOUT a claim would get wrong: {step: handle}, every
    secret-staging _dev step that another secret-staging call follows before the step's stream (or the device) is next
    synchronised, with the handle whose key the last such call staged.  Read off the sequence alone: `synchronize`
    drains everything, a key change the streams it waits for."""
    wrong, pending = {}, []
    for st in sequence:
        if st.kind == "state":
            if st.op in ("synchronize", "switch_key_change"):  # (every route of a switching-key change drains the device)
                pending = []
            elif st.op == "key_change":
                pending = [p for p in pending if p.stream not in st.args["wait"]]
            continue
        if st.op not in SECRET_OPS:
            continue
        for p in pending:
            wrong[p.i] = st.handle
        if st.queued:  # (TRGSW encryption clobbers what is pending and, drained on return, never stays pending itself)
            pending.append(st)
    return {i: h for i, h in wrong.items() if h != sequence[i].handle}


def sum_counts(dicts):
    out = {}
    for d in dicts:
        for k, v in d.items():
            out[k] = out.get(k, 0) + v
    return out


# ---- operands ---------------------------------------------------------------------------------------------------------
def words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def encrypt_border(op, rng_key, first, count, alpha, gadget=None):
    """The borderline mask of an encrypting step's noise samples (keygen_model.borderline: within 2^-20 of a torus
    step): [count] for encrypt and pk_encrypt, [groups][N] for encrypt_trlwe (count: its groups), [count 2t][N] for
    encrypt_trgsw (gadget: its (basebit, t)).  It depends on the generator key, the indices and alpha, never on the
    secret key."""
    import packed_encrypt_model as PEM
    import pk_encrypt_model as PM
    import sym_encrypt_model as SM

    if op == "encrypt_trgsw":
        import cmux_model as CM

        return CM.noise(rng_key, CM.row_indices(first, count, gadget[1]), alpha).border
    if op == "encrypt_trlwe":
        return PEM.noise(rng_key, PEM.group_indices(first, count), alpha).border
    rows = PM.row_indices(first, count)
    return SM.noise(rng_key, rows, alpha, SM.TLWE[1]).border if op == "encrypt" else PM.noise(rng_key, rows, alpha, PM.PKE[1]).border


def decode(phases, mode):
    """client.SecretKey's decodes of phases, as the u32 words tfhe_hip_batch_decrypt* return: the phase, the boolean
    (the phase read as i32 is non-negative), the message mod MESSAGE_MODULUS."""
    from rs_tfhe_amd.client import torus_to_f64

    ph = np.ascontiguousarray(phases, dtype=np.uint32).reshape(-1)
    if mode == "phase":
        return ph
    if mode == "bool":
        return (ph.view(np.int32) >= 0).astype(np.uint32)
    m = MESSAGE_MODULUS
    return ((torus_to_f64(ph) / (1.0 / (2.0 * m)) + 0.5).astype(np.int64) % m).astype(np.uint32)


def make_pools(shape, seed, secrets):
    """The pools of a sequence: genuine encryptions of booleans under the secret key of each handle (`secrets`: handle ->
    an object with encrypt_bool(bits, seed)), and uniformly random level-1 rows, TRLWEs and tables.  "bits:<handle>" are
    the plaintexts."""
    rng = np.random.default_rng([0x9001, seed, shape.n])
    pools = {}
    for h in HANDLES:
        bits = rng.integers(0, 2, POOL).astype(bool)
        pools["bits:" + h] = bits
        pools["lv0:" + h] = np.ascontiguousarray(secrets[h].encrypt_bool(bits, int(rng.integers(1, 1 << 31))), dtype=np.uint32)
    pools["lv1"] = words(rng, (POOL, N + 1))
    pools["trlwe"] = words(rng, (8, 2, N))
    pools["tv"] = words(rng, (8, 2, N))
    # the ring steps: their ROWS_PER_STEP rows, one selector of random words per gadget, and GEN_POOL genuine packed encryptions of known words
    # under each handle's ring key, made on the CPU ("genwords:<handle>" are the plaintexts)
    import packed_encrypt_model as PEM

    pools["ring"] = words(rng, (ROWS_PER_STEP, 2, N))
    for _, t in CMUX_GADGETS:
        pools[f"sel:{t}"] = words(rng, (1, 2 * t, 2, N))
    for h in ("E", "V2"):
        plain = pools["genwords:" + h] = words(rng, (GEN_POOL, N))
        seeds = rng.integers(0, 256, (2, 32)).astype(np.uint8)
        pools["gen:" + h] = PEM.encrypt(secrets[h].key_lv1, plain.reshape(-1), GEN_POOL * N, int(rng.integers(0, 1 << 40)),
                                        shape.alpha_lv1, seeds[0].tobytes(), seeds[1].tobytes())[0]
    return pools


def materialise(st, pools, outputs=None):
    """The operands of a call step as arrays (None where the call takes none; a chained operand from `outputs`, or None
    when `outputs` is None)."""
    got = []
    for spec in st.ins:
        if spec is None:
            got.append(None)
        elif spec[0] == "rows":
            got.append(np.ascontiguousarray(pools[spec[1]][spec[2]]))
        elif spec[0] == "out":
            got.append(None if outputs is None else outputs[spec[1]])
        else:
            got.append(np.ascontiguousarray(spec[1]))
    return got


def out_parts(st, n):
    """The shapes of the device outputs of a step: one, or the two of an encrypting step that returns both forms."""
    if st.op in ("encrypt", "encrypt_trlwe"):
        full, bodies = ((st.count, n + 1), (st.count,)) if st.op == "encrypt" else ((st.count, 2, N), (st.count, N))
        return {"full": [full], "bodies": [bodies], "both": [full, bodies]}[st.args["out"]]
    return [out_shape(st, n)]


def join_parts(parts):
    """full and bodies of one step side by side, per row"""
    parts = [np.ascontiguousarray(p, dtype=np.uint32) for p in parts]
    return parts[0] if len(parts) == 1 else np.concatenate([p.reshape(len(p), -1) for p in parts], axis=1)


def out_shape(st, n):
    c, a = st.count, st.args
    if st.op == "encrypt":
        return (c, {"full": n + 1, "bodies": 1, "both": n + 2}[a["out"]])
    if st.op == "encrypt_trlwe":
        return (c, {"full": 2, "bodies": 1, "both": 3}[a["out"]], N)
    if st.op in ("expand_seeded_trlwe", "trlwe_keyswitch", "cmux"):
        return (c, 2, N)
    if st.op == "encrypt_trgsw":
        return (c, 2 * a["gadget"][1], 2, N)
    if st.op in ("decrypt", "decrypt_trlwe"):
        return (c,)
    if st.op == "trlwe_matmul" and not a["ks"]:
        return (c, N + 1)
    if st.op == "polymul":
        return (c, 2, N)
    if st.op == "lincomb_bootstrap_many":
        return (a["k"] * c, n + 1)
    if st.op in ("blind_rotate", "external_product", "pack_table"):
        return (c, 2, N)
    if st.op == "sample_extract":
        return (c, N + 1)
    if st.op == "pack":
        return (-(-c // N), 2, N)
    return (c, n + 1)


# ---- the backends -------------------------------------------------------------------------------------------------------
class TorchBackend:
    """cuda:0 through torch: 32-bit words travel as int32 tensors, gate codes as uint8, weights as int8."""

    def __init__(self):
        import torch

        self.torch = torch
        self.dev = torch.device("cuda:0")

    def streams(self):
        return [None, self.torch.cuda.Stream(device=0), self.torch.cuda.Stream(device=0)]

    def upload(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a if a.dtype in (np.uint8, np.int8) else a.view(np.int32)).to(self.dev)

    def empty(self, shape):
        return self.torch.full(shape, FILL, dtype=self.torch.int32, device=self.dev)

    def download(self, t):
        return t.cpu().numpy().view(np.uint32)

    def synchronize(self):
        self.torch.cuda.synchronize()

    def stream_synchronize(self, stream):
        (self.torch.cuda.default_stream(0) if stream is None else stream).synchronize()

    def pinned_copy(self, a):
        from rs_tfhe_amd.engine import pinned_copy

        return pinned_copy(a)

    def pinned_empty(self, shape):
        from rs_tfhe_amd.engine import pinned_empty

        return pinned_empty(shape)


class FakeTensor:
    """A numpy array that says it is on the device: what the stand-in handles' _dev methods take."""

    def __init__(self, arr, root=None):
        self.arr = arr
        self.root = self if root is None else root  # the tensor a view was taken from

    def reshape(self, *shape):
        view = self.arr.reshape(*shape)
        assert np.shares_memory(view, self.arr)
        return FakeTensor(view, self.root)

    def __getitem__(self, key):
        return FakeTensor(self.arr[key], self.root)


class FakeBackend:
    def __init__(self, on_synchronize=None, on_stream_synchronize=None):
        self.on_synchronize, self.on_stream_synchronize = on_synchronize, on_stream_synchronize

    def streams(self):
        return [None, "side1", "side2"]

    def upload(self, a):
        return FakeTensor(np.array(a))

    def empty(self, shape):
        return FakeTensor(np.full(shape, FILL, np.uint32))

    def download(self, t):
        return t.arr.copy()

    def synchronize(self):
        if self.on_synchronize:
            self.on_synchronize()

    def stream_synchronize(self, stream):
        if self.on_stream_synchronize:
            self.on_stream_synchronize(stream)

    def pinned_copy(self, a):
        return np.array(a)

    def pinned_empty(self, shape):
        return np.empty(shape, np.uint32)


# ---- the executor -------------------------------------------------------------------------------------------------------
def _host_call(h, st, x, backend, sec=None):
    op, a = st.op, st.args
    if op == "gate":
        if st.form == "pinned":
            out = backend.pinned_empty(x[0].shape)
            got = h.batch_gate(a["code"], x[0], x[1], out=out)
            assert got is out
            return np.array(out)
        return h.batch_gate(a["code"], x[0], x[1])
    if op == "gates_mixed":
        return h.batch_gates_mixed(x[0], x[1], x[2], keyswitch=a["ks"])
    if op == "bootstrap":
        tv = x[1] if a["tv"] == "per" or x[1] is None else x[1][0]
        return h.batch_bootstrap(x[0], tv, keyswitch=a["ks"])
    if op == "tlwe_lincomb":
        return h.batch_tlwe_lincomb(a["ca"], x[0], a["cb"], x[1], a["cc"])
    if op == "lincomb_bootstrap":
        tv = x[2] if a["tv"] == "per" or x[2] is None else x[2][0]
        return h.batch_lincomb_bootstrap(a["ca"], x[0], a["cb"], x[1], a["cc"], tv, keyswitch=a["ks"])
    if op == "lincomb_bootstrap_many":
        return h.batch_lincomb_bootstrap_many(a["ca"], x[0], a["cb"], x[1], a["cc"], x[2][0], n_luts=a["k"], keyswitch=a["ks"])
    if op == "mux":
        return h.batch_mux(x[0], x[1], x[2], a["naive"])
    if op == "blind_rotate":
        return h.batch_blind_rotate(x[0], None if x[1] is None else x[1][0])
    if op == "identity_key_switch":
        return h.batch_identity_key_switch(x[0])
    if op == "sample_extract":
        return h.batch_sample_extract(x[0], a["k"])
    if op == "external_product":
        return h.batch_external_product(x[0], x[1])
    if op == "pack":
        return h.pack(x[0])
    if op == "unpack":
        return h.unpack(x[0], st.count, x[1]) if x[1] is None else h.unpack(x[0], slots=x[1])
    if op == "pack_table":
        return h.pack_table(x[0].reshape(a["m"], st.count, -1), a["m"])
    if op == "bootstrap_bivariate":
        return h.batch_bootstrap_bivariate(x[0], x[1], x[2], a["m"], a["k"], keyswitch=a["ks"])
    if op == "reencrypt":
        return h.batch_reencrypt(x[0])
    if op == "expand_seeded":
        return h.expand_seeded(SeededBodies(h.params, a["seed"], a["first"], x[0]))
    x = shaped(st, x, h.params.n)
    modulus = MESSAGE_MODULUS if a.get("mode") == "message" else None
    if op in ("encrypt", "encrypt_trlwe"):
        call, key = (h.batch_encrypt, sec.key_lv0) if op == "encrypt" else (h.batch_encrypt_trlwe, sec.key_lv1)
        got = call(key, x[0], a["alpha"], a["rng_key"], a["mask_seed"], a["first"], full=a["out"] != "bodies", bodies=a["out"] != "full")
        got = got if isinstance(got, tuple) else (got,)
        return join_parts([getattr(g, "bodies", g) for g in got])
    if op == "expand_seeded_trlwe":
        return h.expand_seeded_trlwe(SeededGroups(a["seed"], a["first"], x[0]))
    if op == "pk_encrypt":
        return h.batch_pk_encrypt(x[0], a["alpha"], a["rng_key"], a["first"])
    if op == "decrypt":
        return h.batch_decrypt(sec.key_lv0 if a["width"] == "lv0" else sec.key_lv1, x[0], a["mode"], modulus)
    if op == "decrypt_trlwe":
        return h.batch_decrypt_trlwe(sec.key_lv1, x[0], st.count, a["mode"], modulus)
    if op == "tlwe_matmul":
        return h.batch_tlwe_matmul(x[0], x[1], x[2])
    if op == "trlwe_matmul":
        return h.batch_trlwe_matmul(x[0], x[1], x[2], keyswitch=a["ks"])
    if op == "polymul":
        return h.batch_trlwe_polymul(x[0], x[1], x[2])
    if op == "conv2d":
        return h.batch_tlwe_conv2d(x[0], x[1], x[2], stride=a["shape"][5], padding=a["shape"][6])
    if op == "trlwe_keyswitch":
        return h.batch_trlwe_keyswitch(a["k"], x[0])
    if op == "cmux":  # (the step's one selector: the first of its operand's)
        return h.batch_trlwe_cmux(x[0][0], a["gadget"][0], a["gadget"][1], x[1], x[2], reference_digits=a["reference"])
    if op == "encrypt_trgsw":
        return h.batch_encrypt_trgsw(sec.key_lv1, x[0], a["gadget"][0], a["gadget"][1], a["alpha"], a["rng_key"], a["first"])
    raise ValueError(op)


def shaped(st, x, n):
    """The operands of a new-family step in the shapes its call takes: views of the flat pool rows, or of a chained
    output (chain C hands the first 62 of its 65 ciphertexts to the matrix; chain D the four TRLWEs of the polynomial
    product as four groups).  numpy arrays, torch tensors and FakeTensors alike."""
    op, a, x = st.op, st.args, list(x)
    if op == "tlwe_matmul":
        rows, cols, groups = a["shape"]
        x[1] = x[1][:groups * cols].reshape(groups, cols, n + 1)
    elif op == "trlwe_matmul":
        x[1] = x[1].reshape(-1, 2, N)
    elif op == "polymul":
        rows, cols, groups = a["shape"]
        x[1] = x[1].reshape(groups, cols, 2, N)
    elif op == "conv2d":
        in_h, in_w, in_c, _, _, _, _, groups = a["shape"]
        x[1] = x[1].reshape(groups, in_h, in_w, in_c, n + 1)
    elif op == "decrypt":
        x[0] = x[0].reshape(-1, (n if a["width"] == "lv0" else N) + 1)
    elif op == "decrypt_trlwe":
        x[0] = x[0].reshape(-1, 2, N)
    return x


def shaped_out(st, out, n):
    """The device output of a shape-table step in the shape its call takes (a view of the flat rows)."""
    if st.op in ("tlwe_matmul", "trlwe_matmul", "polymul"):
        rows, _, groups = st.args["shape"]
        return out.reshape((groups, rows, 2, N) if st.op == "polymul" else (groups, rows, -1))
    if st.op == "conv2d":
        in_h, in_w, _, k, out_c, stride, pad, groups = st.args["shape"]
        return out.reshape(groups, (in_h + 2 * pad[0] - k) // stride[0] + 1, (in_w + 2 * pad[1] - k) // stride[1] + 1, out_c, n + 1)
    return out


class SeededGroups:
    """What Engine.expand_seeded_trlwe reads of a seeded.SeededPackedCiphertexts."""

    def __init__(self, mask_seed, first_group, bodies):
        self.mask_seed, self.first_group, self.bodies = mask_seed, first_group, bodies


class SeededBodies:
    """What Engine.expand_seeded reads of a seeded.SeededCiphertexts."""

    def __init__(self, params, mask_seed, first_index, bodies):
        self.params, self.mask_seed, self.first_index, self.bodies = params, mask_seed, first_index, bodies


def _dev_call(h, st, t, out, stream, sec=None, aux=None):
    op, a = st.op, st.args
    if op == "gate":
        h.batch_gate_dev(a["code"], t[0], t[1], out, stream=stream)
    elif op == "gates_mixed":
        h.batch_gates_mixed_dev(t[0], t[1], t[2], out, stream=stream, keyswitch=a["ks"])
    elif op == "bootstrap":
        h.batch_bootstrap_dev(t[0], out, testvec=t[1], per_ct=a["tv"] == "per", keyswitch=a["ks"], stream=stream)
    elif op == "tlwe_lincomb":
        h.batch_tlwe_lincomb_dev(a["ca"], t[0], a["cb"], t[1], a["cc"], out, stream=stream)
    elif op == "lincomb_bootstrap":
        h.batch_lincomb_bootstrap_dev(a["ca"], t[0], a["cb"], t[1], a["cc"], out, testvec=t[2], per_ct=a["tv"] == "per",
                                      keyswitch=a["ks"], stream=stream)
    elif op == "lincomb_bootstrap_many":
        h.batch_lincomb_bootstrap_many_dev(a["ca"], t[0], a["cb"], t[1], a["cc"], out, t[2], n_luts=a["k"], keyswitch=a["ks"],
                                           stream=stream)
    elif op == "mux":
        h.batch_mux_dev(t[0], t[1], t[2], out, a["naive"], stream=stream)
    elif op == "blind_rotate":
        h.batch_blind_rotate_dev(t[0], out, testvec=t[1], stream=stream)
    elif op == "pack":
        h.pack_dev(t[0], out, stream=stream)
    elif op == "unpack":
        h.unpack_dev(t[0], out, st.count, slots=t[1], stream=stream)
    elif op == "pack_table":
        h.pack_table_dev(t[0], a["m"], out, stream=stream)
    elif op == "bootstrap_bivariate":
        h.batch_bootstrap_bivariate_dev(t[0], t[1], t[2], a["m"], out, n_luts=a["k"], keyswitch=a["ks"], stream=stream)
    elif op == "reencrypt":
        h.batch_reencrypt_dev(t[0], out, stream=stream)
    elif op == "expand_seeded":
        h.expand_seeded_dev(a["seed"], a["first"], t[0], out, stream=stream)
    else:
        _dev_call_families(h, st, shaped(st, t, h.params.n), shaped_out(st, out, h.params.n), stream, sec, aux)


def _dev_call_families(h, st, t, out, stream, sec, aux):
    """The _dev forms of encryption, decryption and the linear layers."""
    op, a = st.op, st.args
    modulus = MESSAGE_MODULUS if a.get("mode") == "message" else None
    if op in ("encrypt", "encrypt_trlwe"):
        call, key = (h.batch_encrypt_dev, sec.key_lv0) if op == "encrypt" else (h.batch_encrypt_trlwe_dev, sec.key_lv1)
        full, bodies = {"full": (out, None), "bodies": (None, out), "both": (out, aux)}[a["out"]]
        call(key, t[0], a["alpha"], a["mask_seed"], a["rng_key"], a["first"], bodies=bodies, out=full, stream=stream)
    elif op == "expand_seeded_trlwe":
        h.expand_seeded_trlwe_dev(a["seed"], a["first"], t[0], out, stream=stream)
    elif op == "pk_encrypt":
        h.batch_pk_encrypt_dev(t[0], out, a["alpha"], a["rng_key"], a["first"], stream=stream)
    elif op == "decrypt":
        h.batch_decrypt_dev(sec.key_lv0 if a["width"] == "lv0" else sec.key_lv1, t[0], out, a["mode"], modulus, stream=stream)
    elif op == "decrypt_trlwe":
        h.batch_decrypt_trlwe_dev(sec.key_lv1, t[0], st.count, out, a["mode"], modulus, stream=stream)
    elif op == "tlwe_matmul":
        h.batch_tlwe_matmul_dev(t[0], t[1], out, bias=t[2], stream=stream)
    elif op == "trlwe_matmul":
        h.batch_trlwe_matmul_dev(t[0], t[1], out, bias=t[2], keyswitch=a["ks"], stream=stream)
    elif op == "polymul":
        h.batch_trlwe_polymul_dev(t[0], t[1], out, bias=t[2], stream=stream)
    elif op == "conv2d":
        h.batch_tlwe_conv2d_dev(t[0], t[1], out, bias=t[2], stride=a["shape"][5], padding=a["shape"][6], stream=stream)
    elif op == "trlwe_keyswitch":
        h.batch_trlwe_keyswitch(a["k"], t[0], out=out, stream=stream)
    elif op == "cmux":
        h.batch_trlwe_cmux(t[0][0], a["gadget"][0], a["gadget"][1], t[1], t[2], reference_digits=a["reference"], out=out, stream=stream)
    elif op == "encrypt_trgsw":  # no stream argument: the context's own, finished on return
        h.batch_encrypt_trgsw_dev(sec.key_lv1, t[0], a["gadget"][0], a["gadget"][1], out, a["alpha"], a["rng_key"], a["first"])
    else:
        raise ValueError(op)


def _state(handles, st, streams, backend, info):
    h = handles[st.handle]
    if st.op in ("profiling_on", "profiling_off"):
        h.set_profiling(st.op == "profiling_on")
    elif st.op == "kernel_times":
        info["kernel_times"].append((st.i, h.kernel_times()))
    elif st.op == "combining_off":
        h.set_combining(0)
    elif st.op == "combining_default":
        h.set_combining(handles["combining_default"])
    elif st.op == "synchronize":
        h.synchronize()
    elif st.op == "load_packing_key":
        h.load_packing_key(handles["packing"][st.handle])
    elif st.op == "key_change":
        for k in st.args["wait"]:  # the caller's part: V2's own work is drained before V2's key changes
            backend.stream_synchronize(streams[k])
        book, target, route = handles["book"], st.args["target"], st.args["route"]
        if route == "load":
            h.load_cloud_key(book[target + "/gen"]["full"])
        elif route == "compressed":
            h.load_compressed_cloud_key(book[target + "/comp"]["comp"])
        else:
            h.gen_cloud_key(*book[target + "/gen"]["gen"])
    elif st.op == "switch_key_change":  # (nothing drained here: the library's device-wide drain is under test)
        name, k, route = st.args["to"], st.args["k"], st.args["route"]
        key = handles["switch_book"][name]
        if route == "gen":  # generated under queued work: the book's words
            ring_key = handles["secrets"][st.handle].key_lv1
            got = h.gen_trlwe_switch_key(ring_key, ring_key, k, key.basebit, key.t, rng_key=switch_gen_key(name))
            assert bytes(got.mask_seed) == bytes(key.mask_seed) and np.array_equal(got.bodies, key.bodies), st
        else:
            if route == "drop_load":
                h.drop_trlwe_switch_key(k)
                assert not h.trlwe_switch_key_is_loaded(k), st
            h.load_trlwe_switch_key(key)
        assert h.trlwe_switch_key_is_loaded(k), st
    elif st.op == "ring_times":  # the getters of the ring families' timing pairs, and each once more
        first = (h.trlwe_switch_times(), h.cmux_times())
        info["ring_times"].append((st.i, first, (h.trlwe_switch_times(), h.cmux_times())))
    else:
        raise ValueError(st.op)


def check_ring_times(sequence, info):
    """Every ring_times step reported the chunk passes the sequence issued while profiling was on (ring_passes), times
    that are no less than zero, and nothing at all when asked again at once."""
    want = ring_passes(sequence)
    assert [i for i, _, _ in info["ring_times"]] == sorted(want)
    for i, (ts, cm), again in info["ring_times"]:
        assert (ts["passes"], cm["passes"]) == want[i], (sequence[i], ts, cm, want[i])
        assert min(ts["digits_ms"], ts["contraction_ms"], cm["digits_ms"], cm["contraction_ms"], cm["addend_ms"]) >= 0.0, (ts, cm)
        assert all(v == 0 for d in again for v in d.values()), (sequence[i], again)
    return want


def run(sequence, handles, streams, pools, backend=None):
    """Make the calls in order, with no synchronisation between steps.  handles: {"E", "V2", "VR": Engine-shaped
    handles; "book": key name -> what each key-change route loads; "packing": handle -> its packing key;
    "combining_default": the context's default; "secrets": handle -> the secret key (key_lv0, key_lv1) its encrypting and
    decrypting steps name; "switch_book": name -> the switching key a switch_key_change brings}.  Before the first step every fresh operand is uploaded (or copied to
    pinned memory), every _dev step gets an output tensor of its own, and the device is synchronised once; host results
    are kept as returned; device results are read after the last step and one device-wide synchronisation.
    Returns ({step: words}, info)."""
    be = backend if backend is not None else TorchBackend()
    n = handles["E"].params.n
    staged, outs, aux, results = {}, {}, {}, {}
    secrets = handles.get("secrets", {})
    info = {"kernel_times": [], "ring_times": [], "seconds": 0.0}
    for st in sequence:
        if st.kind != "call":
            continue
        x = materialise(st, pools)
        if st.dev:
            staged[st.i] = [None if v is None else be.upload(v) for v in x]
            parts = out_parts(st, n)
            outs[st.i] = be.empty(parts[0])
            if len(parts) > 1:  # full and bodies of one encrypting step
                aux[st.i] = be.empty(parts[1])
        else:
            staged[st.i] = [None if v is None else be.pinned_copy(v) for v in x] if st.form == "pinned" else x
    assert len({id(o) for o in list(outs.values()) + list(aux.values())}) == len(outs) + len(aux)
    be.synchronize()
    t0 = time.perf_counter()
    for st in sequence:
        if st.kind == "state":
            _state(handles, st, streams, be, info)
            continue
        h, x = handles[st.handle], staged[st.i]
        for k, spec in enumerate(st.ins):
            if spec is not None and spec[0] == "out":  # a chained operand: the earlier step's own output
                x[k] = outs[spec[1]] if st.dev else results[spec[1]]
        if st.dev:
            _dev_call(h, st, x, outs[st.i], streams[st.stream], secrets.get(st.handle), aux.get(st.i))
        else:
            results[st.i] = np.ascontiguousarray(_host_call(h, st, x, be, secrets.get(st.handle)), dtype=np.uint32).reshape(out_shape(st, n))
            if st.args.get("alone"):
                h.synchronize()
    be.synchronize()
    info["seconds"] = time.perf_counter() - t0
    for i, t in outs.items():
        parts = [be.download(t)] + ([be.download(aux[i])] if i in aux else [])
        results[i] = join_parts(parts).reshape(out_shape(sequence_step(sequence, i), n))
    return results, info


def sequence_step(sequence, i):
    st = sequence[i]
    assert st.i == i
    return st


def final_keys(sequence):
    """The cloud key V2 holds after the last step."""
    key = "K2/gen"
    for st in sequence:
        if st.kind == "state" and st.op == "key_change":
            key = key_after(st)
    return key


def key_after(st):
    return st.args["target"] + ("/comp" if st.args["route"] == "compressed" else "/gen")


# key / re-encryption key / packing key / public key loaded, then a switching key for each k of SWITCH_KS (whichever
# route brought the last one: final_switch_check holds its words)
EXPECTED_FLAGS = {"E": (1, 0, 1, 1, 1, 1, 1), "V2": (1, 0, 1, 1, 1, 1, 1), "VR": (0, 1, 0, 0, 0, 0, 0)}


def flags(handle):
    lib, ctx = handle._lib, handle._member_ctx(0)
    return (lib.tfhe_hip_key_is_loaded(ctx), lib.tfhe_hip_reenc_key_is_loaded(ctx), lib.tfhe_hip_packing_key_is_loaded(ctx),
            lib.tfhe_hip_public_key_is_loaded(ctx)) + tuple(int(handle.trlwe_switch_key_is_loaded(k)) for k in SWITCH_KS)


def final_switch_check(sequence, handles, pools, model):
    """After the last step: a two-row switch under each key the model says a view holds gives the model's words."""
    held = switch_keys_after(sequence)
    rows = pools["ring"][:2]
    model.ring_pool = pools["ring"]  # (the model takes the pool's third row along: expected() asks for it under these keys)
    for h in held:
        for k, name in held[h].items():
            assert handles[h].trlwe_switch_key_is_loaded(k), (h, k)
            got = np.ascontiguousarray(handles[h].batch_trlwe_keyswitch(k, rows), dtype=np.uint32)
            assert np.array_equal(got, model.eval(name, h, "trlwe_keyswitch", {"k": k}, 2, [rows])), (h, k, name)


# ---- the model ----------------------------------------------------------------------------------------------------------
def prep(a, b, ca, cb, cc):
    p = (np.uint32(ca) * a + np.uint32(cb) * b).astype(np.uint32)
    p[..., -1] += np.uint32(cc)
    return p


class Model:
    """The words of one call under one key.  keys: {"params": the product's SecurityParams, "cloud": key name -> the
    oracle's CloudKey, "packing": handle -> (packing key, its key rows), "reenc": the re-encryption key}."""

    def __init__(self, O, keys, ring_memo=None):
        self.O, self.keys, self.p = O, keys, keys["params"]
        self.memo = {}
        # the rows of the ring steps: exact integers under (key or selector, operand row), which models of the same
        # keys may share (37 ms per key row of every evaluation)
        self.ring_memo = {} if ring_memo is None else ring_memo
        self.bootstraps = 0  # blind rotations the oracle ran
        self.ring_log = []  # (op, count, rows handed to the numpy model) of every ring step asked for
        self.ring_pool = None  # the sequence's "ring" pool (expected() sets it): see _ring
        self.rows_evaluated = 0  # rows _rowwise handed to its fn, in all
        self._switchers, self._selectors = {}, {}

    def _ring(self, key, op, a, x):
        """The TRLWE key switch under switching key `key` (trlwe_switch_model) and the packed CMUX under the step's one
        selector (cmux_model): exact in integers, row-wise in their ciphertexts, and no cloud key in them -- a Model with
        O = None and keys {"params", "switch": name -> key (k, basebit, t, mask_seed, bodies), "secrets"} answers them.
        An evaluation costs the negacyclic matrices of every key row whatever its rows, and the ring steps of a sequence
        share the ROWS_PER_STEP rows of the "ring" pool: a step that needs one of them under a key or selector takes the
        others along (`also`), so that no later step pays for that key again."""
        import cmux_model as CM
        import trlwe_switch_model as TM

        before = self.rows_evaluated
        pool = self.ring_pool
        if op == "trlwe_keyswitch":
            if key not in self._switchers:  # one per key
                sk = self.keys["switch"][key]
                assert sk.k == a["k"] and (sk.basebit, sk.t) == switch_key_gadget(key), (key, a)
                self._switchers[key] = TM.Switcher(TM.key_rows(sk.mask_seed, sk.k, sk.t, sk.bodies), sk.k, sk.basebit, sk.t)
            got = self._rowwise(("trlwe_keyswitch", key), self._switchers[key], [x[0].reshape(-1, 2, N)], memo=self.ring_memo,
                                also=None if pool is None else [pool])
        else:
            (basebit, t), rows = a["gadget"], np.ascontiguousarray(x[0][0], dtype=np.uint32)
            digest = hashlib.blake2b(rows.tobytes(), digest_size=16).digest()
            sig = ("cmux", basebit, t, a["reference"], a["d0"], digest)
            sel = self._selectors.pop((digest, basebit, t), None) or _Selector(CM, rows, basebit, t)
            self._selectors[(digest, basebit, t)] = sel  # the two used last: the steps of a sequence share one per gadget
            while len(self._selectors) > 2:
                self._selectors.pop(next(iter(self._selectors)))
            if a["d0"]:
                got = self._rowwise(sig, lambda d0, d1: sel.cmux(d0, d1, a["reference"]), [x[1].reshape(-1, 2, N), x[2].reshape(-1, 2, N)],
                                    memo=self.ring_memo, also=None if pool is None else [np.roll(pool, -1, axis=0), pool])  # (as _Gen.call pairs them)
            else:
                got = self._rowwise(sig, lambda d1: sel.external_product(d1, a["reference"]), [x[2].reshape(-1, 2, N)], memo=self.ring_memo,
                                    also=None if pool is None else [pool])
        self.ring_log.append((op, len(got), self.rows_evaluated - before))
        return got

    def _rowwise(self, sig, fn, operands, cost=0, memo=None, also=None):
        """fn over row-aligned operands ([count, ...] each), evaluated once per distinct row and tiled; memoised by
        (sig, row bytes).  cost: blind rotations of one row.  also: the rows (aligned like `operands`) that the rows of
        this call are drawn from: where every row still to evaluate is one of them, they are all evaluated with it."""
        memo = self.memo if memo is None else memo

        def digests_of(ops):
            flat = np.concatenate([np.ascontiguousarray(o).reshape(len(ops[0]), -1).astype(np.uint32) for o in ops], axis=1)
            return [hashlib.blake2b(r.tobytes(), digest_size=16).digest() for r in flat]

        digests = digests_of(operands)
        first = {}
        for j, d in enumerate(digests):
            first.setdefault(d, j)
        todo = [j for d, j in first.items() if (sig, d) not in memo]
        source = digests
        if todo and also is not None:
            more = digests_of(also)
            if {digests[j] for j in todo} <= set(more):
                operands, source = also, more
                todo = [j for j, d in enumerate(more) if (sig, d) not in memo and more.index(d) == j]
        if todo:
            keys = [source[j] for j in todo]
            got = fn(*[np.ascontiguousarray(o[todo]) for o in operands])
            self.bootstraps += cost * len(todo)
            self.rows_evaluated += len(todo)
            for k, d in enumerate(keys):
                memo[(sig, d)] = np.array(got[k])
        return np.stack([memo[(sig, d)] for d in digests])

    def _many(self, ck, prepared, tv, k, ks):
        from test_gpu_many_lut import many_model

        return np.ascontiguousarray(many_model(self.O, ck, prepared, tv, k, keyswitch=ks).transpose(1, 0, 2))

    def _mixed(self, ck, ks, codes, a, b):
        O, out = self.O, np.empty_like(a)
        for j, code in enumerate(codes.reshape(-1)):
            if ks:
                out[j] = O.batch_gate(ck, int(code), a[j], b[j])[0]
            else:
                out[j] = O.batch_bootstrap(ck, O.gate_prep(int(code), a[j], b[j], self.p.n), keyswitch=False)[0]
        return out

    def eval(self, key, handle, op, a, count, x, secret=None):
        """The words of `op` with arguments `a` on operands `x` under cloud key `key` on `handle`.  secret: the handle
        whose secret key an encrypting or decrypting call stages (its own, unless a racy stand-in says otherwise)."""
        if op in RING_OPS:
            return self._ring(key, op, a, x)
        from rs_tfhe_amd import packing as PK

        if op in NEW_FAMILIES:  # memoised whole: the stand-in, expected() and the calls made alone ask for the same step
            sig = (op, handle, secret or handle, key if a.get("ks") else None, count,
                   tuple(sorted((k, v) for k, v in a.items() if k not in NOTES)),
                   tuple(None if v is None else hashlib.blake2b(np.ascontiguousarray(v).tobytes(), digest_size=16).digest() for v in x))
            if sig not in self.memo:
                self.memo[sig] = np.ascontiguousarray(self._families(key, handle, op, a, count, x, secret or handle), dtype=np.uint32)
            return self.memo[sig].copy()

        O, p = self.O, self.p
        ck = self.keys["cloud"].get(key)
        sig = (key, op, tuple(sorted((k, v) for k, v in a.items() if k not in NOTES)))
        if op == "gate":
            return self._rowwise(sig, lambda u, v: O.batch_gate(ck, a["code"], u, v), x[:2], 1)
        if op == "gates_mixed":
            return self._rowwise(sig, lambda c, u, v: self._mixed(ck, a["ks"], c, u, v), [x[0].astype(np.uint32)[:, None], x[1], x[2]], 1)
        if op in ("bootstrap", "lincomb_bootstrap"):
            cts, tv = (x[0], x[1]) if op == "bootstrap" else (prep(x[0], x[1], a["ca"], a["cb"], a["cc"]), x[2])
            if a["tv"] == "per":
                return self._rowwise(sig, lambda u, t: O.batch_bootstrap(ck, u, t.reshape(-1, 2, N), keyswitch=a["ks"]), [cts, tv], 1)
            one = None if tv is None else tv[0]
            sig += (None if one is None else one.tobytes(),)
            return self._rowwise(sig, lambda u: O.batch_bootstrap(ck, u, one, keyswitch=a["ks"]), [cts], 1)
        if op == "tlwe_lincomb":
            return prep(x[0], x[1], a["ca"], a["cb"], a["cc"])
        if op == "lincomb_bootstrap_many":
            cts, tv = prep(x[0], x[1], a["ca"], a["cb"], a["cc"]), x[2][0]
            got = self._rowwise(sig + (tv.tobytes(),), lambda u: self._many(ck, u, tv, a["k"], a["ks"]), [cts], 1)
            return np.ascontiguousarray(got.transpose(1, 0, 2)).reshape(-1, p.n + 1)  # function-major
        if op == "mux":
            return self._rowwise(sig, lambda u, v, w: O.batch_mux(ck, u, v, w, a["naive"]), x[:3], 3)
        if op == "blind_rotate":
            one = None if x[1] is None else x[1][0]
            sig += (None if one is None else one.tobytes(),)
            return self._rowwise(sig, lambda u: O.batch_blind_rotate(ck, u, one), [x[0]], 1)
        if op == "identity_key_switch":
            return self._rowwise(sig, lambda u: O.batch_identity_key_switching(ck, u), [x[0]])
        if op == "sample_extract":
            return self._rowwise(sig, lambda u: np.stack([O.sample_extract_index(t.reshape(2, N), a["k"]) for t in u]), [x[0]])
        if op == "external_product":
            return self._rowwise(sig, lambda u, idx: np.stack([
                O.external_product_fft(ck.bootstrapping_key[int(i)], t.reshape(2, N), p.l, p.bgbit, ck.decomposition_offset)
                for t, i in zip(u, idx.reshape(-1))]), [x[0], x[1].astype(np.uint32)[:, None]])
        if op in ("pack", "pack_table"):
            pk, rows = self.keys["packing"][handle]
            with _deduped_contraction(PK):
                if op == "pack":
                    return PK.pack_model(p, pk.mask_seed, pk.bodies, x[0], rows=rows)
                return PK.table_model(p, pk.mask_seed, pk.bodies, x[0].reshape(a["m"], count, -1), a["m"], rows=rows)
        if op == "unpack":
            trlwe = x[0].reshape(-1, 2, N)
            slots = np.arange(count) if x[1] is None else x[1].astype(np.int64)
            rows = PK.extract_rows(trlwe, slots)
            return self._rowwise(sig, lambda u: PK.key_switch_model(p, ck.key_switching_key, u), [rows])
        if op == "reencrypt":
            return self._rowwise(("reenc",), lambda u: O.reencrypt_tlwe_lv0(self.keys["oracle_params"], self.keys["reenc"], u), [x[0]])
        if op == "expand_seeded":
            from rs_tfhe_amd.seeded import SeededCiphertexts

            return SeededCiphertexts(p, a["seed"], a["first"], x[0]).expand()
        raise ValueError(op)

    def _families(self, key, handle, op, a, count, x, secret):
        """Encryption (sym_encrypt_model, packed_encrypt_model, pk_encrypt_model: the keyed formats term by term, real
        noise), decryption (client.SecretKey's phases and decodes) and the linear layers (linear's definitions)."""
        import packed_encrypt_model as PEM
        import pk_encrypt_model as PM
        import sym_encrypt_model as SM
        from rs_tfhe_amd import linear as L
        from rs_tfhe_amd import packing as PK
        from rs_tfhe_amd.seeded import SeededPackedCiphertexts

        p = self.p
        sec = self.keys["secrets"][secret]
        step = Step("call", handle, op, "host", count, args=a)
        x = shaped(step, x, p.n)
        if op == "encrypt":
            full, _ = SM.bulk(sec.key_lv0, x[0], a["first"], a["alpha"], a["mask_seed"], a["rng_key"])
            return join_parts({"full": [full], "bodies": [full[:, -1]], "both": [full, full[:, -1]]}[a["out"]])
        if op == "encrypt_trlwe":
            full, _ = PEM.encrypt(sec.key_lv1, x[0], a["words"], a["first"], a["alpha"], a["mask_seed"], a["rng_key"])
            return join_parts({"full": [full], "bodies": [full[:, 1]], "both": [full, full[:, 1]]}[a["out"]])
        if op == "encrypt_trgsw":
            import cmux_model as CM

            return CM.encrypt_trgsw(sec.key_lv1, x[0], a["gadget"][0], a["gadget"][1], a["alpha"], a["rng_key"], a["first"])[0]
        if op == "expand_seeded_trlwe":
            return SeededPackedCiphertexts(p, a["seed"], a["first"], x[0], count * N).expand()
        if op == "pk_encrypt":
            return PM.encrypt(self.keys["public"][handle], a["rng_key"], PM.row_indices(a["first"], count), x[0], a["alpha"])[0]
        if op == "decrypt":
            return decode(sec.phase(x[0]) if a["width"] == "lv0" else sec.phase_lv1(x[0]), a["mode"])
        if op == "decrypt_trlwe":
            return decode(sec.packed_phase(x[0], count), a["mode"])
        if op == "tlwe_matmul":
            return L.matmul_model(p, x[0], x[1], x[2])
        if op == "trlwe_matmul":
            rows = L.matmul_packed_model(p, x[0], x[1], x[2])
            if not a["ks"]:
                return rows
            return PK.key_switch_model(p, self.keys["cloud"][key].key_switching_key, rows.reshape(-1, N + 1))
        if op == "polymul":
            return L.polymul_model(x[0], x[1], x[2])
        if op == "conv2d":
            return L.conv2d_model(p, x[0], x[1], x[2], stride=a["shape"][5], padding=a["shape"][6])
        raise ValueError(op)


def _Selector(CM, rows, basebit, t):
    """cmux_model.Selector as it stands, keeping the halves of its rows' negacyclic matrices (32 MB a row) up to t = 6:
    the variants of a sequence's CMUX steps share one selector per gadget."""
    class Kept(CM.Selector):
        def halves(self, r):
            if self.t > 6:
                return CM.Selector.halves(self, r)
            if r not in self.kept:
                self.kept[r] = CM.Selector.halves(self, r)
            return self.kept[r]

    sel = Kept(rows, basebit, t)
    sel.kept = {}
    return sel


NEW_FAMILIES = SECRET_OPS + UNCLAIMED_OPS + ("pk_encrypt", "trlwe_matmul")
NOTES = ("grow", "alone", "chain", "t_grow", "ring_grow")  # what a step's args say about its place, not about its call


class _deduped_contraction:
    """packing.contraction is row-wise: inside, it runs once per distinct row (pack_model and table_model of 1300 rows
    drawn from three would otherwise spend seconds in the matmul)."""

    def __init__(self, PK):
        self.PK = PK

    def __enter__(self):
        self.orig = orig = self.PK.contraction

        def contraction(params, halves, cts):
            u, inv = np.unique(cts, axis=0, return_inverse=True)
            return orig(params, halves, u)[inv.reshape(-1)]

        self.PK.contraction = contraction

    def __exit__(self, *exc):
        self.PK.contraction = self.orig


def expected(sequence, O, keys, pools, model=None, perturb=None, secret_of=None, switch_of=None, only=None, donor_of=None):
    """Every call step's expected words: {step: words}.  A key-change step changes the key of V2 from that step on, a
    switch_key_change the switching key of its view for its k; a chained operand is the model's own result of the
    earlier step.  perturb=i: one operand of step i is changed (the body of every row moved by 1/2; every plaintext of an
    encrypting step; the message of a selector), in the model only.  secret_of: {step: handle} evaluates those
    secret-staging steps under that handle's secret key; switch_of: {step: name} those switches under that key;
    donor_of: {step: step} gives those steps the first rows of the other step's right words; only: the steps to
    evaluate (closed under chaining)."""
    model = model if model is not None else Model(O, keys)
    model.ring_pool = pools.get("ring")
    key = {"E": "K1", "V2": "K2/gen", "VR": "reenc"}
    held = switch_keys_after(sequence, -1)
    want = {}
    for st in sequence:
        if st.kind == "state":
            if st.op == "key_change":
                key[st.handle] = key_after(st)
            elif st.op == "switch_key_change":
                held[st.handle][st.args["k"]] = st.args["to"]
            continue
        if only is not None and st.i not in only:
            continue
        if st.i in (donor_of or {}):
            want[st.i] = donor_of["words"][donor_of[st.i]].reshape(-1, 2, N)[:st.count].copy()
            continue
        x = materialise(st, pools, want)
        if perturb == st.i and st.op == "encrypt_trgsw":
            x[0] = x[0].copy()
            x[0][:, 1] += 1
        elif perturb == st.i:
            k = next(k for k, v in enumerate(x) if v is not None and v.dtype == np.uint32)
            x[k] = x[k].copy()
            if x[k].ndim == 1:
                x[k] ^= np.uint32(1 << 31)
            else:
                x[k][..., -1] ^= np.uint32(1 << 31)
        n = keys["params"].n
        name = key[st.handle]
        if st.op == "trlwe_keyswitch":
            name = (switch_of or {}).get(st.i, held[st.handle][st.args["k"]])
        want[st.i] = np.ascontiguousarray(model.eval(name, st.handle, st.op, st.args, st.count, x,
                                                     (secret_of or {}).get(st.i)),
                                          dtype=np.uint32).reshape(out_shape(st, n))
    return want


def compare(got, want):
    """The steps whose words differ (every row of every step; a missing or misshapen result differs)."""
    bad = []
    for i in sorted(want):
        g = got.get(i)
        if g is None or g.shape != want[i].shape or not np.array_equal(g, want[i]):
            bad.append(i)
    assert set(got) == set(want), (sorted(got), sorted(want))
    return bad


def describe(sequence, bad, got=None, want=None):
    lines = []
    for i in bad:
        line = repr(sequence[i])
        if got is not None and i in got and got[i].shape == want[i].shape:
            rows = np.flatnonzero((got[i] != want[i]).reshape(len(got[i]), -1).any(axis=1))
            line += f": {len(rows)} of {len(got[i])} rows differ (first {rows[:6].tolist()})"
        lines.append(line)
    return "\n".join(lines)


# ---- plaintexts (a check that does not depend on the device) --------------------------------------------------------------
def _signed(words):
    """torus differences as signed LSB"""
    return (np.asarray(words, np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)


def _negacyclic(poly):
    """T [N][N] int64 with (poly(X) * x(X) mod X^N + 1)[i] = sum_k T[i][k] x[k]"""
    i, k = np.arange(N)[:, None], np.arange(N)[None, :]
    return np.where(k > i, -1, 1) * np.asarray(poly, np.int64)[(i - k) % N]


def chains_decrypt_to_their_plaintext_products(shape, secrets, seq, got, pools, which=("C", "D", "E", "F")):
    """No device and no library in the reference: the phases a chain ends in -- as its decrypting link returned them and
    as the secret key reads them on the CPU off the chain's last ciphertexts -- are W plain + bias (C), the matrix times
    the slots of the polynomial product of the plaintexts (D), psi_3 of the plaintext slots (E), psi_2047 of the words of
    the operand the encrypted bit selects (F), mod 2^32.  Allowed error: 8 sigma.  C and D: the sum of the independent
    Gaussians the fresh encryptions carry, sigma = alpha 2^32 sqrt(sum of the squared weights each noise sample reaches
    the output row with), derived per row below.  E and F: sigma^2 = alpha_lv1^2 (the encryption of the words that come
    through) + trlwe_switch_model.switch_variance of the switching key in force at the chain's switch + (F)
    cmux_model.cmux_variance of the selector's gadget and bit -- the formulas test_trlwe_switch_host.py and
    test_cmux_host.py hold to samples.  A failure chance below 1e-12 over the corpus.  `secrets`: handle -> the client
    secret key.  Returns the chains checked."""
    import cmux_model as CM
    import trlwe_switch_model as TM

    done = 0
    for name, n_links in (("C", 3), ("D", 4), ("E", 3), ("F", 4)):
        if name not in which:
            continue
        links = [st for st in seq if st.kind == "call" and st.args.get("chain") == name]
        assert len(links) == n_links, (name, links)
        sk, enc, dec = secrets[links[0].handle], links[0], links[-1]
        if name in ("E", "F"):
            ks = links[-2]
            alpha = shape.alpha_lv1
            basebit, t = switch_key_gadget(switch_keys_after(seq, ks.i)[ks.handle][ks.args["k"]])
            var = alpha * alpha + TM.switch_variance(basebit, t, alpha)
            if name == "E":
                slots = np.zeros(2 * N, np.uint32)
                slots[:enc.args["words"]] = enc.ins[0][1]
            else:
                bit, mux = enc.args["mu"][0][0], links[1]
                slots = pools["genwords:" + mux.handle][mux.ins[2 if bit else 1][2]]
                var += CM.cmux_variance(mux.args["gadget"][0], mux.args["gadget"][1], alpha, mu=bit)
            want = TM.psi(slots.reshape(2, N), ks.args["k"]).reshape(-1).astype(np.int64)
            bound = 8.0 * 4294967296.0 * np.sqrt(var)
            for who, ph in (("decrypt_trlwe_dev", got[dec.i]), ("the secret key on the CPU", sk.packed_phase(got[ks.i], 2 * N))):
                err = np.abs(_signed(np.asarray(ph, np.int64).reshape(-1) - want))
                assert (err <= bound).all(), f"chain {name} ({who}): {int(err.max())} LSB off, {float(bound):.1f} allowed; {dec}"
            done += 1
            continue
        mm = links[-2]
        rows, cols, groups = mm.args["shape"]
        W, bias = mm.ins[0][1].astype(np.int64), mm.ins[2][1].astype(np.int64)
        if name == "C":
            x = enc.ins[0][1][:groups * cols].astype(np.int64).reshape(groups, cols)  # the plaintexts the matrix takes
            want = x @ W.T + bias[None, :]
            sumsq = np.broadcast_to((W ** 2).sum(axis=1).astype(np.float64), (groups, rows))
            alpha, cpu = shape.alpha_lv0, sk.phase(got[mm.i])
        else:
            poly = links[1]
            p_rows, p_cols, p_groups = poly.args["shape"]
            slots = np.zeros(p_groups * p_cols * N, np.int64)
            slots[:enc.args["words"]] = enc.ins[0][1]
            slots = slots.reshape(p_groups, p_cols, N)
            wp, bp = poly.ins[0][1], poly.ins[2][1].astype(np.int64)
            T = [[_negacyclic(wp[r, c]) for c in range(p_cols)] for r in range(p_rows)]
            Wpad = np.zeros((rows, N), np.int64)
            Wpad[:, :cols] = W
            want = np.empty((groups, rows), np.int64)
            sumsq = np.empty((groups, rows), np.float64)
            for g in range(p_groups):
                for r in range(p_rows):
                    pt = (sum(T[r][c] @ slots[g, c] for c in range(p_cols)) + bp[r]) % (1 << 32)  # slots of the product
                    want[g * p_rows + r] = Wpad @ pt + bias
                    # noise sample k of input polynomial c reaches output row q with weight (Wpad @ T[r][c])[q][k]
                    sumsq[g * p_rows + r] = sum(((Wpad @ T[r][c]).astype(np.float64) ** 2).sum(axis=1) for c in range(p_cols))
            alpha, cpu = shape.alpha_lv1, sk.phase_lv1(got[mm.i])
        bound = 8.0 * alpha * 4294967296.0 * np.sqrt(sumsq)
        for who, ph in (("decrypt_dev", got[dec.i]), ("SecretKey on the CPU", cpu)):
            err = np.abs(_signed(ph.reshape(groups, rows).astype(np.int64) - want))
            assert (err <= bound).all(), f"chain {name} ({who}): {int(err.max())} LSB off, {float(bound.min()):.1f} allowed; {dec}"
        done += 1
    return done



def plaintext(st, pools, O):
    """The booleans a bootstrap-type step on genuine encryptions must decrypt to, or None where the step has no such
    reading (a table of random words, chained or linear operands, no key switch)."""
    if st.kind != "call" or st.sources or st.handle == "VR":
        return None
    bits = pools["bits:" + st.handle]

    def of(k):
        return bits[st.ins[k][2]]

    truth = dict(O.GATE_TRUTH)
    truth[O.GATE_COPY] = lambda a, b: a
    if st.op == "gate":
        return np.array([truth[st.args["code"]](a, b) for a, b in zip(of(0), of(1))], bool)
    if st.op == "gates_mixed" and st.args["ks"]:
        return np.array([truth[int(c)](a, b) for c, a, b in zip(st.ins[0][1], of(1), of(2))], bool)
    if st.op == "bootstrap" and st.args["tv"] is None and st.args["ks"]:
        return of(0).copy()
    if st.op == "mux" and st.args["naive"]:  # (Gates::mux in the reference's own formula carries no decrypt claim)
        return np.where(of(0), of(1), of(2))
    return None
