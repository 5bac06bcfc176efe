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

What is narrower than the full cross product: the pinned form (every operand and the output from pinned_empty, the
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
             "load_packing_key", "key_change")
COEFS = (1, 2, 3, M32, M32 - 1)


class Shape:
    """A parameter shape of the fuzz: its name, n, the counts, whether the oracle gives words (`exact`), and whether
    the tree bootstrap runs (UINT4 only)."""

    def __init__(self, name, n, counts, exact, bivariate):
        self.name, self.n, self.counts, self.exact, self.bivariate = name, n, tuple(counts), exact, bivariate

    def __repr__(self):
        return f"Shape({self.name})"


SHAPES = {
    "SECURITY_128_BIT": Shape("SECURITY_128_BIT", 700, BASE_COUNTS, True, False),
    # l = 1, general rounding, base 32: the column-sliced key switch from ks_sl_chunk_min = 384 rows on
    "SECURITY_UINT4": Shape("SECURITY_UINT4", 820, BASE_COUNTS + (383, 384, 400), False, True),
}
STEPS = 40
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
    return v


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
    return op


def forms_of(op):
    if op in STAGE_OPS:
        return ("host",)
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
        return 0

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
            return f"<{self.i} {self.handle}.{self.op} {self.args if self.op == 'key_change' else ''}>"
        return f"<{self.i} {self.handle}.{variant_name(self.op, self.args)} {self.form} x{self.count} from {self.sources}>"


# ---- the generator ----------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, seed, shape, steps):
        self.seed, self.shape, self.steps = seed, shape, steps
        self.rng = np.random.default_rng([0x5E9F, seed, shape.n])
        self.seq = []
        self.changes = 0
        self.v2_pending = set()  # streams that carry V2 work no step has drained yet

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
        else:
            raise ValueError(op)
        return self.add(Step("call", handle, op, form, count, ins, args))

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
        if prev is not None and prev.dev and (not min_ks_rows or prev.ks_rows >= min_ks_rows):
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

    def grow(self):
        """A call of at least twice any earlier count, directly after un-synchronised device work."""
        self.dev_before()
        # 1.5 x the grow step of the seed before (ensure() keeps a quarter of headroom): a context that runs the corpus
        # seed after seed reallocates at every grow step, not only at the first
        count = max(2 * max(s.count for s in self.seq), int(np.ceil(2 * max(self.shape.counts) * 1.5 ** self.seed)))
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
        else:  # lincomb_dev -> bootstrap_dev
            links = [("tlwe_lincomb", {}), ("bootstrap", {"tv": "one", "ks": True})]
        src = None
        for op, args in links:
            src = self.call(handle, op, args, stream, count, src).i
            yield

    def run(self):
        vs = variants(self.shape)
        order = np.random.default_rng([0xDEC4, self.shape.n]).permutation(len(vs))
        fixed = ["profiling_on", "kernel_times", "profiling_off", "kernel_times", "combining_off", "combining_default",
                 "synchronize", "load_packing_key", "key_change", "key_change", "grow", "pair", "A", "B"]
        budget = {"A": 3, "B": 2}
        n_deck = self.steps - sum(budget.get(f, 1) for f in fixed)
        # where the fixed items go among the deck's draws: the profiling and combining steps keep their order, the
        # others go anywhere, the grow step into the second half
        plan = dict()
        for pos, item in zip(np.sort(self.rng.integers(1, n_deck, 6)), fixed[:6]):
            plan.setdefault(int(pos), []).append(item)
        for item in fixed[6:]:
            pos = self.rng.integers(n_deck // 2 if item == "grow" else 1, n_deck)
            plan.setdefault(int(pos), []).append(item)
        open_chains = []
        for j in range(n_deck):
            for item in plan.get(j, []):
                if item in ("A", "B"):
                    ch = self.chain(item)
                    next(ch)
                    open_chains.append(ch)
                elif item == "grow":
                    self.grow()
                elif item == "pair":
                    self.pair()
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
    for prev, st in zip([None] + sequence[:-1], sequence):
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
        if not prev.dev:
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


def sum_counts(dicts):
    out = {}
    for d in dicts:
        for k, v in d.items():
            out[k] = out.get(k, 0) + v
    return out


# ---- operands ---------------------------------------------------------------------------------------------------------
def words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


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


def out_shape(st, n):
    c, a = st.count, st.args
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
    """cuda:0 through torch: 32-bit words travel as int32 tensors, gate codes as uint8."""

    def __init__(self):
        import torch

        self.torch = torch
        self.dev = torch.device("cuda:0")

    def streams(self):
        return [None, self.torch.cuda.Stream(device=0), self.torch.cuda.Stream(device=0)]

    def upload(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int32)).to(self.dev)

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

    def __init__(self, arr):
        self.arr = arr


class FakeBackend:
    def __init__(self, on_synchronize=None):
        self.on_synchronize = on_synchronize

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
        pass

    def pinned_copy(self, a):
        return np.array(a)

    def pinned_empty(self, shape):
        return np.empty(shape, np.uint32)


# ---- the executor -------------------------------------------------------------------------------------------------------
def _host_call(h, st, x, backend):
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
    raise ValueError(op)


class SeededBodies:
    """What Engine.expand_seeded reads of a seeded.SeededCiphertexts."""

    def __init__(self, params, mask_seed, first_index, bodies):
        self.params, self.mask_seed, self.first_index, self.bodies = params, mask_seed, first_index, bodies


def _dev_call(h, st, t, out, stream):
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
    else:
        raise ValueError(st.op)


def run(sequence, handles, streams, pools, backend=None):
    """Make the calls in order, with no synchronisation between steps.  handles: {"E", "V2", "VR": Engine-shaped
    handles; "book": key name -> what each key-change route loads; "packing": handle -> its packing key;
    "combining_default": the context's default}.  Before the first step every fresh operand is uploaded (or copied to
    pinned memory), every _dev step gets an output tensor of its own, and the device is synchronised once; host results
    are kept as returned; device results are read after the last step and one device-wide synchronisation.
    Returns ({step: words}, info)."""
    be = backend if backend is not None else TorchBackend()
    n = handles["E"].params.n
    staged, outs, results = {}, {}, {}
    info = {"kernel_times": [], "seconds": 0.0}
    for st in sequence:
        if st.kind != "call":
            continue
        x = materialise(st, pools)
        if st.dev:
            staged[st.i] = [None if v is None else be.upload(v) for v in x]
            outs[st.i] = be.empty(out_shape(st, n))
        else:
            staged[st.i] = [None if v is None else be.pinned_copy(v) for v in x] if st.form == "pinned" else x
    assert len({id(o) for o in outs.values()}) == len(outs)
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
            _dev_call(h, st, x, outs[st.i], streams[st.stream])
        else:
            results[st.i] = np.ascontiguousarray(_host_call(h, st, x, be), dtype=np.uint32).reshape(out_shape(st, n))
            if st.args.get("alone"):
                h.synchronize()
    be.synchronize()
    info["seconds"] = time.perf_counter() - t0
    for i, t in outs.items():
        results[i] = be.download(t).reshape(out_shape(sequence_step(sequence, i), n))
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


EXPECTED_FLAGS = {"E": (1, 0, 1), "V2": (1, 0, 1), "VR": (0, 1, 0)}  # key / re-encryption key / packing key loaded


def flags(handle):
    lib, ctx = handle._lib, handle._member_ctx(0)
    return (lib.tfhe_hip_key_is_loaded(ctx), lib.tfhe_hip_reenc_key_is_loaded(ctx), lib.tfhe_hip_packing_key_is_loaded(ctx))


# ---- the model ----------------------------------------------------------------------------------------------------------
def prep(a, b, ca, cb, cc):
    p = (np.uint32(ca) * a + np.uint32(cb) * b).astype(np.uint32)
    p[..., -1] += np.uint32(cc)
    return p


class Model:
    """The words of one call under one key.  keys: {"params": the product's SecurityParams, "cloud": key name -> the
    oracle's CloudKey, "packing": handle -> (packing key, its key rows), "reenc": the re-encryption key}."""

    def __init__(self, O, keys):
        self.O, self.keys, self.p = O, keys, keys["params"]
        self.memo = {}
        self.bootstraps = 0  # blind rotations the oracle ran

    def _rowwise(self, sig, fn, operands, cost=0):
        """fn over row-aligned operands ([count, ...] each), evaluated once per distinct row and tiled; memoised by
        (sig, row bytes).  cost: blind rotations of one row."""
        count = len(operands[0])
        flat = np.concatenate([np.ascontiguousarray(o).reshape(count, -1).astype(np.uint32) for o in operands], axis=1)
        digests = [hashlib.blake2b(r.tobytes(), digest_size=16).digest() for r in flat]
        first = {}
        for j, d in enumerate(digests):
            first.setdefault(d, j)
        todo = [j for d, j in first.items() if (sig, d) not in self.memo]
        if todo:
            got = fn(*[np.ascontiguousarray(o[todo]) for o in operands])
            self.bootstraps += cost * len(todo)
            for k, j in enumerate(todo):
                self.memo[(sig, digests[j])] = np.array(got[k])
        return np.stack([self.memo[(sig, d)] for d in digests])

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

    def eval(self, key, handle, op, a, count, x):
        """The words of `op` with arguments `a` on operands `x` under cloud key `key` on `handle`."""
        from rs_tfhe_amd import packing as PK

        O, p = self.O, self.p
        ck = self.keys["cloud"].get(key)
        sig = (key, op, tuple(sorted((k, v) for k, v in a.items() if k not in ("grow", "alone"))))
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


def expected(sequence, O, keys, pools, model=None, perturb=None):
    """Every call step's expected words: {step: words}.  A key-change step changes the key of V2 from that step on; a
    chained operand is the model's own result of the earlier step.  perturb=i: one operand of step i is changed (the
    body of every row moved by 1/2), in the model only."""
    model = model if model is not None else Model(O, keys)
    key = {"E": "K1", "V2": "K2/gen", "VR": "reenc"}
    want = {}
    for st in sequence:
        if st.kind == "state":
            if st.op == "key_change":
                key[st.handle] = key_after(st)
            continue
        x = materialise(st, pools, want)
        if perturb == st.i:
            k = next(k for k, v in enumerate(x) if v is not None and v.dtype == np.uint32 and v.ndim >= 2)
            x[k] = x[k].copy()
            x[k][..., -1] ^= np.uint32(1 << 31)
        n = keys["params"].n
        want[st.i] = np.ascontiguousarray(model.eval(key[st.handle], st.handle, st.op, st.args, st.count, x),
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
