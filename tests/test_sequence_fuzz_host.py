"""The sequence fuzz without a device (tests/sequence_fuzz.py): the generator is deterministic, the corpus the GPU tests
run holds every condition they rely on, the executor and the model agree on a faithful stand-in handle (every call
evaluated at call time by the same SF.Model.eval that expected() uses, so this holds the executor's plumbing -- routing,
chaining, tiling, key tracking, buffer use -- and NOT the model's own formulas, which only the GPU run at
SECURITY_128_BIT holds to the device), and the comparison fails -- at exactly the clobbered steps -- on a stand-in
that shares one key-switch scratch among its calls, and on one that shares its buffer of staged secrets without a claim.

The ring steps (the TRLWE key switch, the packed CMUX, TRGSW encryption, switch_key_change, ring_times): the stand-in
holds a switching key per k, evaluates a switch under the key held at call time, counts the chunk passes issued while
profiling is on, and every route of a key change drains it as the library's does.  Two more racy devices:
"ring_scratch" shares each family's digit scratch without a claim (a pending ring _dev call gives the first rows of the
family's most recent result of at least its size), "switch_table" replaces a switching key without draining (an
undrained switch of that k on that view runs under the new key); each must be reported at exactly the steps read off the
sequence and their cones, and be right when every call is made alone.  The staged-secret device counts TRGSW encryption
among the calls that overwrite the secret (its device form never stays pending: it has finished on return).  Chains E
and F reach their 8 sigma on the numpy models alone for every sequence the GPU test runs (both shapes of the corpus, each
with its own alpha_lv1 and keys made on the CPU), each ring family reaches 2,049 ciphertexts and its own grow step in
every sequence, and a ring step hands the numpy model at most ROWS_PER_STEP rows whatever its count (counted where the
rows are handed over; exactly three for the 2,049-row step of each family on a model that has seen nothing).  The models
of this module share the ring rows they have evaluated (_RING_MEMO: exact integers under a key or selector and an operand
row).
The directed pair of test_gpu_sequence_fuzz.py for these calls (a host switch on V2 under an un-synchronised
trlwe_keyswitch_dev of the same k on E) measured 16,384 ciphertexts at 2.31 ms alone against 0.09 ms to issue, the first
call still running in all four rounds when the second was entered.

Narrower than the full cross product, as in sequence_fuzz.py: TRGSW encryption's device form has no stream; VR runs no
ring step; switching keys keep s_from = s_to."""
import numpy as np
import pytest

import sequence_fuzz as SF

N = 1024
# a small shape in the exact-product regime (log2(2l) + 10 + (bgbit - 1) + 31 < 51): oracle bootstraps of a millisecond
HOST = SF.Shape("SFUZZ_HOST", 16, SF.BASE_COUNTS, True, False, 2.0e-5, 2.0e-8)
HOST_SEEDS = (0, 1, 2)
_RING_MEMO = {}  # the ring rows every model of this module shares: each (key or selector, row) is evaluated once


# ---- the generator and the corpus ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SF.SHAPES))
def test_same_seed_same_sequence(name):
    a, b, c = SF.random_sequence(3, name), SF.random_sequence(3, name), SF.random_sequence(4, name)
    assert [s.key() for s in a] == [s.key() for s in b]
    assert [s.key() for s in a] != [s.key() for s in c]
    assert SF.STEPS <= len(a) <= SF.STEPS + 16
    assert [s.i for s in a] == list(range(len(a)))


@pytest.mark.parametrize("name", sorted(SF.SHAPES))
def test_corpus_condition(name):
    shape = SF.SHAPES[name]
    seqs = SF.corpus(name)
    assert len(seqs) == 6
    c = SF.sum_counts(SF.adjacency(s) for s in seqs)
    need = ["dev then host", "dev then dev on another stream", "dev then grow", "stage op under a running key switch",
            "key switch of 384 rows or more under a running key switch",
            "V2 after E", "E after V2", "chained pack", "chained unpack", "chained bootstrap",
            "secret-staging call after a secret-staging dev call on another stream",
            "secret-staging host call after a secret-staging dev call",
            "secret-staging call on V2 after a secret-staging dev call on E",
            "secret-staging call on E after a secret-staging dev call on V2",
            "trlwe_matmul:ks under a running key switch", "key switch after a running trlwe_matmul:ks dev",
            "pk_encrypt after a dev call on another stream", "pk_encrypt on V2 after key_change",
            "unclaimed call between two claiming dev calls on other streams",
            "chained tlwe_matmul", "chained polymul", "chained trlwe_matmul", "chained decrypt"]
    need += ["dev then " + op for op in SF.STATE_OPS] + ["state " + op for op in SF.STATE_OPS]
    need += ["op " + SF.variant_name(op, args) for op, args in SF.variants(shape)]
    need += ["form " + f for f in SF.FORMS] + ["route " + r for r in SF.ROUTES]
    need += SF.ring_orders()  # the orders of the TRLWE key switch, the packed CMUX, TRGSW encryption and the switching keys
    short = {k: c.get(k, 0) for k in need if c.get(k, 0) < 3}
    assert not short, short
    assert len(set(need)) == len(need) and {"op " + SF.variant_name(*v) for v in SF.ring_variants()} <= set(need)
    # every ordered pairing of an encrypting and a decrypting secret-staging call
    kinds = [f"secret-staging {b} after {a}" for a in ("enc", "dec") for b in ("enc", "dec")]
    assert all(c.get(k, 0) >= 1 for k in kinds), {k: c.get(k, 0) for k in kinds}
    tables = {op: set() for op in SF.TABLE}
    for seq in seqs:
        for st in seq:
            if st.kind != "call":
                continue
            assert st.form in SF.forms_of(st.op) and st.count >= 1
            if st.op in SF.TABLE:  # the step's shape is one of the table (chain D's matrix takes four groups)
                assert st.args["shape"] in SF.TABLE[st.op] or (st.args.get("chain") == "D" and st.args["shape"] == SF.CHAIN_D_MATMUL)
                tables[st.op].add(st.args["shape"])
            elif st.op == "encrypt_trlwe":  # plaintext words; the count is the groups
                assert st.args["words"] in shape.counts or st.args.get("chain") in ("D", "E")
                assert st.count == -(-st.args["words"] // N)
            elif st.op == "expand_seeded_trlwe":
                assert st.count in (1, 2)
            elif st.op == "decrypt_trlwe" and st.sources:  # the last link of chains E and F: every slot of two groups
                assert st.count == 2 * N and st.args["chain"] in ("E", "F")
            elif st.op == "decrypt_trlwe":
                assert st.count % N and len(st.ins[0][2]) == -(-st.count // N)
            elif st.ring:  # the ring counts (63 / 64 / 65 around the GEMM's 64-row block through 33, 64, 65), or a second pass
                assert st.count in SF.RING_COUNTS + (SF.RING_BIG,) and st.form in ("host", "dev0", "dev1", "dev2")
            else:
                assert st.count in shape.counts or st.args.get("grow") or st.args.get("chain") in ("C", "D")
                assert st.op != "encrypt_trgsw" or st.count <= 5
            if st.op == "pk_encrypt":
                assert st.count <= 520
            if st.op in ("encrypt", "encrypt_trlwe", "pk_encrypt", "encrypt_trgsw"):  # real noise, and no sample two f64 forms may round apart
                assert st.args["alpha"] == (shape.alpha_lv1 if st.op in ("encrypt_trlwe", "encrypt_trgsw") else shape.alpha_lv0) > 0
                assert not SF.encrypt_border(st.op, st.args["rng_key"], st.args["first"], st.count, st.args["alpha"],
                                             st.args.get("gadget")).any(), st
            if st.op == "encrypt_trgsw":  # a bit times a monomial per selector
                mu = st.ins[0][1]
                assert mu.shape == (st.count, N) and mu.dtype == np.int32 and set(np.unique(mu)) <= {0, 1} and (mu.sum(axis=1) <= 1).all()
                assert st.args["gadget"] in SF.TRGSW_GADGETS
            if st.op == "cmux":
                assert st.args["gadget"] in SF.CMUX_GADGETS and (st.ins[1] is not None) == st.args["d0"]
            if st.op in SF.NEW_FAMILIES:
                assert st.handle != "VR"
            for spec in st.ins:  # weights: int8 with both ends of the range
                if spec is not None and spec[0] == "i8":
                    assert spec[1].dtype == np.int8 and (spec[1].size == 1 or (spec[1].min(), spec[1].max()) == (-128, 127))
            for j in st.sources:  # a chained operand: an earlier _dev step on the same stream and handle
                assert j < st.i and seq[j].dev and st.dev and seq[j].handle == st.handle
                # the one exception: TRGSW encryption's device form names no stream and has finished when it returns, so
                # the step chained from its selector may run on any stream
                assert seq[j].stream == st.stream or (seq[j].op == "encrypt_trgsw" and not seq[j].queued)
            assert (st.op == "reencrypt") == (st.handle == "VR")
        # a key change on V2 drains V2's own streams and nothing else
        pending = set()
        for st in seq:
            if st.handle == "V2" and st.dev:
                pending.add(st.stream)
            if st.kind == "state" and st.op == "key_change":
                assert st.handle == "V2" and set(st.args["wait"]) == pending
                pending = set()
    assert all(tables[op] >= set(SF.TABLE[op]) for op in SF.TABLE), tables
    firsts = {st.args["first"] >> 32 != 0 for seq in seqs for st in seq if st.kind == "call" and st.op in ("encrypt", "encrypt_trlwe")}
    assert firsts == {False, True}  # first indices small and above 2^32
    # each ring family reaches RING_BIG = 2,049 ciphertexts, a second chunk pass (once a sequence, and three times over
    # the shape at the least)
    for op in SF.RING_OPS:
        big = [sum(st.op == op and st.count == SF.RING_BIG and st.passes == 2 for st in seq) for seq in seqs]
        assert sum(big) >= 3 and min(big) >= 1, (op, big)
    counts = {st.count for seq in seqs for st in seq if st.kind == "call"}
    assert set(shape.counts) <= counts  # every count, on UINT4 both sides of ks_sl_chunk_min = 384
    # the grow steps rise from seed to seed by more than the quarter of headroom ensure() allocates: a context shared by
    # the corpus, run seed after seed, reallocates at each of them
    grows = [next(st.count for st in seq if st.args.get("grow")) for seq in seqs]
    assert all(b > 1.25 * a for a, b in zip(grows, grows[1:])) and grows[0] >= 2 * max(shape.counts), grows


# ---- stand-in handles ---------------------------------------------------------------------------------------------------
class _Tag:
    def __init__(self, name):
        self.name = name


class _World:
    """What the stand-in handles of one run share: the model that evaluates their calls, the order of the calls, the
    log of key switches and the device outputs still to be read back."""

    def __init__(self, model, n, racy, secrets=None):
        # racy: False, "key_switch", "secret", "ring_scratch" or "switch_table"
        self.model, self.n, self.racy = model, n, racy
        self.secrets = secrets or {}
        self.order = 0
        self.key_switches = []  # (order, rows, words [rows][n+1])
        self.dev_outs = []  # (order, rows, FakeTensor)
        self.log = []  # every _dev call, in order: what read_back needs to evaluate it again
        self.pending = []  # the secret-staging _dev calls no synchronisation has drained yet
        self.ring = []  # the ring _dev calls (entries of the log) no synchronisation has drained yet
        self.profiling = False
        self.passes = {op: 0 for op in SF.RING_OPS}  # chunk passes issued while profiling was on, since the last getter

    def secret_name(self, key):
        """The handle whose secret key a call was given (key_lv0 or key_lv1)"""
        for name in ("E", "V2"):
            sk = self.secrets[name]
            if any(len(k) == len(key) and np.array_equal(k, key) for k in (sk.key_lv0, sk.key_lv1)):
                return name
        raise AssertionError("a key of no handle")

    def staged(self, entry, secret, dev):
        """A secret-staging call.  The racy device has ONE buffer of staged secrets and no claim on it: the kernels of
        the _dev calls still pending read what the last call before the next synchronisation staged."""
        for e in self.pending:
            e["wrong"] = secret
        if dev:
            self.pending.append(entry)

    def queued(self, stream):
        """A _dev call on `stream`: the stream's order holds the ring calls before it on that stream."""
        for e in self.ring:
            if e["stream"] == stream:
                e["covered"] = True

    def ring_call(self, op, count, words, entry):
        """A ring call (entry: its log entry, None for a host form).  The racy device "ring_scratch" shares each family's
        digit scratch without a claim: a _dev call of the family still pending -- its stream not synchronised and no later
        call on it -- reads the digits of the most recent call of the family of at least its size."""
        for e in self.ring:
            if e["op"] == op and e["count"] <= count and not e["covered"]:
                e["donor"] = words
        if entry is not None:
            entry["covered"], entry["donor"] = False, None
            self.ring.append(entry)

    def switch_key_changed(self, handle, k, name):
        """The racy device "switch_table" replaces the rows of a switching key without draining the device: every
        trlwe_keyswitch_dev of that k on that view that no synchronisation has drained runs under the new key."""
        if self.racy != "switch_table":
            return self.synchronized()
        for e in self.ring:
            if e["op"] == "trlwe_keyswitch" and e["name"] == handle and e["args"]["k"] == k:
                e["wrong_key"] = name

    def synchronized(self, stream="all"):
        self.pending = [e for e in self.pending if stream != "all" and e["stream"] != stream]
        self.ring = [e for e in self.ring if stream != "all" and e["stream"] != stream]

    def read_back(self):
        """The racy devices.  "key_switch": every _dev result that went through the key switch's scratch reads as the
        most recent key switch of at least its size.  "secret": every pending secret-staging _dev call ran under the key
        staged last.  "ring_scratch": every pending ring _dev call gives the first rows of the family's most recent
        result of at least its size.  "switch_table": every undrained switch ran under the key that replaced its own.
        What was chained from a wrong step follows it."""
        self.synchronized()
        if self.racy == "key_switch":
            for order, rows, t in self.dev_outs:
                donor = [k for k in self.key_switches if k[1] >= rows][-1]
                if donor[0] != order:
                    t.arr[...] = donor[2][:rows].reshape(t.arr.shape)
        if self.racy in ("secret", "ring_scratch", "switch_table"):
            dirty = set()
            for e in self.log:
                wrong = self.racy == "secret" and e["wrong"] not in (None, e["secret"])
                donor = e.get("donor") if self.racy == "ring_scratch" else None
                key = e.get("wrong_key") if self.racy == "switch_table" else None
                if not wrong and donor is None and key is None and \
                        not any(isinstance(o, SF.FakeTensor) and id(o.root) in dirty for o in e["operands"]):
                    continue
                if donor is not None:
                    got = donor.reshape(len(donor), -1)[:e["count"]]
                else:
                    x = [o.arr if isinstance(o, SF.FakeTensor) else o for o in e["operands"]]
                    got = self.model.eval(key or e["key"], e["name"], e["op"], e["args"], e["count"], x, e["wrong"] if wrong else e["secret"])
                e["write"](np.ascontiguousarray(got, dtype=np.uint32))
                dirty |= {id(o.root) for o in e["outs"]}


class StandIn:
    """An Engine-shaped handle that evaluates each call with SF.Model.eval at call time, under the key it holds then
    (the model expected() uses: an error inside the model is invisible here)."""

    def __init__(self, world, name, params, key, switch=None):
        self.world, self.name, self.params, self.key = world, name, params, key
        self.switch = dict(switch or {})  # k -> the name of the switching key held
        self.calls = []

    def _do(self, op, args, operands, out=None, count=None, form="host", aux=None, secret=None, stream=None, key=None):
        w = self.world
        x = [o.arr if isinstance(o, SF.FakeTensor) else o for o in operands]
        count = len(x[0]) if count is None else count
        key = self.key if key is None else key
        got = np.ascontiguousarray(w.model.eval(key, self.name, op, args, count, x, secret), dtype=np.uint32)
        w.order += 1
        rows = SF.Step("call", self.name, op, form, count, args=args).ks_rows
        if rows:
            w.key_switches.append((w.order, rows, got.reshape(-1, w.n + 1).copy()))
        self.calls.append(op)
        outs = [o for o in (out, aux) if o is not None]

        def write(words):
            if len(outs) == 2:  # full and bodies of one encrypting call, side by side in the model's words
                words = words.reshape(len(words), -1)
                split = outs[0].arr.size // len(words)
                outs[0].arr[...] = words[:, :split].reshape(outs[0].arr.shape)
                outs[1].arr[...] = words[:, split:].reshape(outs[1].arr.shape)
            else:
                outs[0].arr[...] = words.reshape(outs[0].arr.shape)

        entry = {"name": self.name, "key": key, "op": op, "args": args, "count": count, "operands": operands, "outs": outs,
                 "secret": secret, "wrong": None, "stream": stream, "write": write}
        if op in SF.SECRET_OPS:  # (TRGSW encryption has finished when it returns: it clobbers, and never stays pending)
            w.staged(entry, secret, bool(outs) and op != "encrypt_trgsw")
        if outs and op != "encrypt_trgsw":
            w.queued(stream)
        if op in SF.RING_OPS:
            w.ring_call(op, count, got.copy(), entry if outs else None)
            if w.profiling:
                w.passes[op] += -(-count // SF.RING_CHUNK)
        if not outs:
            return got
        for o in outs:
            assert isinstance(o, SF.FakeTensor) and (o.arr == SF.FILL).all(), "an output buffer was used twice"
        write(got)
        w.log.append(entry)
        if rows:
            w.dev_outs.append((w.order, rows, out))

    @staticmethod
    def _tv(testvec, per_ct):
        """(the tables as [.][2][N], "per" / "one" / None) of a test-vector argument."""
        if testvec is None:
            return None, None
        t = testvec.arr if isinstance(testvec, SF.FakeTensor) else np.asarray(testvec)
        return t.reshape(-1, 2, N), "per" if per_ct else "one"

    # -- host forms
    def batch_gate(self, gate, a, b=None, out=None):
        got = self._do("gate", {"code": gate}, [a, b])
        if out is not None:
            out[...] = got
            return out
        return got

    def batch_gates_mixed(self, gates, a, b, keyswitch=True):
        return self._do("gates_mixed", {"ks": keyswitch}, [gates, a, b])

    def batch_bootstrap(self, cts, testvec=None, keyswitch=True):
        tv, kind = self._tv(testvec, testvec is not None and np.asarray(testvec).ndim == 3)
        return self._do("bootstrap", {"tv": kind, "ks": keyswitch}, [cts, tv])

    def batch_tlwe_lincomb(self, ca, a, cb=0, b=None, cconst=0):
        return self._do("tlwe_lincomb", {"ca": ca, "cb": cb, "cc": cconst}, [a, b])

    def batch_lincomb_bootstrap(self, ca, a, cb=0, b=None, cconst=0, testvec=None, keyswitch=True):
        tv, kind = self._tv(testvec, testvec is not None and np.asarray(testvec).ndim == 3)
        return self._do("lincomb_bootstrap", {"ca": ca, "cb": cb, "cc": cconst, "tv": kind, "ks": keyswitch}, [a, b, tv])

    def batch_lincomb_bootstrap_many(self, ca, a, cb=0, b=None, cconst=0, testvec=None, n_luts=2, keyswitch=True):
        tv, _ = self._tv(testvec, False)
        return self._do("lincomb_bootstrap_many", {"ca": ca, "cb": cb, "cc": cconst, "k": n_luts, "ks": keyswitch}, [a, b, tv])

    def batch_mux(self, a, b, c, naive):
        return self._do("mux", {"naive": naive}, [a, b, c])

    def batch_blind_rotate(self, cts, testvec=None):
        tv, kind = self._tv(testvec, False)
        return self._do("blind_rotate", {"tv": kind}, [cts, tv])

    def batch_identity_key_switch(self, lv1):
        return self._do("identity_key_switch", {}, [lv1])

    def batch_sample_extract(self, trlwe, k=0):
        return self._do("sample_extract", {"k": k}, [trlwe])

    def batch_external_product(self, trlwe, bsk_index):
        return self._do("external_product", {}, [trlwe, bsk_index])

    def pack(self, cts):
        return self._do("pack", {}, [cts])

    def unpack(self, trlwe, count=None, slots=None):
        count = len(slots) if slots is not None else count
        return self._do("unpack", {"slots": slots is not None}, [trlwe, slots], count=count)

    def pack_table(self, stage1, m):
        s1 = np.asarray(stage1)
        return self._do("pack_table", {"m": m}, [s1.reshape(-1, s1.shape[-1])], count=s1.shape[1])

    def batch_reencrypt(self, cts):
        return self._do("reencrypt", {}, [cts])

    def expand_seeded(self, seeded):
        return self._do("expand_seeded", {"seed": seeded.mask_seed, "first": seeded.first_index}, [seeded.bodies])

    # -- device forms
    def batch_gate_dev(self, gate, a, b, out, stream=None):
        self._do("gate", {"code": gate}, [a, b], out, form="dev0", stream=stream)

    def batch_gates_mixed_dev(self, gates, a, b, out, stream=None, keyswitch=True):
        self._do("gates_mixed", {"ks": keyswitch}, [gates, a, b], out, form="dev0", stream=stream)

    def batch_bootstrap_dev(self, cts, out, testvec=None, per_ct=False, keyswitch=True, stream=None):
        tv, kind = self._tv(testvec, per_ct)
        self._do("bootstrap", {"tv": kind, "ks": keyswitch}, [cts, tv], out, form="dev0", stream=stream)

    def batch_tlwe_lincomb_dev(self, ca, a, cb, b, cconst, out, stream=None):
        self._do("tlwe_lincomb", {"ca": ca, "cb": cb, "cc": cconst}, [a, b], out, form="dev0", stream=stream)

    def batch_lincomb_bootstrap_dev(self, ca, a, cb, b, cconst, out, testvec=None, per_ct=False, keyswitch=True, stream=None):
        tv, kind = self._tv(testvec, per_ct)
        self._do("lincomb_bootstrap", {"ca": ca, "cb": cb, "cc": cconst, "tv": kind, "ks": keyswitch}, [a, b, tv], out, form="dev0", stream=stream)

    def batch_lincomb_bootstrap_many_dev(self, ca, a, cb, b, cconst, out, testvec, n_luts=2, per_ct=False, keyswitch=True,
                                         stream=None):
        tv, _ = self._tv(testvec, False)
        self._do("lincomb_bootstrap_many", {"ca": ca, "cb": cb, "cc": cconst, "k": n_luts, "ks": keyswitch}, [a, b, tv], out,
                 form="dev0", stream=stream)

    def batch_mux_dev(self, a, b, c, out, naive, stream=None):
        self._do("mux", {"naive": naive}, [a, b, c], out, form="dev0", stream=stream)

    def batch_blind_rotate_dev(self, cts, out_trlwe, testvec=None, stream=None):
        tv, kind = self._tv(testvec, False)
        self._do("blind_rotate", {"tv": kind}, [cts, tv], out_trlwe, form="dev0", stream=stream)

    def pack_dev(self, cts, out, stream=None):
        self._do("pack", {}, [cts], out, form="dev0", stream=stream)

    def unpack_dev(self, trlwe, out, count, slots=None, stream=None):
        self._do("unpack", {"slots": slots is not None}, [trlwe, slots], out, count=count, form="dev0", stream=stream)

    def pack_table_dev(self, stage1, m, out, stream=None):
        self._do("pack_table", {"m": m}, [stage1], out, count=len(out.arr), form="dev0", stream=stream)

    def batch_reencrypt_dev(self, a, out, stream=None):
        self._do("reencrypt", {}, [a], out, form="dev0", stream=stream)

    def expand_seeded_dev(self, mask_seed, first_index, bodies, out, stream=None):
        self._do("expand_seeded", {"seed": mask_seed, "first": first_index}, [bodies], out, form="dev0", stream=stream)

    # -- encryption, decryption and the linear layers: host forms (stream=None) and device forms (out=...)
    class _Bodies:
        def __init__(self, bodies):
            self.bodies = bodies

    def _encrypt(self, op, key, plain, alpha, rng_key, mask_seed, first, full, bodies, out=None, aux=None, stream=None):
        kind = "both" if full and bodies else "full" if full else "bodies"
        n_plain = len(plain.arr if isinstance(plain, SF.FakeTensor) else plain)
        args = {"out": kind, "alpha": alpha, "rng_key": rng_key, "mask_seed": mask_seed, "first": first}
        count = n_plain
        if op == "encrypt_trlwe":
            args["words"], count = n_plain, -(-n_plain // N)
        got = self._do(op, args, [plain], out, count, "host" if out is None else "dev0", aux, self.world.secret_name(key), stream)
        if out is not None:
            return None
        if kind == "full":
            return got
        got = got.reshape(count, -1)
        width = N if op == "encrypt_trlwe" else 1
        bod = got[:, -width:].reshape(-1) if width == 1 else got[:, -width:]
        if kind == "bodies":
            return self._Bodies(bod)
        return got[:, :-width].reshape((count, 2, N) if width == N else (count, -1)), self._Bodies(bod)

    def batch_encrypt(self, key_lv0, plain, alpha=None, rng_key=None, mask_seed=None, first_index=0, full=True, bodies=False):
        return self._encrypt("encrypt", key_lv0, plain, alpha, rng_key, mask_seed, first_index, full, bodies)

    def batch_encrypt_dev(self, key_lv0, plain, alpha, mask_seed, rng_key=None, first_index=0, bodies=None, out=None, stream=None):
        first, second = (out, bodies) if out is not None else (bodies, None)
        self._encrypt("encrypt", key_lv0, plain, alpha, rng_key, mask_seed, first_index, out is not None, bodies is not None,
                      first, second, stream)

    def batch_encrypt_trlwe(self, key_lv1, plain, alpha=None, rng_key=None, mask_seed=None, first_group=0, full=True, bodies=False):
        return self._encrypt("encrypt_trlwe", key_lv1, plain, alpha, rng_key, mask_seed, first_group, full, bodies)

    def batch_encrypt_trlwe_dev(self, key_lv1, plain, alpha, mask_seed, rng_key=None, first_group=0, bodies=None, out=None,
                                stream=None):
        first, second = (out, bodies) if out is not None else (bodies, None)
        self._encrypt("encrypt_trlwe", key_lv1, plain, alpha, rng_key, mask_seed, first_group, out is not None, bodies is not None,
                      first, second, stream)

    def expand_seeded_trlwe(self, seeded):
        return self._do("expand_seeded_trlwe", {"seed": seeded.mask_seed, "first": seeded.first_group}, [seeded.bodies])

    def expand_seeded_trlwe_dev(self, mask_seed, first_group, bodies, out, stream=None):
        self._do("expand_seeded_trlwe", {"seed": mask_seed, "first": first_group}, [bodies], out, form="dev0", stream=stream)

    def batch_pk_encrypt(self, plain, alpha, rng_key=None, first_index=0):
        return self._do("pk_encrypt", {"alpha": alpha, "rng_key": rng_key, "first": first_index}, [plain])

    def batch_pk_encrypt_dev(self, plain, out, alpha, rng_key=None, first_index=0, stream=None):
        self._do("pk_encrypt", {"alpha": alpha, "rng_key": rng_key, "first": first_index}, [plain], out, form="dev0", stream=stream)

    def _mode(self, mode, modulus):
        assert (modulus == SF.MESSAGE_MODULUS) == (mode == "message")
        return mode

    def batch_decrypt(self, key, cts, mode="phase", modulus=None, out=None, stream=None):
        width = "lv0" if len(key) == self.params.n else "lv1"
        return self._do("decrypt", {"mode": self._mode(mode, modulus), "width": width}, [cts], out,
                        form="host" if out is None else "dev0", secret=self.world.secret_name(key), stream=stream)

    def batch_decrypt_dev(self, key, cts, out, mode="phase", modulus=None, stream=None):
        self.batch_decrypt(key, cts, mode, modulus, out, stream)

    def batch_decrypt_trlwe(self, key_lv1, packed, count, mode="phase", modulus=None, out=None, stream=None):
        return self._do("decrypt_trlwe", {"mode": self._mode(mode, modulus)}, [packed], out, count,
                        "host" if out is None else "dev0", secret=self.world.secret_name(key_lv1), stream=stream)

    def batch_decrypt_trlwe_dev(self, key_lv1, packed, count, out, mode="phase", modulus=None, stream=None):
        self.batch_decrypt_trlwe(key_lv1, packed, count, mode, modulus, out, stream)

    @staticmethod
    def _shape(t):
        return (t.arr if isinstance(t, SF.FakeTensor) else np.asarray(t)).shape

    def batch_tlwe_matmul(self, w, cts, bias=None, out=None, stream=None):
        (rows, cols), groups = self._shape(w), self._shape(cts)[0]
        return self._do("tlwe_matmul", {"bias": bias is not None, "shape": (rows, cols, groups)}, [w, cts, bias], out, groups * rows,
                        "host" if out is None else "dev0", stream=stream)

    def batch_tlwe_matmul_dev(self, w, cts, out, bias=None, stream=None):
        self.batch_tlwe_matmul(w, cts, bias, out, stream)

    def batch_trlwe_matmul(self, w, trlwe, bias=None, keyswitch=True, out=None, stream=None):
        (rows, cols), groups = self._shape(w), self._shape(trlwe)[0]
        return self._do("trlwe_matmul", {"ks": keyswitch, "bias": bias is not None, "shape": (rows, cols, groups)}, [w, trlwe, bias],
                        out, groups * rows, "host" if out is None else "dev0", stream=stream)

    def batch_trlwe_matmul_dev(self, w, trlwe, out, bias=None, keyswitch=True, stream=None):
        self.batch_trlwe_matmul(w, trlwe, bias, keyswitch, out, stream)

    def batch_trlwe_polymul(self, w, trlwe, bias=None, out=None, stream=None):
        (rows, cols, _), groups = self._shape(w), self._shape(trlwe)[0]
        return self._do("polymul", {"bias": bias is not None, "shape": (rows, cols, groups)}, [w, trlwe, bias], out, groups * rows,
                        "host" if out is None else "dev0", stream=stream)

    def batch_trlwe_polymul_dev(self, w, trlwe, out, bias=None, stream=None):
        self.batch_trlwe_polymul(w, trlwe, bias, out, stream)

    def batch_tlwe_conv2d(self, w, cts, bias=None, stride=1, padding=0, out=None, stream=None):
        (out_c, k, _, in_c), (groups, in_h, in_w, _, _) = self._shape(w), self._shape(cts)
        shape = (in_h, in_w, in_c, k, out_c, tuple(stride), tuple(padding), groups)
        count = groups * out_c * ((in_h + 2 * padding[0] - k) // stride[0] + 1) * ((in_w + 2 * padding[1] - k) // stride[1] + 1)
        return self._do("conv2d", {"bias": bias is not None, "shape": shape}, [w, cts, bias], out, count,
                        "host" if out is None else "dev0", stream=stream)

    def batch_tlwe_conv2d_dev(self, w, cts, out, bias=None, stride=1, padding=0, stream=None):
        self.batch_tlwe_conv2d(w, cts, bias, stride, padding, out, stream)

    # -- the TRLWE key switch, the packed CMUX and TRGSW encryption (one method for both forms, as Engine's)
    def batch_trlwe_keyswitch(self, k, trlwe, out=None, stream=None):
        dev = isinstance(trlwe, SF.FakeTensor)
        assert (out is not None) == dev and self.switch.get(k) is not None, (self.name, k)
        return self._do("trlwe_keyswitch", {"k": k}, [trlwe], out, form="dev0" if dev else "host", stream=stream, key=self.switch[k])

    def batch_trlwe_cmux(self, sel, basebit, t, d0, d1, reference_digits=False, out=None, stream=None):
        dev = isinstance(d1, SF.FakeTensor)
        assert (out is not None) == dev and isinstance(sel, SF.FakeTensor) == dev and self._shape(sel) == (2 * t, 2, N)
        return self._do("cmux", {"gadget": (basebit, t), "d0": d0 is not None, "reference": reference_digits},
                        [sel.reshape(1, 2 * t, 2, N), d0, d1], out, self._shape(d1)[0], "dev0" if dev else "host", stream=stream)

    def batch_encrypt_trgsw(self, key_lv1, mu, basebit, t, alpha=None, rng_key=None, first_index=0, out=None):
        args = {"gadget": (basebit, t), "alpha": alpha, "rng_key": rng_key, "first": first_index}
        return self._do("encrypt_trgsw", args, [mu], out, self._shape(mu)[0], "host" if out is None else "dev0",
                        secret=self.world.secret_name(key_lv1))

    def batch_encrypt_trgsw_dev(self, key_lv1, mu, basebit, t, out, alpha=None, rng_key=None, first_index=0):
        self.batch_encrypt_trgsw(key_lv1, mu, basebit, t, alpha, rng_key, first_index, out)

    def gen_trlwe_switch_key(self, key_from_lv1, key_to_lv1, k=1, basebit=4, t=6, rng_key=None, alpha=None, download=True):
        """The key of the book made under `rng_key` (what a generation under queued work must give)."""
        name = SF.switch_key_name(self.name, k, (basebit, t))
        assert rng_key == SF.switch_gen_key(name) and self.world.secret_name(key_from_lv1) == self.world.secret_name(key_to_lv1) == self.name
        self.world.switch_key_changed(self.name, k, name)
        self.switch[k] = name
        return self.world.model.keys["switch"][name]

    def load_trlwe_switch_key(self, key):
        name = SF.switch_key_name(self.name, key.k, (key.basebit, key.t))
        assert self.world.model.keys["switch"][name] is key
        self.world.switch_key_changed(self.name, key.k, name)
        self.switch[key.k] = name

    def drop_trlwe_switch_key(self, k):
        assert self.switch.get(k) is not None
        self.world.switch_key_changed(self.name, k, None)
        self.switch[k] = None

    def trlwe_switch_key_is_loaded(self, k):
        return self.switch.get(k) is not None

    def _times(self, op, names):
        passes, self.world.passes[op] = self.world.passes[op], 0
        return dict({n: 0.25 * passes for n in names}, passes=passes)

    def trlwe_switch_times(self):
        return self._times("trlwe_keyswitch", ("digits_ms", "contraction_ms"))

    def cmux_times(self):
        return self._times("cmux", ("digits_ms", "contraction_ms", "addend_ms"))

    # -- state
    def load_cloud_key(self, tag):
        self.key = tag.name

    load_compressed_cloud_key = load_cloud_key

    def gen_cloud_key(self, tag, key_lv1, seed=None):
        self.key = tag.name

    def load_packing_key(self, pk):
        self.calls.append("load_packing_key")

    def set_profiling(self, on):
        self.calls.append("set_profiling")
        self.world.profiling = bool(on)

    def kernel_times(self):
        return {}

    def set_combining(self, n):
        self.calls.append("set_combining")

    def synchronize(self):
        self.world.synchronized()


@pytest.fixture(scope="module")
def host_keys(O):
    """The keys of the small shape: five cloud keys (K1 of the engine; two of each of K2 and K3, one per way a key
    change can bring them), a packing key per handle, a re-encryption key, the secret keys the pools encrypt under (and
    the encrypting and decrypting steps name), and a public key of SF.PK_SIZE rows per handle."""
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import SecurityParams

    op = O.Params(HOST.name, HOST.n, 2, 8, 2, 5, 2.0e-5, 2.0e-8)
    pp = SecurityParams(op.name, 0, op.n, op.l, op.bgbit, op.basebit, op.t, op.alpha_lv0, op.alpha_lv1)
    sk = {k: O.SecretKey(op, 70 + j) for j, k in enumerate(("K1", "K2", "K3"))}
    cloud = {"K1": O.CloudKey(sk["K1"], 71)}
    for j, name in enumerate(("K2/gen", "K2/comp", "K3/gen", "K3/comp")):
        cloud[name] = O.CloudKey(sk[name[:2]], 80 + j)
    packing = {}
    for h, k in (("E", "K1"), ("V2", "K2")):
        pk = SecretKey(pp, sk[k].key_lv0, sk[k].key_lv1).packing_key(rng_key=90 + len(packing))
        packing[h] = (pk, PK.key_rows(pp, pk.mask_seed, pk.bodies))
    import sym_encrypt_model as SM

    client = {h: SecretKey(pp, sk[k].key_lv0, sk[k].key_lv1) for h, k in (("E", "K1"), ("V2", "K2"))}
    public = {h: SM.public_key(c.key_lv0, SF.PK_SIZE, pp.alpha_lv0, SF.PK_GEN_KEY)[0] for h, c in client.items()}
    import trlwe_switch_model as TM

    # the switching keys (s_from = s_to = the handle's ring key): what each view starts with and what a change brings
    switch = {}
    for name in SF.switch_book_names():
        h, k = name.split(":")[:2]
        switch[name] = TM.make_key(client[h].key_lv1, client[h].key_lv1, int(k), *SF.switch_key_gadget(name), SF.switch_gen_key(name),
                                   pp.alpha_lv1)
    keys = {"params": pp, "oracle_params": op, "cloud": cloud, "packing": packing, "secrets": client, "public": public,
            "reenc": O.gen_reenc_key(op, sk["K1"].key_lv0, 95, key_to=sk["K3"].key_lv0), "switch": switch}
    secrets = {"E": sk["K1"], "V2": sk["K2"], "VR": sk["K1"]}
    return keys, secrets


def _model(O, keys, pools):
    """A model of the sequence whose pools these are (it evaluates the rows of the "ring" pool together), sharing the
    ring rows of this module."""
    model = SF.Model(O, keys, _RING_MEMO)
    model.ring_pool = pools["ring"]
    return model


def _stand_ins(model, keys, racy):
    world = _World(model, keys["params"].n, racy, keys["secrets"])
    book = {name: {"full": _Tag(name), "comp": _Tag(name), "gen": (_Tag(name), None, 0)} for name in keys["cloud"]}
    start = SF.switch_keys_after([], -1)
    handles = {"E": StandIn(world, "E", keys["params"], "K1", start["E"]), "V2": StandIn(world, "V2", keys["params"], "K2/gen", start["V2"]),
               "VR": StandIn(world, "VR", keys["params"], "reenc"), "book": book, "switch_book": keys["switch"],
               "packing": {h: pk for h, (pk, _) in keys["packing"].items()}, "combining_default": 256,
               "secrets": keys["secrets"]}
    return world, handles


@pytest.mark.parametrize("seed", HOST_SEEDS)
def test_harness_and_model_agree_on_a_faithful_stand_in(O, host_keys, seed):
    keys, secrets = host_keys
    seq = SF.random_sequence(seed, HOST)
    pools = SF.make_pools(HOST, seed, secrets)
    world, handles = _stand_ins(_model(O, keys, pools), keys, racy=False)
    be = SF.FakeBackend(world.read_back, world.synchronized)
    got, info = SF.run(seq, handles, be.streams(), pools, be)
    model = _model(O, keys, pools)
    want = SF.expected(seq, O, keys, pools, model)
    assert sorted(got) == [st.i for st in seq if st.kind == "call"]
    assert SF.compare(got, want) == [], SF.describe(seq, SF.compare(got, want), got, want)
    assert handles["V2"].key == SF.final_keys(seq)
    assert len(info["kernel_times"]) == 2
    # the ring families: the passes each ring_times step reports, the keys each view holds after the last step, the
    # chains that end in plaintext within their 8 sigma (the reference alone, on the CPU)
    passes = SF.check_ring_times(seq, info)
    assert len(passes) == 2 and sum(map(sum, passes.values())) > 0
    assert {h: handles[h].switch for h in ("E", "V2")} == SF.switch_keys_after(seq) and handles["VR"].switch == {}
    SF.final_switch_check(seq, handles, pools, model)
    assert SF.chains_decrypt_to_their_plaintext_products(HOST, keys["secrets"], seq, got, pools) == 4
    # a ring step costs the model at most ROWS_PER_STEP rows, whatever its count (2,049 among them)
    ring = [st for st in seq if st.ring]
    assert len(world.model.ring_log) >= len(ring) and max(st.count for st in ring) == SF.RING_BIG
    assert all(rows <= SF.ROWS_PER_STEP for _, _, rows in world.model.ring_log + model.ring_log)
    cost = sum(min(s.count, SF.ROWS_PER_STEP) * s.oracle_bootstraps for s in seq)
    assert 0 < cost <= SF.MAX_ORACLE_BOOTSTRAPS
    # the blind rotations the oracle ran: a handful per step, whatever the steps' counts
    assert 0 < model.bootstraps <= cost < sum(st.count for st in seq)
    # made alone (host forms, a synchronisation after each): the same words
    world2, handles2 = _stand_ins(model, keys, racy=False)
    alone, _ = SF.run(SF.as_host(seq), handles2, be.streams(), pools, SF.FakeBackend())
    assert SF.compare(alone, want) == []


@pytest.mark.parametrize("seed", HOST_SEEDS)
def test_comparison_fails_at_exactly_the_clobbered_steps(O, host_keys, seed):
    """A device whose key switches share one output scratch: each _dev step reads back the most recent key switch of at
    least its size.  The comparison reports those steps and no other."""
    keys, secrets = host_keys
    seq = SF.random_sequence(seed, HOST)
    pools = SF.make_pools(HOST, seed, secrets)
    model = _model(O, keys, pools)
    world, handles = _stand_ins(model, keys, racy="key_switch")
    be = SF.FakeBackend(world.read_back, world.synchronized)
    got, _ = SF.run(seq, handles, be.streams(), pools, be)
    want = SF.expected(seq, O, keys, pools, model)
    n = keys["params"].n
    clobbered = []
    for st in seq:
        if not st.dev or not st.ks_rows:
            continue
        donor = [d for d in seq if d.kind == "call" and d.ks_rows >= st.ks_rows][-1]
        if donor.i != st.i and not np.array_equal(want[donor.i].reshape(-1, n + 1)[:st.ks_rows], want[st.i].reshape(-1, n + 1)):
            clobbered.append(st.i)
    assert len(clobbered) >= 5
    assert SF.compare(got, want) == clobbered


@pytest.mark.parametrize("seed", HOST_SEEDS)
def test_comparison_fails_at_exactly_the_steps_of_an_unclaimed_secret(O, host_keys, seed):
    """A device whose one buffer of staged secrets is shared without a claim: a secret-staging _dev step that another
    secret-staging call follows before the next synchronisation runs under the later call's key.  The comparison
    reports those steps and what is chained from them, and no other.  The steps are read off the sequence
    (SF.unclaimed_secret_steps), their words off the model under the other handle's key; a step whose words the other
    key does not change (a one-row boolean, say) is no failure."""
    keys, secrets = host_keys
    seq = SF.random_sequence(seed, HOST)
    pools = SF.make_pools(HOST, seed, secrets)
    model = _model(O, keys, pools)
    world, handles = _stand_ins(model, keys, racy="secret")
    be = SF.FakeBackend(world.read_back, world.synchronized)
    got, _ = SF.run(seq, handles, be.streams(), pools, be)
    want = SF.expected(seq, O, keys, pools, model)
    wrong_key = SF.unclaimed_secret_steps(seq)
    for i, h in wrong_key.items():
        assert seq[i].dev and seq[i].op in SF.SECRET_OPS and h != seq[i].handle and h in ("E", "V2")
        later = [st for st in seq[i + 1:] if st.kind == "call" and st.op in SF.SECRET_OPS and st.handle == h]
        assert later and not any(st.kind == "state" and st.op == "synchronize" for st in seq[i + 1:later[0].i])
    assert len(wrong_key) >= 3  # (every sequence carries two pairs made for this, and chains C and D)
    raced = SF.expected(seq, O, keys, pools, model, secret_of=wrong_key)
    predicted = [i for i in sorted(want) if not np.array_equal(want[i], raced[i])]
    cones = set().union(*(SF.cone(seq, i) for i in wrong_key))
    assert set(predicted) <= cones
    # a phase or a ciphertext never survives another key (but a chain whose head was encrypted under the other key too
    # decrypts to the right phases again under it)
    sure = [i for i in wrong_key if seq[i].args.get("mode", "phase") == "phase" and not seq[i].sources]
    assert len(sure) >= 2 and set(sure) <= set(predicted)
    assert SF.compare(got, want) == predicted, SF.describe(seq, SF.compare(got, want), got, want)
    # the same device with every call made alone (a synchronisation after each) is right
    world2, handles2 = _stand_ins(model, keys, racy="secret")
    be2 = SF.FakeBackend(world2.read_back, world2.synchronized)
    alone, _ = SF.run(SF.as_host(seq), handles2, be2.streams(), pools, be2)
    assert SF.compare(alone, want) == []


@pytest.mark.parametrize("seed", HOST_SEEDS)
def test_comparison_fails_at_exactly_the_ring_clobbered_steps(O, host_keys, seed):
    """A device whose ring families (the TRLWE key switch, the packed CMUX) each share their digit scratch without a
    claim: a ring _dev step still pending -- its stream not synchronised, no later call on it -- when a call of its family
    of at least its size is made gives the first rows of that call's result.  The steps are read off the sequence
    (SF.ring_clobbered_steps), their words off the model; the comparison reports them and what is chained from them, and
    no other (a step whose donor holds the same rows is no failure)."""
    keys, secrets = host_keys
    seq = SF.random_sequence(seed, HOST)
    pools = SF.make_pools(HOST, seed, secrets)
    model = _model(O, keys, pools)
    world, handles = _stand_ins(model, keys, racy="ring_scratch")
    be = SF.FakeBackend(world.read_back, world.synchronized)
    got, _ = SF.run(seq, handles, be.streams(), pools, be)
    want = SF.expected(seq, O, keys, pools, model)
    donors = SF.ring_clobbered_steps(seq)
    for i, j in donors.items():
        assert seq[i].ring and seq[i].dev and seq[j].op == seq[i].op and j > i and seq[j].count >= seq[i].count
        assert not any(st.kind == "state" and st.op == "synchronize" or st.queued and st.stream == seq[i].stream for st in seq[i + 1:j])
    raced = SF.expected(seq, O, keys, pools, model, donor_of=dict(donors, words=want))
    predicted = [i for i in sorted(want) if not np.array_equal(want[i], raced[i])]
    assert set(predicted) <= set().union(*(SF.cone(seq, i) for i in donors))
    assert len([i for i in predicted if i in donors]) >= 3  # (the ring items put a family's calls on other streams back to back)
    assert SF.compare(got, want) == predicted, SF.describe(seq, SF.compare(got, want), got, want)
    # the same device with every call made alone (a synchronisation after each) is right
    world2, handles2 = _stand_ins(model, keys, racy="ring_scratch")
    be2 = SF.FakeBackend(world2.read_back, world2.synchronized)
    alone, _ = SF.run(SF.as_host(seq), handles2, be2.streams(), pools, be2)
    assert SF.compare(alone, want) == []


@pytest.mark.parametrize("seed", HOST_SEEDS)
def test_comparison_fails_at_exactly_the_steps_of_an_undrained_switching_key(O, host_keys, seed):
    """A device whose switch_key_change replaces a key's rows without draining: a trlwe_keyswitch_dev of that k on that
    view that nothing has synchronised runs under the new key (another gadget: other digits against other rows).  The
    steps are read off the sequence (SF.undrained_switch_steps); the comparison reports them and what is chained from
    them, and no other."""
    keys, secrets = host_keys
    seq = SF.random_sequence(seed, HOST)
    pools = SF.make_pools(HOST, seed, secrets)
    model = _model(O, keys, pools)
    world, handles = _stand_ins(model, keys, racy="switch_table")
    be = SF.FakeBackend(world.read_back, world.synchronized)
    got, _ = SF.run(seq, handles, be.streams(), pools, be)
    want = SF.expected(seq, O, keys, pools, model)
    wrong_key = SF.undrained_switch_steps(seq)
    assert len(wrong_key) >= 2  # (each switch_key_change of the generator follows a queued switch of its view and k)
    for i, name in wrong_key.items():
        assert seq[i].dev and seq[i].op == "trlwe_keyswitch" and name.startswith(f"{seq[i].handle}:{seq[i].args['k']}:")
    raced = SF.expected(seq, O, keys, pools, model, switch_of=wrong_key)
    predicted = [i for i in sorted(want) if not np.array_equal(want[i], raced[i])]
    assert set(wrong_key) <= set(predicted) <= set().union(*(SF.cone(seq, i) for i in wrong_key))
    assert SF.compare(got, want) == predicted, SF.describe(seq, SF.compare(got, want), got, want)
    assert {h: handles[h].switch for h in ("E", "V2")} == SF.switch_keys_after(seq)
    # the same device with every call made alone is right
    world2, handles2 = _stand_ins(model, keys, racy="switch_table")
    be2 = SF.FakeBackend(world2.read_back, world2.synchronized)
    alone, _ = SF.run(SF.as_host(seq), handles2, be2.streams(), pools, be2)
    assert SF.compare(alone, want) == []


_CORPUS_SECRETS = {}


def _corpus_secrets(name):
    """The secret keys of the GPU test's world of shape `name` (E under K1, V2 under K2)."""
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import PARAM_SETS

    if name not in _CORPUS_SECRETS:
        sk = [SecretKey.new(PARAM_SETS[name], 7100 + j) for j in range(2)]
        _CORPUS_SECRETS[name] = {"E": sk[0], "V2": sk[1], "VR": sk[0]}
    return PARAM_SETS[name], _CORPUS_SECRETS[name]


@pytest.mark.parametrize("seed", SF.SEEDS["SECURITY_128_BIT"])
@pytest.mark.parametrize("name", sorted(SF.SHAPES))
def test_ring_chains_reach_their_bound_on_the_model(name, seed):
    """Chains E and F of every sequence the GPU test runs -- both shapes of the corpus, each with its own alpha_lv1 (on
    these sets 2.0e-8 and 2.2e-16: under a (1, 32) key the latter bound is below one LSB and asks for equality; under a
    gadget of t basebit < 32 it is rounding variance alone) -- evaluated by the numpy models alone (a Model that answers
    ring ops and needs no oracle) under keys made on the CPU, decrypt to psi_k of their plaintexts within the 8 sigma the
    GPU test applies."""
    import trlwe_switch_model as TM

    shape = SF.SHAPES[name]
    p, secrets = _corpus_secrets(name)
    assert seed in SF.SEEDS[name] and p.alpha_lv1 == shape.alpha_lv1
    seq = SF.random_sequence(seed, shape)
    pools = SF.make_pools(shape, seed, secrets)
    only = {st.i for st in seq if st.kind == "call" and st.args.get("chain") in ("E", "F")}
    assert len(only) == 7
    switch = {}  # the keys in force at the chains' switches
    for st in seq:
        if st.i in only and st.op == "trlwe_keyswitch":
            key = SF.switch_keys_after(seq, st.i)[st.handle][st.args["k"]]
            ring = secrets[st.handle].key_lv1
            switch[key] = TM.make_key(ring, ring, st.args["k"], *SF.switch_key_gadget(key), SF.switch_gen_key(key), p.alpha_lv1)
    ring_keys = {"params": p, "switch": switch, "secrets": secrets}
    want = SF.expected(seq, None, ring_keys, pools, SF.Model(None, ring_keys), only=only)
    assert SF.chains_decrypt_to_their_plaintext_products(shape, secrets, seq, want, pools, ("E", "F")) == 2


@pytest.mark.parametrize("op", SF.RING_OPS)
def test_a_ring_step_of_2049_rows_costs_the_model_three(host_keys, op):
    """The RING_BIG step of each family on a model that has seen nothing: ROWS_PER_STEP rows reach the numpy model (the
    rows _rowwise hands to it, counted there), whatever the step's count."""
    keys, secrets = host_keys
    seq = SF.random_sequence(0, HOST)
    pools = SF.make_pools(HOST, 0, secrets)
    st = next(st for st in seq if st.op == op and st.count == SF.RING_BIG)
    assert not st.sources
    ring_keys = {"params": keys["params"], "switch": keys["switch"], "secrets": keys["secrets"]}
    model = SF.Model(None, ring_keys)
    want = SF.expected(seq, None, ring_keys, pools, model, only={st.i})
    assert want[st.i].shape == (SF.RING_BIG, 2, N) and len(np.unique(want[st.i].reshape(SF.RING_BIG, -1), axis=0)) == SF.ROWS_PER_STEP
    assert model.ring_log == [(op, SF.RING_BIG, SF.ROWS_PER_STEP)] and model.rows_evaluated == SF.ROWS_PER_STEP
    # again: nothing more; and a model without the memo's help gives the same words for the last row alone
    SF.expected(seq, None, ring_keys, pools, model, only={st.i})
    assert model.ring_log[1:] == [(op, SF.RING_BIG, 0)]
    x = SF.materialise(st, pools, {})
    plain = SF.Model(None, ring_keys)
    key = SF.switch_keys_after(seq, st.i)[st.handle][st.args["k"]] if op == "trlwe_keyswitch" else None
    for j in (SF.RING_BIG - 1,):  # (a CMUX step's first operand is its one selector)
        xj = [v if v is None or (op == "cmux" and k == 0) else v[j:j + 1] for k, v in enumerate(x)]
        assert np.array_equal(plain.eval(key, st.handle, op, st.args, 1, xj)[0], want[st.i][j]), j
    assert plain.rows_evaluated == 1


def test_comparison_sees_one_wrong_step_on_the_stand_in(O, host_keys):
    """One operand of the head of a chain (A: gate -> pack -> unpack; C: encrypt -> tlwe_matmul -> decrypt) perturbed
    in the model only: that step and the steps chained from it."""
    keys, secrets = host_keys
    seq = SF.random_sequence(0, HOST)
    pools = SF.make_pools(HOST, 0, secrets)
    model = _model(O, keys, pools)
    world, handles = _stand_ins(model, keys, racy=False)
    be = SF.FakeBackend()
    got, _ = SF.run(seq, handles, be.streams(), pools, be)
    for head_op in ("gate", "encrypt"):
        head = next(st.i for st in seq if st.kind == "call" and st.op == head_op and len(SF.cone(seq, st.i)) == 3)
        wrong = SF.expected(seq, O, keys, pools, model, perturb=head)
        assert SF.compare(got, wrong) == sorted(SF.cone(seq, head)), head_op
    # and of chains E (encrypt_trlwe -> trlwe_keyswitch -> decrypt_trlwe) and F (encrypt_trgsw -> cmux -> trlwe_keyswitch
    # -> decrypt_trlwe: the selector's message moved)
    for which, links in (("E", 3), ("F", 4)):
        head = next(st.i for st in seq if st.kind == "call" and st.args.get("chain") == which)
        assert len(SF.cone(seq, head)) == links
        wrong = SF.expected(seq, O, keys, pools, model, perturb=head)
        assert SF.compare(got, wrong) == sorted(SF.cone(seq, head)), which
