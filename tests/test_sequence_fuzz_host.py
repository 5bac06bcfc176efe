"""The sequence fuzz without a device (tests/sequence_fuzz.py): the generator is deterministic, the corpus the GPU tests
run holds every condition they rely on, the executor and the model agree on a faithful stand-in handle (every call
evaluated at call time by the same SF.Model.eval that expected() uses, so this holds the executor's plumbing -- routing,
chaining, tiling, key tracking, buffer use -- and NOT the model's own formulas, which only the GPU run at
SECURITY_128_BIT holds to the device), and the comparison fails -- at exactly the clobbered steps -- on a stand-in
that shares one key-switch scratch among its calls."""
import numpy as np
import pytest

import sequence_fuzz as SF

N = 1024
# a small shape in the exact-product regime (log2(2l) + 10 + (bgbit - 1) + 31 < 51): oracle bootstraps of a millisecond
HOST = SF.Shape("SFUZZ_HOST", 16, SF.BASE_COUNTS, True, False)
HOST_SEEDS = (0, 1, 2)


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
            "V2 after E", "E after V2", "chained pack", "chained unpack", "chained bootstrap"]
    need += ["dev then " + op for op in SF.STATE_OPS] + ["state " + op for op in SF.STATE_OPS]
    need += ["op " + SF.variant_name(op, args) for op, args in SF.variants(shape)]
    need += ["form " + f for f in SF.FORMS] + ["route " + r for r in SF.ROUTES]
    short = {k: c.get(k, 0) for k in need if c.get(k, 0) < 3}
    assert not short, short
    for seq in seqs:
        for st in seq:
            if st.kind != "call":
                continue
            assert st.form in SF.forms_of(st.op) and st.count >= 1
            assert st.count in shape.counts or st.args.get("grow")
            for j in st.sources:  # a chained operand: an earlier _dev step on the same stream and handle
                assert j < st.i and seq[j].dev and st.dev and seq[j].stream == st.stream and seq[j].handle == st.handle
            assert (st.op == "reencrypt") == (st.handle == "VR")
        # a key change on V2 drains V2's own streams and nothing else
        pending = set()
        for st in seq:
            if st.handle == "V2" and st.dev:
                pending.add(st.stream)
            if st.kind == "state" and st.op == "key_change":
                assert st.handle == "V2" and set(st.args["wait"]) == pending
                pending = set()
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

    def __init__(self, model, n, racy):
        self.model, self.n, self.racy = model, n, racy
        self.order = 0
        self.key_switches = []  # (order, rows, words [rows][n+1])
        self.dev_outs = []  # (order, rows, FakeTensor)

    def read_back(self):
        """The racy device: every _dev result that went through the key switch's scratch reads as the most recent key
        switch of at least its size."""
        if not self.racy:
            return
        for order, rows, t in self.dev_outs:
            donor = [k for k in self.key_switches if k[1] >= rows][-1]
            if donor[0] != order:
                t.arr[...] = donor[2][:rows].reshape(t.arr.shape)


class StandIn:
    """An Engine-shaped handle that evaluates each call with SF.Model.eval at call time, under the key it holds then
    (the model expected() uses: an error inside the model is invisible here)."""

    def __init__(self, world, name, params, key):
        self.world, self.name, self.params, self.key = world, name, params, key
        self.calls = []

    def _do(self, op, args, operands, out=None, count=None, form="host"):
        w = self.world
        x = [o.arr if isinstance(o, SF.FakeTensor) else o for o in operands]
        count = len(x[0]) if count is None else count
        got = np.ascontiguousarray(w.model.eval(self.key, self.name, op, args, count, x), dtype=np.uint32)
        w.order += 1
        rows = SF.Step("call", self.name, op, form, count, args=args).ks_rows
        if rows:
            w.key_switches.append((w.order, rows, got.reshape(-1, w.n + 1).copy()))
        self.calls.append(op)
        if out is None:
            return got
        assert isinstance(out, SF.FakeTensor) and (out.arr == SF.FILL).all(), "an output buffer was used twice"
        out.arr[...] = got.reshape(out.arr.shape)
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
        self._do("gate", {"code": gate}, [a, b], out, form="dev0")

    def batch_gates_mixed_dev(self, gates, a, b, out, stream=None, keyswitch=True):
        self._do("gates_mixed", {"ks": keyswitch}, [gates, a, b], out, form="dev0")

    def batch_bootstrap_dev(self, cts, out, testvec=None, per_ct=False, keyswitch=True, stream=None):
        tv, kind = self._tv(testvec, per_ct)
        self._do("bootstrap", {"tv": kind, "ks": keyswitch}, [cts, tv], out, form="dev0")

    def batch_tlwe_lincomb_dev(self, ca, a, cb, b, cconst, out, stream=None):
        self._do("tlwe_lincomb", {"ca": ca, "cb": cb, "cc": cconst}, [a, b], out, form="dev0")

    def batch_lincomb_bootstrap_dev(self, ca, a, cb, b, cconst, out, testvec=None, per_ct=False, keyswitch=True, stream=None):
        tv, kind = self._tv(testvec, per_ct)
        self._do("lincomb_bootstrap", {"ca": ca, "cb": cb, "cc": cconst, "tv": kind, "ks": keyswitch}, [a, b, tv], out, form="dev0")

    def batch_lincomb_bootstrap_many_dev(self, ca, a, cb, b, cconst, out, testvec, n_luts=2, per_ct=False, keyswitch=True,
                                         stream=None):
        tv, _ = self._tv(testvec, False)
        self._do("lincomb_bootstrap_many", {"ca": ca, "cb": cb, "cc": cconst, "k": n_luts, "ks": keyswitch}, [a, b, tv], out,
                 form="dev0")

    def batch_mux_dev(self, a, b, c, out, naive, stream=None):
        self._do("mux", {"naive": naive}, [a, b, c], out, form="dev0")

    def batch_blind_rotate_dev(self, cts, out_trlwe, testvec=None, stream=None):
        tv, kind = self._tv(testvec, False)
        self._do("blind_rotate", {"tv": kind}, [cts, tv], out_trlwe, form="dev0")

    def pack_dev(self, cts, out, stream=None):
        self._do("pack", {}, [cts], out, form="dev0")

    def unpack_dev(self, trlwe, out, count, slots=None, stream=None):
        self._do("unpack", {"slots": slots is not None}, [trlwe, slots], out, count=count, form="dev0")

    def pack_table_dev(self, stage1, m, out, stream=None):
        self._do("pack_table", {"m": m}, [stage1], out, count=len(out.arr), form="dev0")

    def batch_reencrypt_dev(self, a, out, stream=None):
        self._do("reencrypt", {}, [a], out, form="dev0")

    def expand_seeded_dev(self, mask_seed, first_index, bodies, out, stream=None):
        self._do("expand_seeded", {"seed": mask_seed, "first": first_index}, [bodies], out, form="dev0")

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

    def kernel_times(self):
        return {}

    def set_combining(self, n):
        self.calls.append("set_combining")

    def synchronize(self):
        pass


@pytest.fixture(scope="module")
def host_keys(O):
    """The keys of the small shape: five cloud keys (K1 of the engine; two of each of K2 and K3, one per way a key
    change can bring them), a packing key per handle, a re-encryption key, and the secret keys the pools encrypt under."""
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
    keys = {"params": pp, "oracle_params": op, "cloud": cloud, "packing": packing,
            "reenc": O.gen_reenc_key(op, sk["K1"].key_lv0, 95, key_to=sk["K3"].key_lv0)}
    secrets = {"E": sk["K1"], "V2": sk["K2"], "VR": sk["K1"]}
    return keys, secrets


def _stand_ins(model, keys, racy):
    world = _World(model, keys["params"].n, racy)
    book = {name: {"full": _Tag(name), "comp": _Tag(name), "gen": (_Tag(name), None, 0)} for name in keys["cloud"]}
    handles = {"E": StandIn(world, "E", keys["params"], "K1"), "V2": StandIn(world, "V2", keys["params"], "K2/gen"),
               "VR": StandIn(world, "VR", keys["params"], "reenc"), "book": book,
               "packing": {h: pk for h, (pk, _) in keys["packing"].items()}, "combining_default": 256}
    return world, handles


@pytest.mark.parametrize("seed", HOST_SEEDS)
def test_harness_and_model_agree_on_a_faithful_stand_in(O, host_keys, seed):
    keys, secrets = host_keys
    seq = SF.random_sequence(seed, HOST)
    pools = SF.make_pools(HOST, seed, secrets)
    world, handles = _stand_ins(SF.Model(O, keys), keys, racy=False)
    be = SF.FakeBackend(world.read_back)
    got, info = SF.run(seq, handles, be.streams(), pools, be)
    model = SF.Model(O, keys)
    want = SF.expected(seq, O, keys, pools, model)
    assert sorted(got) == [st.i for st in seq if st.kind == "call"]
    assert SF.compare(got, want) == [], SF.describe(seq, SF.compare(got, want), got, want)
    assert handles["V2"].key == SF.final_keys(seq)
    assert len(info["kernel_times"]) == 2
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
    model = SF.Model(O, keys)
    world, handles = _stand_ins(model, keys, racy=True)
    be = SF.FakeBackend(world.read_back)
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


def test_comparison_sees_one_wrong_step_on_the_stand_in(O, host_keys):
    """One operand of the head of a chain perturbed in the model only: that step and the steps chained from it."""
    keys, secrets = host_keys
    seq = SF.random_sequence(0, HOST)
    pools = SF.make_pools(HOST, 0, secrets)
    model = SF.Model(O, keys)
    world, handles = _stand_ins(model, keys, racy=False)
    be = SF.FakeBackend()
    got, _ = SF.run(seq, handles, be.streams(), pools, be)
    head = next(st.i for st in seq if st.kind == "call" and st.op == "gate" and len(SF.cone(seq, st.i)) == 3)
    wrong = SF.expected(seq, O, keys, pools, model, perturb=head)
    assert SF.compare(got, wrong) == sorted(SF.cone(seq, head))
