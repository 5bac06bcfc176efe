"""Sequence fuzz on the GPU (tests/sequence_fuzz.py): any order of calls, forms and streams on one context and its key
views, with no synchronisation between the steps.

SECURITY_128_BIT (the exact-product regime): every word of every row of every step against the model (the CPU oracle
under the key the handle holds at that step; packing.pack_model / key_switch_model / table_model for the key-switch
forms the reference lacks), the loaded flags after the last step, and tfhe_hip_get_kernel_times after every profiling
toggle.  SECURITY_UINT4 (l = 1, general rounding, the column-sliced key switch, inexact products): the property is
order-independence, so the reference is THE SAME CALL MADE ALONE -- every step by its host form on a second context
with the same keys, a synchronisation after each -- word for word (kernels agree bit for bit across forms and counts:
test_dispatch_crossovers_bit_exact; isolated calls are held to the oracle by the other suites); and every gate-type
output on genuine encryptions decrypts to its truth table.  A directed test holds the one pair found by reading: a
host key switch issued while an un-synchronised unpack_dev still walks the shared digit scratch.

The six sequences of a shape run on one context, seed after seed, and scratch never shrinks: the grow step of seed s
is 1.5 x that of seed s - 1 (more than ensure()'s quarter of headroom), so each of them reallocates under in-flight
work, not only the first.

Every key of a shape is made on the GPU once (tfhe_hip_gen_cloud_key with a seed, tfhe_hip_gen_compressed_cloud_key
with a generator key) and exported, so that each route of a key change (load, compressed load, seeded generation) has
a key whose words the model knows."""
import time

import numpy as np
import pytest

import sequence_fuzz as SF

pytestmark = pytest.mark.gpu

N = 1024
_WORLDS = {}


class _World:
    pass


def _world(O, name):
    """One shape: the context (engine E, key views V2 and VR), a second context with the same keys (the calls made
    alone), the key book, the oracle's form of every key (exact shapes), three streams."""
    if name in _WORLDS:
        return _WORLDS[name]
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import PARAM_SETS

    w = _World()
    w.shape, w.p, w.op = SF.SHAPES[name], PARAM_SETS[name], O.PARAM_SETS[name]
    p = w.p
    w.sk = {k: SecretKey.new(p, 7100 + j) for j, k in enumerate(("K1", "K2", "K3"))}
    w.eng = R.Engine(p, 0)
    w.eng.gen_cloud_key(w.sk["K1"].key_lv0, w.sk["K1"].key_lv1, seed=7201)
    exported = {"K1": w.eng.export_cloud_key()} if w.shape.exact else {}
    w.book = {}
    tmp = w.eng.new_key_view()
    try:
        for j, t in enumerate(("K2", "K3")):
            k0, k1 = w.sk[t].key_lv0, w.sk[t].key_lv1
            tmp.gen_cloud_key(k0, k1, seed=7210 + j)
            w.book[t + "/gen"] = {"gen": (k0, k1, 7210 + j), "full": tmp.export_cloud_key()}
            w.book[t + "/comp"] = {"comp": tmp.gen_compressed_cloud_key(k0, k1, rng_key=bytes(range(j, j + 32)))}
            if w.shape.exact:
                exported[t + "/gen"] = w.book[t + "/gen"]["full"]
                exported[t + "/comp"] = tmp.export_cloud_key()
    finally:
        tmp.close()
    w.packing = {"E": w.sk["K1"].packing_key(rng_key=7301), "V2": w.sk["K2"].packing_key(rng_key=7302)}
    w.reenc = O.gen_reenc_key(w.op, w.sk["K1"].key_lv0, 7401, key_to=w.sk["K3"].key_lv0)
    w.default_combining = w.eng.combine_stats()["max_count"]

    def handles(eng):
        v2, vr = eng.new_key_view(), eng.new_key_view()
        v2.load_cloud_key(w.book["K2/gen"]["full"])
        vr.load_reenc_key(w.reenc)
        eng.load_packing_key(w.packing["E"])
        v2.load_packing_key(w.packing["V2"])
        return {"E": eng, "V2": v2, "VR": vr, "book": w.book, "packing": w.packing, "combining_default": w.default_combining}

    w.handles = handles(w.eng)
    w.alone = None
    if not w.shape.exact:
        w.eng2 = R.Engine(p, 0)
        w.eng2.gen_cloud_key(w.sk["K1"].key_lv0, w.sk["K1"].key_lv1, seed=7201)  # the seeded generator: the same key
        w.alone = handles(w.eng2)
    w.be = SF.TorchBackend()
    w.streams = w.be.streams()
    w.secrets = {"E": w.sk["K1"], "V2": w.sk["K2"], "VR": w.sk["K1"]}
    w.keys = w.model = None
    if w.shape.exact:
        cloud = {k: O.CloudKey.from_arrays(w.op, c.bootstrapping_key, c.key_switching_key, c.decomposition_offset,
                                           c.blind_rotate_testvec) for k, c in exported.items()}
        w.keys = {"params": p, "oracle_params": w.op, "cloud": cloud, "reenc": w.reenc,
                  "packing": {h: (pk, PK.key_rows(p, pk.mask_seed, pk.bodies)) for h, pk in w.packing.items()}}
        w.model = SF.Model(O, w.keys)
    w.report, w.got, w.pools = {}, {}, {}
    _WORLDS[name] = w
    return w


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    for w in _WORLDS.values():
        for eng in (w.eng, getattr(w, "eng2", None)):
            if eng is not None:
                eng.close()  # its key views go first
    _WORLDS.clear()


def _reset(w, handles):
    """Where every sequence starts: V2 under K2 (as generated), profiling off, the default combining, nothing queued."""
    handles["V2"].load_cloud_key(w.book["K2/gen"]["full"])
    handles["E"].set_profiling(False)
    handles["E"].kernel_times()
    handles["E"].set_combining(w.default_combining)
    handles["E"].synchronize()
    w.be.synchronize()


def _run(w, seed):
    seq = SF.random_sequence(seed, w.shape)
    pools = w.pools[seed] = SF.make_pools(w.shape, seed, w.secrets)
    _reset(w, w.handles)
    got, info = SF.run(seq, w.handles, w.streams, pools, w.be)
    for i, kt in info["kernel_times"]:  # tfhe_hip_get_kernel_times answered after each profiling toggle
        assert kt["blind_rotate_launches"] >= 0 and kt["key_switch_ms"] >= 0.0, (i, kt)
    assert len(info["kernel_times"]) == 2
    for h in SF.HANDLES:
        assert SF.flags(w.handles[h]) == SF.EXPECTED_FLAGS[h], (h, SF.flags(w.handles[h]))
    w.got[seed] = got
    return seq, pools, got, info


@pytest.mark.parametrize("seed", SF.SEEDS["SECURITY_128_BIT"])
def test_sequences_128bit(O, seed):
    w = _world(O, "SECURITY_128_BIT")
    seq, pools, got, info = _run(w, seed)
    t0 = time.perf_counter()
    before = w.model.bootstraps
    want = SF.expected(seq, O, w.keys, pools, w.model)
    oracle_s = time.perf_counter() - t0
    assert w.model.bootstraps - before <= SF.MAX_ORACLE_BOOTSTRAPS
    bad = SF.compare(got, want)
    w.report[seed] = (len(seq), SF.adjacency(seq), info["seconds"], oracle_s, sum(len(g) for g in got.values()))
    print(f"seed {seed}: {len(seq)} steps issued in {info['seconds']:.3f} s, model {oracle_s:.2f} s "
          f"({w.model.bootstraps - before} oracle bootstraps), {len(bad)} steps differ")
    assert not bad, f"seed {seed}:\n" + SF.describe(seq, bad, got, want)
    # the key V2 holds after the last step answers a call of its own
    rows = pools["lv0:V2"][:2]
    assert np.array_equal(w.handles["V2"].batch_gate(0, rows, rows[::-1]),
                          O.batch_gate(w.keys["cloud"][SF.final_keys(seq)], 0, rows, rows[::-1]))


@pytest.mark.parametrize("seed", SF.SEEDS["SECURITY_UINT4"])
def test_sequences_uint4(O, seed):
    w = _world(O, "SECURITY_UINT4")
    seq, pools, got, info = _run(w, seed)
    _reset(w, w.alone)
    t0 = time.perf_counter()
    alone, _ = SF.run(SF.as_host(seq), w.alone, w.streams, pools, w.be)
    alone_s = time.perf_counter() - t0
    bad = SF.compare(got, alone)
    w.report[seed] = (len(seq), SF.adjacency(seq), info["seconds"], alone_s, sum(len(g) for g in got.values()))
    print(f"seed {seed}: {len(seq)} steps issued in {info['seconds']:.3f} s, the same calls alone {alone_s:.2f} s, "
          f"{len(bad)} steps differ")
    assert not bad, f"seed {seed}:\n" + SF.describe(seq, bad, got, alone)
    # gate-type outputs on genuine encryptions decrypt to the plaintext model's value (no device in this check)
    key, checked = "K2/gen", 0
    for st in seq:
        if st.kind == "state" and st.op == "key_change":
            key = SF.key_after(st)
        bits = SF.plaintext(st, pools, O)
        if bits is None or (st.handle == "V2" and not key.startswith("K2")):
            continue
        assert np.array_equal(w.secrets[st.handle].decrypt_bool(got[st.i]), bits), st
        checked += 1
    assert checked >= 5


def test_comparison_sees_one_wrong_step(O):
    """One operand of one mid-sequence step (the head of the gate_dev -> pack_dev -> unpack_dev chain) perturbed in the
    model only: exactly that step and the steps chained from it are reported."""
    w = _world(O, "SECURITY_128_BIT")
    seed = SF.SEEDS["SECURITY_128_BIT"][0]
    seq = SF.random_sequence(seed, w.shape)
    if seed not in w.got:
        _run(w, seed)
    head = next(st.i for st in seq if st.kind == "call" and st.op == "gate" and len(SF.cone(seq, st.i)) == 3)
    assert 0 < head < len(seq) - 1
    wrong = SF.expected(seq, O, w.keys, w.pools[seed], w.model, perturb=head)
    assert SF.compare(w.got[seed], wrong) == sorted(SF.cone(seq, head))


_DIRECTED = {}


def test_host_key_switch_after_an_unsynchronised_dev_call(O):
    """unpack_dev of 65,536 slots on a side stream (one slab of the column-sliced key switch), then AT ONCE a host
    batch_identity_key_switch of 400 rows (>= ks_sl_chunk_min: the sliced kernel again, whose digits pass writes the
    start of the context's ks_dig), then both results against the same two calls made alone.  Four rounds, each with
    its own data.

    The pair only means something if the second call is issued while the first still runs: the first call alone is timed
    once with events, and every round asserts that its unpack_dev has not finished when the host call is entered (and
    says so if it has).  Whether it is still unfinished when the host call RETURNS depends on the library: a
    launch_key_switch that claims the scratch drains the side stream first, so the host call returns after it; the
    report line gives both durations and what was seen."""
    import torch

    w = _world(O, "SECURITY_UINT4")
    e, n = w.handles["E"], w.p.n
    _reset(w, w.handles)
    assert "key_switch=sliced" in e.describe_dispatch(400) and "key_switch=sliced" in e.describe_dispatch(65536)
    side = torch.cuda.Stream(device=0)
    rng = np.random.default_rng(7500)
    out = torch.empty((65536, n + 1), dtype=torch.int32, device="cuda:0")
    ref = torch.empty_like(out)
    rounds, first_ms = [], None
    for r in range(4):
        trlwe = w.be.upload(SF.words(rng, (64, 2, N)))
        lv1 = SF.words(rng, (400, N + 1))
        # alone
        e.unpack_dev(trlwe, ref, 65536, stream=side)
        torch.cuda.synchronize()
        if first_ms is None:  # (the run above also grew the scratch: this one is the call as the rounds make it)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(side)
            e.unpack_dev(trlwe, ref, 65536, stream=side)
            b.record(side)
            torch.cuda.synchronize()
            first_ms = a.elapsed_time(b)
        want_ks = e.batch_identity_key_switch(lv1)
        e.synchronize()
        out.fill_(SF.FILL)
        torch.cuda.synchronize()
        # the pair
        done = torch.cuda.Event()
        t0 = time.perf_counter()
        e.unpack_dev(trlwe, out, 65536, stream=side)
        done.record(side)
        running_at_issue = not done.query()
        t1 = time.perf_counter()
        got_ks = e.batch_identity_key_switch(lv1)
        running_at_return = not done.query()
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        wrong_first = int((out != ref).sum().item())
        wrong_second = int((got_ks != want_ks).sum())
        rounds.append((running_at_issue, running_at_return, (t1 - t0) * 1e3, (t2 - t1) * 1e3, wrong_first, wrong_second))
    _DIRECTED["line"] = (f"directed pair: unpack_dev(65536) alone {first_ms:.2f} ms; per round (first still running when the "
                         f"host call was issued / when it returned, ms to issue, ms in the host call, wrong words of the "
                         f"first / second result): "
                         + "; ".join(f"{a}/{b} {x:.2f} {y:.2f} {u}/{v}" for a, b, x, y, u, v in rounds))
    print(_DIRECTED["line"])
    for r, (at_issue, _, issue_ms, _, _, _) in enumerate(rounds):
        assert at_issue and issue_ms < first_ms, \
            f"round {r}: the first call ({first_ms:.2f} ms alone) had finished before the host call was issued " \
            f"({issue_ms:.2f} ms after it): the pair did not overlap on this machine and shows nothing"
    assert [(u, v) for *_, u, v in rounds] == [(0, 0)] * 4, _DIRECTED["line"]


@pytest.mark.parametrize("name", sorted(SF.SHAPES))
def test_report(O, name):
    """What the shape's sequences reached (shown by pytest -rA)."""
    w = _world(O, name)
    for seed in SF.SEEDS[name]:
        if seed not in w.report:
            (test_sequences_128bit if w.shape.exact else test_sequences_uint4)(O, seed)
    rep = [w.report[s] for s in SF.SEEDS[name]]
    c = SF.sum_counts(r[1] for r in rep)
    keep = [k for k in c if not k.startswith(("op ", "form ", "state ", "route ", "chained "))]
    print(f"{name}: {len(rep)} sequences, {sum(r[0] for r in rep)} steps, {sum(r[4] for r in rep)} rows compared word for word")
    print("  adjacency: " + ", ".join(f"{k}: {c[k]}" for k in sorted(keep)))
    print("  forms: " + ", ".join(f"{k[5:]}: {c[k]}" for k in sorted(c) if k.startswith("form ")))
    print("  seconds per sequence (issue to the last synchronisation): " + ", ".join(f"{r[2]:.3f}" for r in rep))
    print(f"  seconds per sequence ({'model' if w.shape.exact else 'the same calls alone'}): " + ", ".join(f"{r[3]:.2f}" for r in rep))
    if name == "SECURITY_UINT4" and "line" in _DIRECTED:
        print("  " + _DIRECTED["line"])
    assert sum(r[0] for r in rep) >= 6 * SF.STEPS
