"""Sequence fuzz on the GPU (tests/sequence_fuzz.py): any order of calls, forms and streams on one context and its key
views, with no synchronisation between the steps.

SECURITY_128_BIT (the exact-product regime): every word of every row of every step against the model (the CPU oracle
under the key the handle holds at that step; packing.pack_model / key_switch_model / table_model for the key-switch
forms the reference lacks), the loaded flags after the last step, and tfhe_hip_get_kernel_times after every profiling
toggle.  SECURITY_UINT4 (l = 1, general rounding, the column-sliced key switch, inexact products): the property is
order-independence, so the reference is THE SAME CALL MADE ALONE -- every step by its host form on a second context
with the same keys, a synchronisation after each -- word for word (kernels agree bit for bit across forms and counts:
test_dispatch_crossovers_bit_exact; isolated calls are held to the oracle by the other suites); and every gate-type
output on genuine encryptions decrypts to its truth table, and the two chains that start in a fresh encryption
(encrypt -> tlwe_matmul -> decrypt; encrypt_trlwe -> polymul -> trlwe_matmul -> decrypt) end in the plaintext product
within 8 sigma of the encryption noise, by a computation that uses neither the device nor the library.  A directed test
holds the one pair found by reading: a host key switch issued while an un-synchronised unpack_dev still walks the shared
digit scratch; a second one the pair of the staged secrets: a host decryption under another view's key issued while an
un-synchronised encrypt_trlwe_dev still reads the context's one buffer of them.

The steps cover gates, bootstraps, the packing and table key switches, and -- with real noise, keys and indices of
their own per step -- public-key and symmetric encryption, packed encryption and expansion, decryption, the dense and
packed linear layers, the convolution and the polynomial product.

The ring steps -- the TRLWE key switch, the packed CMUX with caller-held selectors, TRGSW encryption, the switching-key
changes (generated under queued work, loaded, dropped and loaded; another (basebit, t) each time, and no drain but the
library's own) and the getters of their timing pairs -- run in both shapes: every word against trlwe_switch_model and
cmux_model (exact in integers on every parameter set, so on SECURITY_UINT4 too, beside the same call made alone), the
chunk passes each ring_times step reports against the sequence, the switching key each view holds after the last step
by a two-row switch under it, and chains E (encrypt_trlwe -> trlwe_keyswitch -> decrypt_trlwe) and F (encrypt_trgsw ->
cmux -> trlwe_keyswitch -> decrypt_trlwe) against psi_k of their plaintexts within 8 sigma of the encryption, the CMUX
and the switch.  A third directed pair holds the two views' key tables over one ts_dig: a host switch on V2 issued
while an un-synchronised trlwe_keyswitch_dev of the same k on E still runs pass after pass through the digit scratch
(measured: 16,384 ciphertexts last 2.31 ms alone against 0.09 ms to issue; the host call was entered 0.08 ms after it,
found it running in all four rounds and returned 2.6 - 2.7 ms later; no wrong word).
Narrower than the full cross product: TRGSW encryption's device form has no stream, VR runs none of this, switching
keys keep s_from = s_to.

The six sequences of a shape run on one context, seed after seed, and scratch never shrinks: the grow step of seed s
is 1.5 x that of seed s - 1 (more than ensure()'s quarter of headroom), so each of them reallocates under in-flight
work, not only the first.  The ring families' digit scratch cannot rise that way: ts_dig and cm_dig are capped at 2,048
ciphertexts of the largest t, so they are reallocated under running calls in the first two or three sequences of a
shape only, and the ring grow and "through t alone" steps of the later sequences hold the order of
the calls alone (sequence_fuzz.py says what that leaves uncovered).

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
    w.secrets = {"E": w.sk["K1"], "V2": w.sk["K2"], "VR": w.sk["K1"]}
    # the switching keys (s_from = s_to = the handle's ring key), each generated once under its fixed generator key and
    # downloaded: what each view starts with and what a switch_key_change brings, by any of its routes
    w.switch_book = {}
    tmp = w.eng.new_key_view()
    try:
        for key in SF.switch_book_names():
            h, k = key.split(":")[:2]
            ring = w.secrets[h].key_lv1
            w.switch_book[key] = tmp.gen_trlwe_switch_key(ring, ring, int(k), *SF.switch_key_gadget(key), rng_key=SF.switch_gen_key(key))
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
        # a public key beside each cloud key, under the handle's own secret (a fixed generator key: the same words on
        # every context); a key change on V2 leaves it in place
        public = {h: x.gen_public_key(w.secrets[h].key_lv0, size=SF.PK_SIZE, rng_key=SF.PK_GEN_KEY) for h, x in (("E", eng), ("V2", v2))}
        assert all(np.array_equal(public[h], w.public.setdefault(h, public[h])) for h in public)
        return {"E": eng, "V2": v2, "VR": vr, "book": w.book, "packing": w.packing, "combining_default": w.default_combining,
                "secrets": w.secrets, "switch_book": w.switch_book}

    w.public = {}
    w.handles = handles(w.eng)
    w.alone = None
    if not w.shape.exact:
        w.eng2 = R.Engine(p, 0)
        w.eng2.gen_cloud_key(w.sk["K1"].key_lv0, w.sk["K1"].key_lv1, seed=7201)  # the seeded generator: the same key
        w.alone = handles(w.eng2)
    w.be = SF.TorchBackend()
    w.streams = w.be.streams()
    w.keys = w.model = None
    # the ring steps need no cloud key: a model of them alone where the oracle gives no words
    w.ring_keys = {"params": p, "switch": w.switch_book, "secrets": w.secrets}
    w.ring_model = SF.Model(None, w.ring_keys)
    if w.shape.exact:
        cloud = {k: O.CloudKey.from_arrays(w.op, c.bootstrapping_key, c.key_switching_key, c.decomposition_offset,
                                           c.blind_rotate_testvec) for k, c in exported.items()}
        w.keys = {"params": p, "oracle_params": w.op, "cloud": cloud, "reenc": w.reenc, "secrets": w.secrets, "public": w.public,
                  "packing": {h: (pk, PK.key_rows(p, pk.mask_seed, pk.bodies)) for h, pk in w.packing.items()},
                  "switch": w.switch_book}
        w.model = w.ring_model = SF.Model(O, w.keys)
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
    """Where every sequence starts: V2 under K2 (as generated), each view's starting switching keys, profiling off and
    its timing pairs drained, the default combining, nothing queued."""
    handles["V2"].load_cloud_key(w.book["K2/gen"]["full"])
    for h, held in SF.switch_keys_after([], -1).items():
        for name in held.values():
            handles[h].load_trlwe_switch_key(w.switch_book[name])
    handles["E"].set_profiling(False)
    handles["E"].kernel_times()
    handles["E"].trlwe_switch_times()
    handles["E"].cmux_times()
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
    SF.check_ring_times(seq, info)  # tfhe_hip_get_trlwe_switch_times / _cmux_times: the passes issued while profiling was on
    for h in SF.HANDLES:
        assert SF.flags(w.handles[h]) == SF.EXPECTED_FLAGS[h], (h, SF.flags(w.handles[h]))
    SF.final_switch_check(seq, w.handles, pools, w.ring_model)  # the switching keys each view holds after the last step
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
    assert SF.chains_decrypt_to_their_plaintext_products(w.shape, w.secrets, seq, got, pools, ("E", "F")) == 2
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
    # the ring steps (exact in integers on every set), TRGSW encryption and chains E and F: the numpy model, word for word
    t0 = time.perf_counter()
    only = {st.i for st in seq if st.ring or st.op == "encrypt_trgsw" or st.args.get("chain") in ("E", "F")}
    want = SF.expected(seq, None, w.ring_keys, pools, w.ring_model, only=only)
    bad = [i for i in sorted(want) if got[i].shape != want[i].shape or not np.array_equal(got[i], want[i])]
    print(f"seed {seed}: {len(want)} ring steps against the numpy model in {time.perf_counter() - t0:.2f} s, {len(bad)} differ")
    assert sorted(want) == sorted(only) and not bad, f"seed {seed}:\n" + SF.describe(seq, bad, got, want)
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
    checked += SF.chains_decrypt_to_their_plaintext_products(w.shape, w.secrets, seq, got, pools)
    assert checked >= 7


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
    # and the head of chain E (encrypt_trlwe -> trlwe_keyswitch -> decrypt_trlwe)
    head = next(st.i for st in seq if st.kind == "call" and st.op == "encrypt_trlwe" and st.args.get("chain") == "E")
    assert len(SF.cone(seq, head)) == 3
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


PAIR_WORDS = 64 << 20  # plaintext words of the second directed pair's first call


def test_host_decrypt_after_an_unsynchronised_encrypt_trlwe(O):
    """batch_encrypt_trlwe_dev on a side stream under K1's ring key (E stages K, s1 [N] and the spectrum of s1 in the
    context's sym_sec), then AT ONCE a host batch_decrypt (bool, lv0) of 400 rows under K2's key on the key view V2
    (another view, another key, another layout of the same sym_sec: 64 words of key bits), then both results against
    the same two calls made alone.  Four rounds, each with its own data, keys and group indices.

    As in the pair above, the first call alone is timed once with events, and every round asserts that it had not
    finished when the host call was entered.  Its size is the smallest power-of-two count of plaintext words for which
    the call alone lasts at least ten times the time it takes to issue it, capped at 64 Mi: measured on an MI355X,
    doubling from 16 Ki, no smaller count got there, and 64 Mi words (65,536 groups, 512 MiB of ciphertexts) last
    0.73 - 0.75 ms alone against 0.05 - 0.07 ms to issue.  In the rounds the host call was entered 0.06 - 0.09 ms after the
    first, which was still running all four times, and returned 0.74 - 0.78 ms later, after it had finished: the claim on
    sym_sec makes the host call wait for the side stream; without one it would stage K2's bits under the running
    kernel.  0 wrong words in both results."""
    import torch

    w = _world(O, "SECURITY_UINT4")
    e, v2, p = w.handles["E"], w.handles["V2"], w.p
    _reset(w, w.handles)
    side = torch.cuda.Stream(device=0)
    rng = np.random.default_rng(7600)
    k1, k2 = w.sk["K1"].key_lv1, w.sk["K2"].key_lv0
    words = PAIR_WORDS

    def encrypt(plain, keys, out):
        e.batch_encrypt_trlwe_dev(k1, plain, p.alpha_lv1, keys[0], keys[1], keys[2], out=out, stream=side)

    def fresh_keys():
        return rng.integers(0, 256, 32).astype(np.uint8).tobytes(), rng.integers(0, 256, 32).astype(np.uint8).tobytes(), \
            int(rng.integers(0, 1 << 40))

    plain = w.be.upload(SF.words(rng, words))
    ref = torch.empty((words // N, 2, N), dtype=torch.int32, device="cuda:0")
    keys = fresh_keys()
    encrypt(plain, keys, ref)  # (grows sym_sec and warms the kernels)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(side)
    t0 = time.perf_counter()
    encrypt(plain, keys, ref)
    issue_alone_ms = (time.perf_counter() - t0) * 1e3
    b.record(side)
    torch.cuda.synchronize()
    first_ms = a.elapsed_time(b)
    out = torch.empty_like(ref)
    rounds = []
    for r in range(4):
        plain = w.be.upload(SF.words(rng, words))
        keys = fresh_keys()
        cts = w.sk["K2"].encrypt_bool(rng.integers(0, 2, 400).astype(bool), 7610 + r)
        # alone
        encrypt(plain, keys, ref)
        torch.cuda.synchronize()
        want_bits = v2.batch_decrypt(k2, cts, "bool")
        v2.synchronize()
        assert np.array_equal(want_bits.astype(bool), w.sk["K2"].decrypt_bool(cts))
        out.fill_(SF.FILL)
        torch.cuda.synchronize()
        # the pair
        done = torch.cuda.Event()
        t0 = time.perf_counter()
        encrypt(plain, keys, out)
        done.record(side)
        running_at_issue = not done.query()
        t1 = time.perf_counter()
        got_bits = v2.batch_decrypt(k2, cts, "bool")
        running_at_return = not done.query()
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        wrong_first = int((out != ref).sum().item())
        wrong_second = int((got_bits != want_bits).sum())
        rounds.append((running_at_issue, running_at_return, (t1 - t0) * 1e3, (t2 - t1) * 1e3, wrong_first, wrong_second))
    _DIRECTED["line2"] = (f"directed pair: encrypt_trlwe_dev({words} words) alone {first_ms:.2f} ms, {issue_alone_ms:.3f} ms to issue; per "
                          f"round (first still running when the host decrypt was issued / when it returned, ms to issue, ms in "
                          f"the host call, wrong words of the first / second result): "
                          + "; ".join(f"{a}/{b} {x:.2f} {y:.2f} {u}/{v}" for a, b, x, y, u, v in rounds))
    print(_DIRECTED["line2"])
    for r, (at_issue, _, issue_ms, _, _, _) in enumerate(rounds):
        assert at_issue and issue_ms < first_ms, \
            f"round {r}: the first call ({first_ms:.2f} ms alone) had finished before the host call was issued " \
            f"({issue_ms:.2f} ms after it): the pair did not overlap on this machine and shows nothing"
    assert [(u, v) for *_, u, v in rounds] == [(0, 0)] * 4, _DIRECTED["line2"]


PAIR_SWITCH_START, PAIR_SWITCH_CAP = 16384, 65536  # ciphertexts of the third directed pair's first call


def test_host_switch_after_an_unsynchronised_trlwe_keyswitch_dev(O):
    """trlwe_keyswitch_dev (k = 1) of many ciphertexts on a side stream under E's (4, 6) key (pass after pass of 2,048
    through the context's ts_dig), then AT ONCE a host batch_trlwe_keyswitch of 65 ciphertexts under the same k on the key
    view V2 -- V2's own table, its (2, 16) key, and the start of the same ts_dig -- then both results against the same
    two calls made alone.  Four rounds, each with its own data.

    As in the pairs above, the first call alone is timed once with events, and every round asserts that it had not
    finished when the host call was entered.  Its size is the smallest power of two from 16,384 ciphertexts for which
    the call alone lasts at least ten times the time it takes to issue it, capped at 65,536 (512 MiB in, 512 MiB out).
    Measured on an MI355X: the first size tried, 16,384 ciphertexts (128 MiB in, 128 MiB out, eight passes), lasts
    2.31 ms alone against 0.09 ms to issue, so no larger one was needed.  In the rounds the host switch on V2 was entered
    0.08 ms after the first call, which was still running all four times, and returned 2.6 - 2.7 ms later, after it had
    finished: the claim on the context's scratch makes the host call wait for the side stream; without one its digits
    pass would write V2's 65 x 16 digit rows under the running contraction.  0 wrong words in both results."""
    import torch

    w = _world(O, "SECURITY_UINT4")
    e, v2 = w.handles["E"], w.handles["V2"]
    _reset(w, w.handles)
    assert SF.SWITCH_START["E"][1] == (4, 6) and SF.SWITCH_START["V2"][1] == (2, 16)
    side = torch.cuda.Stream(device=0)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(7700)
    rng = np.random.default_rng(7700)

    def fresh(count):
        return torch.randint(-(1 << 31), (1 << 31) - 1, (count, 2, N), dtype=torch.int32, device="cuda:0", generator=gen)

    count, tried = PAIR_SWITCH_START, []
    while True:
        cts = fresh(count)
        ref = torch.empty_like(cts)
        e.batch_trlwe_keyswitch(1, cts, out=ref, stream=side)  # (grows ts_dig and warms the kernels)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(side)
        t0 = time.perf_counter()
        e.batch_trlwe_keyswitch(1, cts, out=ref, stream=side)
        issue_alone_ms = (time.perf_counter() - t0) * 1e3
        b.record(side)
        torch.cuda.synchronize()
        first_ms = a.elapsed_time(b)
        tried.append((count, first_ms, issue_alone_ms))
        if first_ms >= 10.0 * issue_alone_ms or count >= PAIR_SWITCH_CAP:
            break
        del cts, ref
        count *= 2
    out = torch.empty_like(ref)
    rounds = []
    for r in range(4):
        cts = fresh(count)
        small = SF.words(rng, (65, 2, N))
        # alone
        e.batch_trlwe_keyswitch(1, cts, out=ref, stream=side)
        torch.cuda.synchronize()
        want_small = v2.batch_trlwe_keyswitch(1, small)
        v2.synchronize()
        out.fill_(SF.FILL)
        torch.cuda.synchronize()
        # the pair
        done = torch.cuda.Event()
        t0 = time.perf_counter()
        e.batch_trlwe_keyswitch(1, cts, out=out, stream=side)
        done.record(side)
        running_at_issue = not done.query()
        t1 = time.perf_counter()
        got_small = v2.batch_trlwe_keyswitch(1, small)
        running_at_return = not done.query()
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        wrong_first = int((out != ref).sum().item())
        wrong_second = int((got_small != want_small).sum())
        rounds.append((running_at_issue, running_at_return, (t1 - t0) * 1e3, (t2 - t1) * 1e3, wrong_first, wrong_second))
    # (the two views' keys differ: the same small call on E gives other words)
    assert not np.array_equal(e.batch_trlwe_keyswitch(1, small), want_small)
    _DIRECTED["line3"] = (f"directed pair: trlwe_keyswitch_dev({count}) alone {first_ms:.2f} ms, {issue_alone_ms:.3f} ms to issue (sizes "
                          f"tried: " + ", ".join(f"{c}: {x:.2f} / {y:.3f}" for c, x, y in tried) + "); per round (first still running "
                          f"when issued / when the host switch on V2 returned, ms to issue, ms in the host call, wrong words of "
                          f"the first / second result): "
                          + "; ".join(f"{a}/{b} {x:.2f} {y:.2f} {u}/{v}" for a, b, x, y, u, v in rounds))
    print(_DIRECTED["line3"])
    for r, (at_issue, _, issue_ms, _, _, _) in enumerate(rounds):
        assert at_issue and issue_ms < first_ms, \
            f"round {r}: the first call ({first_ms:.2f} ms alone) had finished before the host call was issued " \
            f"({issue_ms:.2f} ms after it): the pair did not overlap on this machine and shows nothing"
    assert [(u, v) for *_, u, v in rounds] == [(0, 0)] * 4, _DIRECTED["line3"]


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
    if name == "SECURITY_UINT4":
        for key in ("line", "line2", "line3"):
            if key in _DIRECTED:
                print("  " + _DIRECTED[key])
    assert sum(r[0] for r in rep) >= 6 * SF.STEPS
