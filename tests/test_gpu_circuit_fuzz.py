"""The native circuit scheduler on the GPU under random circuits (tests/circuit_fuzz.py): every word of every wire of
every row against the CPU oracle evaluating the same nodes one by one.  Custom parameter shapes in the exact-product
regime (every word has one right answer; small n keeps the oracle cheap) plus SECURITY_80_BIT; the default dispatch in
every regime its plan can produce, with the circuit's per-row index gathers; pools of two and three members on one GPU;
subset gathers; plan eviction; and a check that the comparison notices ONE wrong operand.  No tolerance anywhere.

Large batches are periodic in the batch with period 7 (`inputs[:, j] = base[:, j % 7]`): rows never interact, so the
oracle evaluates 7 rows and ALL B rows are compared with the tiled result.  (A mis-index by a multiple of 7 rows would
hide behind that: test_distinct_rows uses 24 different rows.)"""
import collections
import ctypes as C
import re
import time

import numpy as np
import pytest

import circuit_fuzz as F

pytestmark = pytest.mark.gpu
PERIOD = 7
ROUNDING = {F.SHAPES[0]: "fast", F.SHAPES[1]: "fast", F.SHAPES[2]: "general"}  # log2(2l) + 10 + (bgbit - 1) + 31 < 51
PART = r"\[\d+,\d+\)"
REGIMES = {  # the blind-rotation plans of plan_blind_rotate (tfhe_hip_describe_dispatch prints them)
    "single": rf"single{PART}", "pair": rf"pair{PART}", "pair+single": rf"pair{PART}\+single{PART}",
    "batch": rf"batch{PART}", "batch+single": rf"batch{PART}\+single{PART}", "batch+pair": rf"batch{PART}\+pair{PART}",
}
L1_CANNOT = {"pair+single", "batch+pair"}  # plan_blind_rotate: not at l = 1


class Ctx:
    pass


@pytest.fixture(scope="module", params=F.SHAPES, ids=lambda s: "n%d_l%d_bg%d" % s[:3])
def ctx(request, O):
    """One parameter shape: oracle keys, the product's key, an Engine of its own, the shape's corpus."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import SecurityParams

    n, l, bgbit, basebit, t = request.param
    op = O.Params(f"CFUZZ_{n}_{l}_{bgbit}", n, l, bgbit, basebit, t, 2.0e-5, 2.0e-8)
    x = Ctx()
    x.shape, x.n, x.l = request.param, n, l
    x.sk, x.ck = O.keygen(op, 6100 + n)
    x.pp = SecurityParams(op.name, 0, n, l, bgbit, basebit, t, op.alpha_lv0, op.alpha_lv1)
    x.pk = R.CloudKey(x.pp, x.ck.bootstrapping_key, x.ck.key_switching_key, x.ck.decomposition_offset, x.ck.blind_rotate_testvec)
    x.circuits = F.corpus(request.param)
    x.base, x.ref7, x.report = {}, {}, collections.OrderedDict()
    x.rows = 0
    x.eng = R.Engine(x.pp, 0)
    try:
        x.eng.load_cloud_key(x.pk)
        yield x
    finally:
        for c in x.circuits:
            c._drop_native()  # its plans' device memory goes before the context does
        x.eng.close()


def _words(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def _base(O, x, c):
    """(7 uniformly random input rows, every wire of them on the oracle) of corpus circuit `c`, computed once."""
    if c.seed not in x.ref7:
        x.base[c.seed] = _words(np.random.default_rng(9000 + c.seed), (c.n_inputs, PERIOD, x.n + 1))
        t0 = time.time()
        x.ref7[c.seed] = F.reference(c, O, x.ck, x.base[c.seed])
        x.report.setdefault("oracle seconds", []).append(round(time.time() - t0, 2))
    return x.base[c.seed], x.ref7[c.seed]


def _tiled(a, B):
    return np.ascontiguousarray(a[:, np.arange(B) % PERIOD])


def _dev(c, handle, inputs):
    import torch

    got = c.run_dev(handle, torch.from_numpy(inputs.view(np.int32)).to("cuda:0"))
    handle.synchronize()
    torch.cuda.synchronize()
    return got.cpu().numpy().view(np.uint32)


def _same(x, got, want, what):
    """Every word of every wire of every row."""
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = sorted({int(w) for w in np.argwhere((got != want).any(axis=2))[:, 0]})
        rows = sorted({int(r) for r in np.argwhere((got != want).any(axis=2))[:, 1]})[:12]
        raise AssertionError(f"{what}: wires {bad} differ (first rows {rows})")
    x.rows += got.shape[0] * got.shape[1]


def _plan(eng, count):
    return eng.describe_dispatch(count).split()[0].split("=", 1)[1]


def _batches_for(eng, W, regime, members=None):
    """The batches B >= 8 (not multiples of the period) whose widest launch, W x B ciphertexts, the default dispatch
    runs as `regime`: the smallest (just past the crossover: the shortest second part) and one from the middle of the
    regime (a second part of a hundred rows or more); [] if no batch does."""
    hits = [B for B in range(8, 8192 // W + 1) if B % PERIOD and re.fullmatch(REGIMES[regime], _plan(eng, W * B))
            and (members is None or members[0].members_for(W * B) == members[1])]
    first = [B for B in hits if B < hits[0] + 1024 // W]  # the regime's first stretch (those with a batch part recur)
    return sorted({first[0], first[len(first) // 2]}) if first else []


def test_rounding_modes(ctx):
    assert ctx.eng.rounding_mode == ROUNDING[ctx.shape]
    assert set(ROUNDING.values()) == {"fast", "general"}
    assert len(ctx.circuits) >= 8


def test_engine_host_arrays(O, ctx):
    """(a) c.run(eng, inputs) at B = 7 and B = 1: all wires equal the reference."""
    for c in ctx.circuits:
        base, ref = _base(O, ctx, c)
        _same(ctx, c.run(ctx.eng, base), ref, f"seed {c.seed} B=7")
        _same(ctx, c.run(ctx.eng, base[:, :1]), ref[:, :1], f"seed {c.seed} B=1")


def test_dispatch_regimes_with_index_gathers(O, ctx):
    """(b) For every circuit and every blind-rotation plan the default dispatch can produce, the batch B at which the
    circuit's widest launch (W x B rows, gathered by per-row indices) runs under that plan -- asked of
    describe_dispatch, the crossovers follow the CU count -- through run() and run_dev(): the tiled reference.
    Every regime is reached by at least two circuits; at l = 1 exactly `pair+single` and `batch+pair` are not."""
    reached = collections.OrderedDict((r, []) for r in REGIMES)
    for c in ctx.circuits:
        base, ref = _base(O, ctx, c)
        W = F.widest_bootstrap_launch(c)
        assert W >= 3
        for regime, B in ((r, B) for r in REGIMES for B in _batches_for(ctx.eng, W, r)):
            plan = _plan(ctx.eng, W * B)
            assert re.fullmatch(REGIMES[regime], plan), (regime, plan)
            reached[regime].append((c.seed, W, B, plan))
            inputs, want = _tiled(base, B), _tiled(ref, B)
            _same(ctx, c.run(ctx.eng, inputs), want, f"seed {c.seed} {regime} B={B} [{plan}] run")
            _same(ctx, _dev(c, ctx.eng, inputs), want, f"seed {c.seed} {regime} B={B} [{plan}] run_dev")
    ctx.report["regimes (seed, W, B, plan)"] = reached
    missing = {r for r, hit in reached.items() if not hit}
    assert missing == (L1_CANNOT if ctx.l == 1 else set()), missing
    assert all(len({seed for seed, *_ in hit}) >= 2 for r, hit in reached.items() if r not in missing), reached


def test_pools_of_two_and_three(O, ctx):
    """(c) R.Pool(pp, [0, 0]) and R.Pool(pp, [0, 0, 0]) (uneven shares), every home, run() and run_dev(), at B = 7 and at
    a batch whose widest launch is cut over every member: the engine's words and the reference.  The circuits hold
    folded gates on the key's own test vector, a materialised lincomb, a mux with a linear operand and a many-LUT group
    of several nodes."""
    import rs_tfhe_amd as R

    cs = F.pool_circuits(ctx.circuits)[:2]
    assert len(cs) == 2
    for c in cs:
        names = {n for n, _ in c.motifs}
        assert all(names & set(alt) for alt in F.POOL_NEEDS), names
    used = []
    for members in (2, 3):
        pool = R.Pool(ctx.pp, [0] * members)
        try:
            pool.load_cloud_key(ctx.pk)
            for c in cs:
                base, ref = _base(O, ctx, c)
                W = F.widest_bootstrap_launch(c)
                big = _batches_for(ctx.eng, W, "batch+single", (pool, members))[-1]
                assert pool.members_for(W * big) == members
                for B in (PERIOD, big):
                    inputs, want = _tiled(base, B), _tiled(ref, B)
                    _same(ctx, c.run(ctx.eng, inputs), want, f"seed {c.seed} engine B={B}")
                    _same(ctx, c.run(pool, inputs), want, f"seed {c.seed} pool[{members}] run B={B}")
                    for home in range(members):
                        pool.home = home
                        _same(ctx, _dev(c, pool, inputs), want, f"seed {c.seed} pool[{members}] home {home} run_dev B={B}")
                    pool.home = 0
                    used.append((members, c.seed, B))
        finally:
            for c in cs:
                c._drop_native()
            pool.close()
    ctx.report["pool (members, seed, B)"] = used


def test_distinct_rows(O, ctx):
    """(d) B = 24 with 24 DIFFERENT random rows (nothing periodic): engine run / run_dev and a two-member pool against
    the reference computed for all 24 rows."""
    import rs_tfhe_amd as R

    c = F.pool_circuits(ctx.circuits)[0]
    inputs = _words(np.random.default_rng(9500 + c.seed), (c.n_inputs, 24, ctx.n + 1))
    want = F.reference(c, O, ctx.ck, inputs)
    _same(ctx, c.run(ctx.eng, inputs), want, f"seed {c.seed} distinct run")
    _same(ctx, _dev(c, ctx.eng, inputs), want, f"seed {c.seed} distinct run_dev")
    pool = R.Pool(ctx.pp, [0, 0])
    try:
        pool.load_cloud_key(ctx.pk)
        _same(ctx, c.run(pool, inputs), want, f"seed {c.seed} distinct pool run")
        pool.home = 1
        _same(ctx, _dev(c, pool, inputs), want, f"seed {c.seed} distinct pool run_dev")
    finally:
        c._drop_native()
        pool.close()


def test_gather_subsets(O, ctx):
    """(e) tfhe_hip_circuit_gather_dev after one tfhe_hip_circuit_run_dev: all wires; a reversed subset with linear
    wires and a repeated wire; a different subset of the same length; the first subset again (the cached CSR is
    rewritten in between) -- each the rows of the first.  A wire index >= n_wires: EINVAL, nothing written."""
    import torch

    from rs_tfhe_amd import _capi

    lib, eng = _capi.lib(), ctx.eng
    c = ctx.circuits[1]
    base, ref = _base(O, ctx, c)
    B, w = PERIOD, ctx.n + 1
    h = c._native_handle()
    sp = eng._stream_ptr(eng.home, None)
    t_in = torch.from_numpy(base.view(np.int32)).to("cuda:0")
    store = torch.empty((c.slots, B, w), dtype=torch.int32, device="cuda:0")
    eng._chk(lib.tfhe_hip_circuit_run_dev(eng._ctx, h, eng._tp(eng.home, t_in), eng._tp(eng.home, store), B, sp))

    def gather(wires):
        idx = np.array(wires, np.uint32)
        out = torch.full((len(idx), B, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        rc = lib.tfhe_hip_circuit_gather_dev(eng._ctx, h, eng._tp(eng.home, store), B, idx.ctypes.data_as(C.c_void_p), len(idx),
                                             eng._tp(eng.home, out), sp)
        torch.cuda.synchronize()
        return rc, out.cpu().numpy().view(np.uint32)

    rc, every = gather(range(c.n_wires))
    assert rc == _capi.OK
    _same(ctx, every, ref, f"seed {c.seed} gather of all wires")
    lin = [x for x in range(c.n_wires) if F.is_linear(c, x)]
    assert len(lin) >= 4
    rng = np.random.default_rng(9600)
    sub1 = sorted({int(x) for x in rng.choice(c.n_wires, 9, replace=False)} | set(lin[:3]), reverse=True)
    sub1.append(sub1[2])  # a wire twice
    sub2 = [int(x) for x in rng.choice(c.n_wires, len(sub1))]
    assert sub2 != sub1 and set(sub2) - set(sub1)
    for sub in (sub1, sub2, sub1, [c.n_wires - 1]):
        rc, got = gather(sub)
        assert rc == _capi.OK
        _same(ctx, got, every[sub], f"seed {c.seed} gather of {sub}")
    rc, got = gather([0, c.n_wires, 1])
    assert rc == _capi.EINVAL and (got == 0x5A5A5A5A).all()
    rc, got = gather(sub1)  # and the plan is as good as before
    assert rc == _capi.OK and np.array_equal(got, every[sub1])


def _free_bytes():
    import torch

    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info(0)[0]


def test_plan_eviction(O, ctx):
    """(f) One circuit at six batch sizes in turn, then the first again (a circuit keeps four plans: two are evicted,
    then the first is rebuilt): the same words each time.  Device memory: device-resident runs (a plan holds its
    index arrays only) leave it where it was after the first run; host-array runs (a plan holds its store too, 16 MiB
    here) may keep three more plans than after the first run and nothing beyond that, and a second pass of the
    same seven runs -- five more evictions -- adds nothing."""
    c = ctx.circuits[2]
    base, ref = _base(O, ctx, c)
    slack = 8 << 20
    row = c.slots * (ctx.n + 1) * 4
    B0 = 2 * slack // row + 6  # a plan's store is 16 MiB or more: one that was not given back would show
    Bs = list(range(B0, B0 - 6, -1))  # the largest first: the context's own scratch is at its size from then on
    store = row * B0

    def once(run, B):
        _same(ctx, run(_tiled(base, B)), _tiled(ref, B), f"seed {c.seed} B={B}")

    c._drop_native()  # no plan of an earlier test
    dev = lambda inputs: _dev(c, ctx.eng, inputs)  # noqa: E731
    once(dev, Bs[0])
    first = _free_bytes()
    for B in Bs[1:] + Bs[:1]:
        once(dev, B)
    assert first - _free_bytes() < slack
    c._drop_native()
    host = lambda inputs: c.run(ctx.eng, inputs)  # noqa: E731
    once(host, Bs[0])
    first = _free_bytes()
    for B in Bs[1:] + Bs[:1]:
        once(host, B)
    settled = _free_bytes()
    # a cached plan: its store with the allocator's quarter of headroom, at most 9 bytes of indices and gate codes per
    # store row, and up to 2 MiB of allocation granularity on each of its three buffers
    plan = store + store // 4 + 9 * c.slots * B0 + 3 * (2 << 20)
    assert first - settled < 3 * plan + slack, (first - settled) >> 20
    for B in Bs[1:] + Bs[:1]:
        once(host, B)
    assert settled - _free_bytes() < slack
    c._drop_native()


def test_comparison_sees_one_wrong_operand(O, ctx):
    """(g) The same circuit with ONE node perturbed (operands of an and_ny swapped; ca and cb of a pbs exchanged; the
    function index of a many-LUT consumer moved by one): the GPU result of the ORIGINAL differs from the reference of
    the perturbed circuit on that wire, and on nothing outside the wires that depend on it."""
    c = next(c for c in ctx.circuits if len(F.perturbation_sites(c)) == 3)
    base, ref = _base(O, ctx, c)
    inputs = base[:, :2]
    got = c.run(ctx.eng, inputs)
    _same(ctx, got, ref[:, :2], f"seed {c.seed} B=2")
    for kind, wire in F.perturbation_sites(c).items():
        wrong = F.reference(F.perturbed(c, kind, wire), O, ctx.ck, inputs)
        differs = {w for w in range(c.n_wires) if not np.array_equal(got[w], wrong[w])}
        assert wire in differs and differs <= F.cone(c, wire), (kind, wire, sorted(differs))
    ctx.report["one wrong operand seen at (seed, sites)"] = (c.seed, F.perturbation_sites(c))


def test_report(ctx):
    """What the shape's tests reached (shown by pytest -rA)."""
    motifs = collections.Counter(n for c in ctx.circuits for n, _ in c.motifs)
    print(f"shape {ctx.shape}: {len(ctx.circuits)} circuits, {sum(c.n_wires - c.n_inputs for c in ctx.circuits)} nodes, "
          f"{sum(F.n_bootstraps(c) for c in ctx.circuits)} bootstrap nodes, {ctx.rows} wire rows compared word for word")
    print("motifs:", dict(motifs))
    for k, v in ctx.report.items():
        if isinstance(v, dict):
            print(k)
            for r, hit in v.items():
                print(f"  {r}: {len({seed for seed, *_ in hit})} circuits, {len(hit)} batches {hit}")
        else:
            print(f"{k}: {v}")
    assert ctx.rows > 0


def test_security_80_bit(O, keys80):
    """Two corpus circuits at a reference parameter set (n = 550), B = 3, run() and run_dev(): the reference."""
    from test_gpu_circuit import _engine

    sk, ck = keys80
    eng = _engine(ck)
    x = Ctx()
    x.rows = 0
    for c in F.corpus("SECURITY_80_BIT"):
        inputs = _words(np.random.default_rng(9700 + c.seed), (c.n_inputs, 3, ck.params.n + 1))
        want = F.reference(c, O, ck, inputs)
        _same(x, c.run(eng, inputs), want, f"seed {c.seed} 80 bit run")
        _same(x, _dev(c, eng, inputs), want, f"seed {c.seed} 80 bit run_dev")
