"""The native circuit scheduler's host side under random circuits (tests/circuit_fuzz.py): the schedule of several
hundred seeded DAGs against an independent model of the levelisation and the fold rule, and the condition the GPU fuzz's
fixed corpus (tests/test_gpu_circuit_fuzz.py) has to meet.  No device."""
import collections

import pytest

import circuit_fuzz as F


def _all_corpus():
    return [c for key in F.CORPUS for c in F.corpus(key)]


def test_generator_is_deterministic():
    a, b = F.random_circuit(17, 4, 50), F.random_circuit(17, 4, 50)
    assert a._nodes == b._nodes and a.motifs == b.motifs and all((x == y).all() for x, y in zip(a._luts, b._luts))
    assert F.random_circuit(18, 4, 50)._nodes != a._nodes


def test_schedule_of_random_circuits():
    """check_schedule over 400 seeds of 1-80 nodes and 1-6 inputs: unique slots, every stored wire in the slot range of
    the level the model derives (never above Python's `_level`), contiguous levels, level sizes from the node list,
    the function-major many-LUT layout, every operand row written before the launch that reads it."""
    strict = 0
    for seed in range(400):
        c = F.random_circuit(seed, 1 + seed % 6, 1 + (7 * seed) % 80)
        level = F.check_schedule(c)
        strict += sum(L < c._level[w] for w, L in level.items())
    assert strict > 0  # the divergence exists: zero and cancelling coefficients lower the native level only


def test_check_schedule_can_fail():
    """Fed the many-LUT layout node-major (node q's k functions side by side) instead of function-major, the check
    fails on a circuit with a group of several nodes -- and on nothing else about that circuit."""
    c = next(c for c in _all_corpus() if any(n == "many_group_of_several" for n, _ in c.motifs))
    F.check_schedule(c)
    with pytest.raises(AssertionError, match="many-LUT layout"):
        F.check_schedule(c, many_layout="node_major")


def test_corpus_condition():
    """Over the GPU test's fixed seed lists: every motif at least three times; levels with a lincomb launch, an nks
    launch, a gate launch, two or more lut launches, a many-LUT launch of two or more nodes; every circuit 20-60
    bootstrap nodes and at least three wide; native level <= Python level everywhere, strictly somewhere."""
    cs = _all_corpus()
    motifs = collections.Counter(n for c in cs for n, _ in c.motifs)
    assert set(motifs) <= set(F.MOTIFS)
    assert all(motifs[m] >= 3 for m in F.MOTIFS), dict(motifs)
    seen = collections.Counter()
    strict = 0
    for c in cs:
        level = F.check_schedule(c)
        strict += sum(L < c._level[w] for w, L in level.items())
        assert 20 <= F.n_bootstraps(c) <= 60 and F.widest_bootstrap_launch(c) >= 3, (c.seed, F.n_bootstraps(c))
        for lv in c.describe():
            seen["lincomb"] += lv["lincomb_launches"] > 0
            seen["nks"] += lv["nks_launches"] > 0
            seen["gate"] += lv["gate_launches"] > 0
            seen["two_lut_launches"] += lv["lut_launches"] >= 2
        for name, w in c.motifs:  # a many-LUT group of >= 2 nodes: the heads' slots are consecutive
            if name == "many_group_of_several":
                k = c._nodes[w - c.n_inputs][7]
                seen["many_group"] += k >= 2 and c.wire_slot(w + 1) - c.wire_slot(w) >= 2
    assert all(seen[k] > 0 for k in ("lincomb", "nks", "gate", "two_lut_launches", "many_group")), dict(seen)
    assert strict > 0
    print("motifs:", dict(motifs), "levels with:", dict(seen))


def test_corpus_serves_every_gpu_case():
    """Per parameter shape: circuits for the pool case (a folded gate on the key's own test vector, a materialised
    lincomb, a mux with a linear operand, a many-LUT group of several nodes -- from the motif lists) and one circuit
    with all three perturbation sites for the sensitivity case."""
    for key in F.SHAPES:
        cs = F.corpus(key)
        assert len(cs) >= 8
        assert len(F.pool_circuits(cs)) >= 2, key
        assert any(len(F.perturbation_sites(c)) == 3 for c in cs), key


def test_cone_and_perturbation():
    import rs_tfhe_amd as R

    c = R.Circuit(3)
    x = c.xor(0, 1)
    n = c.not_(x)
    y = c.and_ny(n, 2)
    z = c.or_(0, 2)
    m = c.mux(y, z, 0)
    assert F.cone(c, x) == {x, n, y, m} and F.cone(c, z) == {z, m} and F.cone(c, 2) == {2, y, z, m}
    assert F.perturbation_sites(c) == {"and_ny_swapped": y}
    p = F.perturbed(c, "and_ny_swapped", y)
    assert p._nodes[y - 3] == ("gate", F.ANDNY, 2, n) and c._nodes[y - 3] == ("gate", F.ANDNY, n, 2)
    assert [a for a, b in zip(p._nodes, c._nodes) if a != b] == [p._nodes[y - 3]]
