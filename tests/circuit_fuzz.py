"""Random circuits for the native circuit scheduler (tfhe_hip_circuit_*): a seeded DAG generator over the Python
`Circuit` API, the named constructs ("motifs") that force one scheduler path each, an independent model of the
levelisation and of the fold rule to hold the host-side schedule to, the CPU-oracle reference of a circuit, and the
fixed corpus the host and GPU fuzz tests share.  A plain module (no tests in it), like closed_forms.py."""
import bisect

import numpy as np

NO_SLOT = 0xFFFFFFFF
COPY = 10
ANDNY = 6
M32 = 0xFFFFFFFF

# coefficients that make terms merge, cancel and vanish (2^31 doubles to zero)
COEFS = (0, 1, 1, 2, 3, 5, M32, M32 - 1, 1 << 31)
NONZERO = (1, 2, 3, M32, M32 - 1)

MOTIFS = (
    "fold_to_gate_code", "fold_swapped", "fold_own_launch", "fold_cancels", "same_wire_twice", "copy", "constant_operand",
    "materialise_for_gate", "materialise_for_mux", "materialise_for_pbs", "materialised_twice", "lin_of_lin",
    "lin_output_only", "pbs_two_lin_operands_fold", "pbs_cb_zero_lin_operand", "many_group_of_several",
    "two_lut_groups_one_level", "zero_coefficient_term", "mux_chain",
)

# (ca, cb, cconst) of the gate codes 0..10 (src/gates.rs:54-150; COPY bootstraps a itself)
_E8, _Q4 = 0x20000000, 0x40000000
GATE_COEFS = ((M32, M32, _E8), (1, 1, _E8), (1, 1, -_E8 & M32), (1, 2, _Q4), (1, M32 - 1, -_Q4 & M32), (M32, M32, -_E8 & M32),
              (M32, 1, -_E8 & M32), (1, M32, -_E8 & M32), (M32, 1, _E8), (1, M32, _E8), (1, 0, 0))


# ---- an independent model of the levelisation and the fold rule ----------------------------------------------------
class Model:
    """Per wire of a Circuit: `level` (inputs 0, a bootstrap one above its deepest operand, a linear node at the level
    of the deepest stored wire its EXPANSION still names) and, for linear nodes, `exp` = ({stored wire: coefficient
    != 0}, constant).  Extended node by node, so the generator can ask while it builds."""

    def __init__(self, c):
        self.c = c
        self.level = [0] * c.n_inputs
        self.exp = [None] * c.n_inputs

    def expand(self, w):
        return self.exp[w] if self.exp[w] is not None else ({w: 1}, 0)

    @staticmethod
    def axpy(acc, s, e):
        t, k = acc
        for w, coef in e[0].items():
            v = (t.get(w, 0) + s * coef) & M32
            if v:
                t[w] = v
            else:
                t.pop(w, None)
        return t, (k + s * e[1]) & M32

    def comb(self, ca, a, cb, b, cc):
        """The expanded ca*a + cb*b + cc: ({wire: coef}, constant)."""
        acc = self.axpy(({}, 0), ca, self.expand(a))
        if cb:
            acc = self.axpy(acc, cb, self.expand(b))
        return acc[0], (acc[1] + cc) & M32

    def extend(self):
        c, lv = self.c, self.level
        for i in range(len(lv) - c.n_inputs, len(c._nodes)):
            node = c._nodes[i]
            kind, e = node[0], None
            if kind == "gate":
                L = 1 + max(lv[node[2]], 0 if node[1] == COPY else lv[node[3]])
            elif kind == "mux":
                L = 1 + max(lv[node[1]], lv[node[2]], lv[node[3]])
            elif kind in ("pbs", "pbs_many"):
                L = 1 + max(lv[node[2]], lv[node[4]] if node[3] else 0)
            elif kind == "pbs_fn":
                L = lv[node[1]]
            else:
                e = ({}, node[2])
                for coef, w in node[1]:
                    e = self.axpy(e, coef, self.expand(w))
                L = max((lv[w] for w in e[0]), default=0)
            lv.append(L)
            self.exp.append(e)
        return self


def is_linear(c, w):
    return w >= c.n_inputs and c._nodes[w - c.n_inputs][0] == "lin"


def operands(c, w):
    """The wires node `w` names (a many-LUT function names its head)."""
    if w < c.n_inputs:
        return []
    node = c._nodes[w - c.n_inputs]
    kind = node[0]
    if kind == "gate":
        return [node[2]] if node[1] == COPY else [node[2], node[3]]
    if kind == "mux":
        return list(node[1:4])
    if kind in ("pbs", "pbs_many"):
        return [node[2]] + ([node[4]] if node[3] else [])
    if kind == "pbs_fn":
        return [node[1]]
    return [x for _, x in node[1]]


def cone(c, wire):
    """`wire` and every wire that depends on it."""
    dep = {wire}
    for w in range(wire + 1, c.n_wires):
        if any(o in dep for o in operands(c, w)):
            dep.add(w)
    return dep


def n_bootstraps(c):
    """Bootstrap nodes: gates, muxes, pbs, many-LUT heads."""
    return sum(n[0] in ("gate", "mux", "pbs", "pbs_many") for n in c._nodes)


# ---- the generator ---------------------------------------------------------------------------------------------------
class _Builder:
    def __init__(self, seed, n_inputs, luts):
        import rs_tfhe_amd as R

        self.rng = np.random.default_rng(seed)
        self.c = R.Circuit(n_inputs)
        self.c.motifs = []       # (name, wire): what was built on purpose, counted by the corpus check
        self.c.seed = seed
        self.m = Model(self.c)
        self.no_pick = set()     # wires nothing may read (lin_output_only)
        self.luts = [self.c.lut(self.words((2, 1024))) for _ in range(luts)]

    def words(self, shape):
        return self.rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)

    # -- picking wires --
    def stored(self):
        self.m.extend()
        return [w for w in range(self.c.n_wires) if not is_linear(self.c, w)]

    def pick(self, pool=None):
        """Half from the last few wires (depth), half from anywhere (long-lived wires, fan-out)."""
        pool = [w for w in (pool if pool is not None else range(self.c.n_wires)) if w not in self.no_pick]
        recent = pool[-6:]
        return int(self.rng.choice(recent if self.rng.random() < 0.5 else pool))

    def distinct(self, k, pool=None):
        """k different stored wires, or None."""
        pool = [w for w in (pool if pool is not None else self.stored()) if w not in self.no_pick]
        if len(pool) < k:
            return None
        near = pool[-8:] if self.rng.random() < 0.5 and len(pool[-8:]) >= k else pool
        return [int(x) for x in self.rng.choice(near, k, replace=False)]

    def coef(self, pool=COEFS):
        return int(pool[self.rng.integers(0, len(pool))])

    def cconst(self):
        return 0 if self.rng.random() < 0.4 else int(self.rng.integers(0, 1 << 32))

    def lut(self):
        return int(self.rng.choice(self.luts))

    def lin3(self, ws=None):
        """A linear node over three different stored wires (a bootstrap cannot fold it), or None."""
        ws = ws or self.distinct(3)
        if ws is None:
            return None
        return self.c.lincomb([(self.coef(NONZERO), w) for w in ws], self.cconst())

    def wide(self, ca, cb, a, b):
        """ca*a + cb*b keeps more than two source wires (it could cancel down to a fold)."""
        self.m.extend()
        return len(self.m.comb(ca, a, cb, b, 0)[0]) > 2

    def mark(self, name, wire):
        self.c.motifs.append((name, int(wire)))
        return True

    # -- the random mix --
    def random_node(self):
        c, r = self.c, self.rng.random()
        if r < 0.35:
            c.gate(int(self.rng.integers(0, 11)), self.pick(), self.pick())
        elif r < 0.47:
            c.mux(self.pick(), self.pick(), self.pick())
        elif r < 0.59:
            c.pbs(self.coef(), self.pick(), self.coef(), self.pick(), self.cconst(), self.lut())
        elif r < 0.67:
            c.pbs_many(self.coef(), self.pick(), self.coef(), self.pick(), self.cconst(), self.lut(),
                       int(self.rng.choice([1, 2, 4, 8])))
        elif r < 0.75:
            c.not_(self.pick())
        elif r < 0.78:
            c.constant(bool(self.rng.integers(0, 2)))
        else:
            c.lincomb([(self.coef(), self.pick()) for _ in range(int(self.rng.integers(0, 5)))], self.cconst())

    # -- motifs: each returns False when the circuit has too few wires for it yet --
    def fold_to_gate_code(self):
        ws = self.distinct(2)
        return ws and self.mark("fold_to_gate_code", self.c.and_(self.c.not_(ws[0]), ws[1]))

    def fold_swapped(self):
        ws = self.distinct(2)
        if not ws:
            return False
        lo, hi = sorted(ws)
        return self.mark("fold_swapped", self.c.xor(self.c.lincomb([(1, hi), (2, lo)]), self.c.lincomb([])))

    def fold_own_launch(self):
        ws = self.distinct(2)
        return ws and self.mark("fold_own_launch", self.c.xor(self.c.not_(ws[0]), ws[1]))

    def fold_cancels(self):
        x = self.pick(self.stored())
        return self.mark("fold_cancels", self.c.nand(x, self.c.not_(x)))

    def same_wire_twice(self):
        x = self.pick(self.stored())
        return self.mark("same_wire_twice", self.c.xor(x, x))

    def copy(self):
        return self.mark("copy", self.c.gate(COPY, self.pick(self.stored()), self.pick(self.stored())))

    def constant_operand(self):
        x = self.pick(self.stored())
        k = self.c.constant(bool(self.rng.integers(0, 2)))
        return self.mark("constant_operand", self.c.or_(k, x) if self.rng.random() < 0.5 else self.c.and_(x, k))

    def materialise_for_gate(self):
        s = self.lin3()
        if s is None:
            return False
        op, y = int(self.rng.integers(0, 10)), self.pick(self.stored())
        g = self.c.gate(op, s, y)
        return self.wide(*GATE_COEFS[op][:2], s, y) and self.mark("materialise_for_gate", g)

    def materialise_for_mux(self):
        ws = self.distinct(3)
        if not ws:
            return False
        pos = int(self.rng.integers(0, 3))
        ops = [self.pick(self.stored()) for _ in range(3)]
        ops[pos] = self.c.not_(ws[0]) if self.rng.random() < 0.5 else self.lin3(ws)
        return self.mark("materialise_for_mux", self.c.mux(*ops))

    def materialise_for_pbs(self):
        s = self.lin3()
        if s is None:
            return False
        ca, cb, y = self.coef(NONZERO), self.coef(NONZERO), self.pick(self.stored())
        g = self.c.pbs(ca, s, cb, y, self.cconst(), self.lut())
        return self.wide(ca, cb, s, y) and self.mark("materialise_for_pbs", g)

    def materialised_twice(self):
        s = self.lin3()
        if s is None:
            return False
        y = self.pick(self.stored())
        g1 = self.c.nand(s, y)
        g2 = self.c.and_(s, g1)  # one level above g1: `need` keeps the earlier level
        return self.wide(M32, M32, s, y) and self.mark("materialised_twice", g2)

    def lin_of_lin(self):
        ws = self.distinct(3)
        if not ws:
            return False
        inner = self.c.lincomb([(1, ws[0]), (3, ws[1])], self.cconst())
        outer = self.c.lincomb([(2, inner), (1, self.c.not_(ws[2]))], self.cconst())
        return self.mark("lin_of_lin", self.c.or_(outer, ws[0]))

    def lin_output_only(self):
        ws = self.distinct(2)
        if not ws:
            return False
        s = self.c.lincomb([(self.coef(NONZERO), ws[0]), (self.coef(NONZERO), ws[1])], self.cconst())
        self.no_pick.add(s)
        return self.mark("lin_output_only", s)

    def pbs_two_lin_operands_fold(self):
        ws = self.distinct(2)
        if not ws:
            return False
        x, y = ws
        l1, l2 = self.c.lincomb([(1, x), (2, y)], self.cconst()), self.c.lincomb([(3, x), (M32, y)])
        return self.mark("pbs_two_lin_operands_fold", self.c.pbs(self.coef(NONZERO), l1, self.coef(NONZERO), l2, self.cconst(), self.lut()))

    def pbs_cb_zero_lin_operand(self):
        ws = self.distinct(2)
        if not ws:
            return False
        op = self.c.not_(ws[0]) if self.rng.random() < 0.5 else self.c.lincomb([(2, ws[0]), (M32, ws[1])], self.cconst())
        return self.mark("pbs_cb_zero_lin_operand", self.c.pbs(self.coef(NONZERO), op, 0, op, self.cconst(), self.lut()))

    def same_level(self, k):
        """k different stored wires of one level (the deepest level that has k, or a random one)."""
        by = {}
        for w in self.stored():
            if w not in self.no_pick:
                by.setdefault(self.m.level[w], []).append(w)
        ok = sorted(L for L, ws in by.items() if len(ws) >= k)
        if not ok:
            return None
        L = ok[-1] if self.rng.random() < 0.5 else int(self.rng.choice(ok))
        return [int(x) for x in self.rng.choice(by[L], k, replace=False)]

    def many_group_of_several(self):
        q = int(self.rng.integers(2, 4))
        ws = self.same_level(q + 1)
        if not ws:
            return False
        ws = sorted(ws, reverse=self.rng.random() < 0.5)  # the shared operand first or last of all: one coefficient order
        k, ca, cb, cc, lut = int(self.rng.choice([2, 4, 8])), self.coef(NONZERO), self.coef(NONZERO), self.cconst(), self.lut()
        outs = [self.c.pbs_many(ca, ws[i], cb, ws[q], cc, lut, k) for i in range(q)]  # equal keys, one level
        last = None
        for fns in outs:  # a later node reads function j > 0 of each
            j = int(self.rng.integers(1, k))
            last = self.c.gate(int(self.rng.integers(0, 10)), fns[j], fns[0] if last is None else last)
        return self.mark("many_group_of_several", outs[0][0])

    def two_lut_groups_one_level(self):
        ws = self.distinct(2)
        if not ws:
            return False
        x, y = ws
        a = self.c.pbs(1, x, 1, y, 0, self.luts[0])
        self.c.pbs(1, x, 2, y, 5, self.luts[-1])
        self.c.pbs(1, x, 1, y, 0, self.luts[0])  # joins the first group
        return self.mark("two_lut_groups_one_level", a)

    def zero_coefficient_term(self):
        st = self.stored()
        deep = max(st, key=lambda w: (self.m.level[w], w))
        if self.m.level[deep] == 0:
            return False
        x, y = int(self.rng.integers(0, self.c.n_inputs)), int(self.rng.integers(0, self.c.n_inputs))
        terms = [(0, deep), (1, x)] if self.rng.random() < 0.5 else [(1 << 31, deep), (1, x), (1 << 31, deep)]
        return self.mark("zero_coefficient_term", self.c.and_(self.c.lincomb(terms), y))  # native level 1

    def mux_chain(self):
        x, y, z = (self.pick(self.stored()) for _ in range(3))
        m1 = self.c.mux(x, y, z)
        m2 = self.c.mux(m1, z, y)
        return self.mark("mux_chain", self.c.mux(y, m2, m1))


def random_circuit(seed, n_inputs, n_nodes, *, luts=3):
    """A circuit of at least `n_nodes` nodes over `n_inputs` inputs, deterministic in `seed`: the random mix of every
    node kind, interleaved with a seeded selection of MOTIFS (a motif adds a few nodes, so the count can overshoot).
    `luts` random [2][1024] tables are registered.  `c.motifs` lists (name, wire) of what was built on purpose."""
    b = _Builder(seed, n_inputs, luts)
    chosen = [MOTIFS[i] for i in b.rng.permutation(len(MOTIFS))]  # this circuit's order: it gets as far as its size allows
    at = 0
    while b.c.n_wires - n_inputs < n_nodes:
        if b.rng.random() < 0.4:
            name = chosen[at % len(chosen)]
            at += 1
            if getattr(b, name)():
                continue
        b.random_node()
    return b.c


# ---- the schedule against the model ----------------------------------------------------------------------------------
def wire_level(d, slot):
    """The level whose slot range holds `slot`."""
    return bisect.bisect_right([lv["begin"] for lv in d], slot) - 1


def check_schedule(c, many_layout="function_major"):
    """Asserts the structural invariants of the native schedule of `c` (describe / slots / wire_slot / operand_slots)
    against the node list and the Model.  `many_layout`: the many-LUT slot layout to expect ("node_major" is wrong on
    purpose: the tests use it to show that this check can fail).  Returns {wire: native level} of the stored wires."""
    d = c.describe()
    m = Model(c).extend()
    n_in = c.n_inputs
    assert d[0]["begin"] == 0 and d[0]["end"] == n_in
    for prev, lv in zip(d, d[1:]):
        assert lv["begin"] == prev["end"] and lv["end"] >= lv["begin"], (c.seed, lv)
    assert c.slots == d[-1]["end"] == n_in + sum(lv["end"] - lv["begin"] for lv in d[1:])
    slot = [c.wire_slot(w) for w in range(c.n_wires)]
    level, seen = {}, set()
    for w in range(c.n_wires):
        if is_linear(c, w):
            assert slot[w] == NO_SLOT, (c.seed, w)
            continue
        assert slot[w] < c.slots and slot[w] not in seen, (c.seed, w, slot[w])
        seen.add(slot[w])
        level[w] = L = wire_level(d, slot[w])
        assert L == m.level[w], (c.seed, w, L, m.level[w])     # the level the model derives
        assert L <= c._level[w], (c.seed, w, L, c._level[w])   # Python's may be higher (zero / cancelling terms), never lower
    # level sizes from the node list
    for L, lv in enumerate(d):
        if L == 0:
            continue
        mine = [w for w in level if level[w] == L and w >= n_in]
        kinds = [c._nodes[w - n_in] for w in mine]
        muxes = sum(n[0] == "mux" for n in kinds)
        heads = [n for n in kinds if n[0] == "pbs_many"]
        boots = sum(n[0] in ("gate", "mux", "pbs", "pbs_many") for n in kinds)
        assert lv["nks_nodes"] == 2 * muxes and lv["nks_launches"] == (1 if muxes else 0), (c.seed, L)
        assert lv["gate_nodes"] + lv["lut_nodes"] == boots, (c.seed, L, lv, boots)
        single = lv["lut_nodes"] - len(heads)  # describe() counts a many-LUT node once
        assert single >= 0
        size = lv["lincomb_nodes"] + lv["nks_nodes"] + lv["gate_nodes"] + single + sum(n[7] for n in heads)
        assert lv["end"] - lv["begin"] == size, (c.seed, L, lv, size)
        for k in ("lincomb", "gate"):
            assert lv[k + "_launches"] == (1 if lv[k + "_nodes"] else 0)
        # many-LUT groups: heads of one level with equal (lut, folded coefficients, k), in wire order
        groups = {}
        for w in mine:
            n = c._nodes[w - n_in]
            if n[0] == "pbs_many":
                groups.setdefault(_lut_key(m, n), []).append(w)
        for key, hs in groups.items():
            base, nodes, k = slot[hs[0]], len(hs), key[-1]
            for q, h in enumerate(hs):
                for j in range(k):
                    want = base + j * nodes + q if many_layout == "function_major" else base + q * k + j
                    assert slot[h + j] == want, (c.seed, "many-LUT layout", h, j, slot[h + j], want)
    # operands: written before the launch that reads them
    mat_rows = _mat_rows(d)
    for w, L in level.items():
        if w < n_in:
            continue
        n, ops = c._nodes[w - n_in], c.operand_slots(w)
        begin = d[L]["begin"]
        mat = range(begin, begin + d[L]["lincomb_nodes"])  # this level's lincomb launch runs first

        def row_ok(o, wire):
            """`o` is the row a bootstrap reads for operand `wire`: its slot, its plain alias', or a materialised row."""
            alias = _plain(m, wire)
            if alias is not None:
                return o == slot[alias]
            return o not in seen and o in mat_rows and o < begin + d[L]["lincomb_nodes"]

        assert all(o < begin or o in mat for o in ops), (c.seed, w, ops, begin)
        if n[0] == "mux":
            assert len(ops) == 3 and all(row_ok(o, x) for o, x in zip(ops, n[1:4])), (c.seed, w, ops)
            continue
        if n[0] == "pbs_fn":
            assert ops == c.operand_slots(n[1])
            continue
        gate = n[0] == "gate"
        ca, cb, cc = GATE_COEFS[n[1]] if gate else (n[1], n[3], n[5])
        a, b = n[2], (n[3] if gate else n[4])
        if not cb:
            b = a
        pa, pb = _plain(m, a), _plain(m, b)
        if gate and pa is not None and pb is not None:
            assert ops == [slot[pa], slot[pb]], (c.seed, w, ops)  # plain operands (or plain aliases): as named
            continue
        t, k = m.comb(ca, a, cb, b, cc)
        if len(t) <= 2:  # folded into the prologue: the source wires of the combination (slot 0 when it has none)
            src = [slot[x] for x in sorted(t)] or [0]
            if gate and len(ops) == 2 and len(src) == 1:
                src = src * 2
            assert sorted(ops) == sorted(src), (c.seed, w, ops, src)
            if not gate:
                assert ops == src, (c.seed, w, ops, src)  # lut launches: in wire order, coefficients alongside
        else:
            assert len(ops) == (2 if gate or cb else 1) and row_ok(ops[0], a) and (len(ops) == 1 or row_ok(ops[1], b)), (c.seed, w, ops)
    check_motifs(c, d, slot)
    return level


def _plain(m, w):
    """The stored wire that `w` is (itself, or the one a linear node 1 * x + 0 aliases), else None."""
    t, k = m.expand(w)
    return next(iter(t)) if k == 0 and list(t.values()) == [1] else None


def _mat_rows(d):
    """The slots the lincomb launches write (first in their level's range)."""
    return {o for lv in d[1:] for o in range(lv["begin"], lv["begin"] + lv["lincomb_nodes"])}


def _lut_key(m, n):
    """(lut, ca, cb, cc, k) of a pbs / pbs_many node as its launch carries them: the folded combination's when it has
    at most two source wires (terms in wire order), its own otherwise."""
    t, k = m.comb(n[1], n[2], n[3], n[4], n[5])
    nl = n[7] if n[0] == "pbs_many" else 0
    if len(t) <= 2:
        cs = [t[x] for x in sorted(t)] + [0, 0]
        return (n[6], cs[0], cs[1], k, nl)
    return (n[6], n[1], n[3], n[5], nl)


def check_motifs(c, d, slot):
    """What each motif is there to force, where the schedule shows it."""
    n_in = c.n_inputs
    mat_rows = _mat_rows(d)
    for name, w in c.motifs:
        if name == "lin_output_only":
            assert slot[w] == NO_SLOT
            continue
        n = c._nodes[w - n_in]
        ops = c.operand_slots(w)
        lv = d[wire_level(d, slot[w])]
        if name == "fold_to_gate_code":  # and(not(x), y) == and_ny(x, y): the gate launch reads x and y
            x = c._nodes[n[2] - n_in][1][0][1]
            assert ops == [slot[x], slot[n[3]]] and lv["gate_nodes"] >= 1, (c.seed, name, ops)
        elif name == "fold_swapped":     # hi + 2 lo + 1/4 == xor(hi, lo): matched with the two wires exchanged
            (_, hi), (_, lo) = c._nodes[n[2] - n_in][1]
            assert lo < hi and ops == [slot[hi], slot[lo]], (c.seed, name, ops)
        elif name == "fold_own_launch":
            assert lv["lut_launches"] >= 1 and len(ops) == 2
        elif name == "fold_cancels":
            assert ops == [0] and lv["lut_launches"] >= 1, (c.seed, name, ops)
        elif name == "same_wire_twice":
            assert ops == [slot[n[2]]] * 2
        elif name == "copy":
            assert ops == [slot[n[2]]] * 2
        elif name in ("materialise_for_gate", "materialise_for_pbs", "materialise_for_mux"):
            assert any(o in mat_rows for o in ops), (c.seed, name, ops)
        elif name == "materialised_twice":  # read again one level up: the row of the earlier level
            first = c.operand_slots(n[3])
            assert ops[0] == first[0] and first[0] < lv["begin"] and first[0] in mat_rows, (c.seed, name, ops, first)
        elif name == "zero_coefficient_term":
            assert wire_level(d, slot[w]) == 1 < c._level[w], (c.seed, name)
        elif name == "many_group_of_several":
            assert lv["lut_nodes"] >= 2


def widest_bootstrap_launch(c):
    """Node count of the widest bootstrap launch that describe() shows exactly: nks and gate launches, and a level's
    lut launch where it has only one."""
    w = 0
    for lv in c.describe():
        w = max(w, lv["nks_nodes"], lv["gate_nodes"], lv["lut_nodes"] if lv["lut_launches"] == 1 else 0)
    return w


# ---- reference -------------------------------------------------------------------------------------------------------
def reference(c, O, ck, inputs):
    """Every wire of `c` on the CPU oracle, node by node: [n_wires][B][n+1]."""
    from test_gpu_many_lut import many_model

    def gate(op, a, b):
        if op == COPY:  # not an oracle gate: the bootstrap of a itself
            return O.batch_bootstrap(ck, a)
        return O.batch_gate(ck, op, a, b)

    return c.run_reference(gate, inputs, mux_fn=lambda a, b, cc: O.batch_mux(ck, a, b, cc, naive=False),
                           pbs_fn=lambda tv, x: O.batch_bootstrap(ck, x, testvec=tv),
                           many_fn=lambda tv, prep, k: many_model(O, ck, prep, tv, k))


# ---- perturbations (the comparison can see) ----------------------------------------------------------------------------
def perturbation_sites(c):
    """{kind: wire} of the first node of each kind that one wrong operand can be planted in."""
    n_in, out = c.n_inputs, {}
    for i, n in enumerate(c._nodes):
        w = n_in + i
        if n[0] == "gate" and n[1] == ANDNY and n[2] != n[3]:
            out.setdefault("and_ny_swapped", w)
        if n[0] == "pbs" and n[3] and n[1] != n[3] and n[2] != n[4]:
            out.setdefault("pbs_ca_cb_exchanged", w)
        if n[0] == "gate" and n[2] >= n_in:
            src = c._nodes[n[2] - n_in]
            head = n[2] if src[0] == "pbs_many" else src[1] if src[0] == "pbs_fn" else None
            if head is not None and c._nodes[head - n_in][7] >= 2:
                out.setdefault("many_function_index", w)
    return out


def perturbed(c, kind, wire):
    """A copy of `c` (reference evaluation only) with the one node `wire` changed as `kind` says."""
    import rs_tfhe_amd as R

    p = R.Circuit(c.n_inputs)
    p._nodes, p._luts, p._n_wires = list(c._nodes), list(c._luts), c._n_wires
    n_in = c.n_inputs
    n = c._nodes[wire - n_in]
    if kind == "and_ny_swapped":
        n = (n[0], n[1], n[3], n[2])
    elif kind == "pbs_ca_cb_exchanged":
        n = (n[0], n[3], n[2], n[1]) + tuple(n[4:])
    else:  # function j <-> j + 1 of the many-LUT node the gate reads (the last function: j - 1)
        src = c._nodes[n[2] - n_in]
        head, j = (n[2], 0) if src[0] == "pbs_many" else (src[1], src[2])
        k = c._nodes[head - n_in][7]
        n = (n[0], n[1], head + (j + 1 if j + 1 < k else j - 1), n[3])
    p._nodes[wire - n_in] = n
    return p


# ---- the corpus the GPU test runs (and the host test holds to the corpus condition) ----------------------------------
SHAPES = ((64, 2, 8, 2, 5), (96, 3, 6, 2, 8), (80, 1, 10, 5, 3))  # (n, l, bgbit, basebit, t): the exact-product regime
CORPUS = {  # shape -> [(seed, n_inputs, n_nodes)]
    SHAPES[0]: [(s, 3 + s % 4, 64 + 3 * (s % 5)) for s in range(100, 112)],
    SHAPES[1]: [(s, 3 + s % 4, 64 + 3 * (s % 5)) for s in range(200, 212)],
    SHAPES[2]: [(s, 3 + s % 4, 64 + 3 * (s % 5)) for s in range(300, 312)],
    "SECURITY_80_BIT": [(400, 4, 56), (401, 5, 56)],
}


# what the pool case needs of a circuit, by motif: a folded gate on the key's own test vector, a materialised lincomb, a
# mux with a linear operand, a many-LUT group of several nodes
POOL_NEEDS = (("fold_own_launch", "fold_cancels"), ("materialise_for_gate", "materialise_for_pbs"), ("materialise_for_mux",),
              ("many_group_of_several",))


def pool_circuits(cs):
    return [c for c in cs if all(any(n in alt for n, _ in c.motifs) for alt in POOL_NEEDS)]


def corpus(key):
    return [random_circuit(*spec) for spec in CORPUS[key]]
