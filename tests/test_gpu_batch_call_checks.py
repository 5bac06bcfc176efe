"""Characterisation of the argument checks of the nine batch operations of the C ABI (include/tfhe_hip.h), on each of
their four forms: context / host pointers (`tfhe_hip_batch_X`), context / device pointers (`tfhe_hip_batch_X_dev`),
pool / host pointers (`tfhe_hip_pool_batch_X`) and pool / device pointers on a home member (`tfhe_hip_pool_batch_X_dev`).

What is pinned is which check fires first, with which return code and which error text -- including the places where
the forms differ (an unknown gate at count 0 is TFHE_HIP_OK through the host forms and TFHE_HIP_EINVAL through the
device forms; a pool prefixes "device N: " to what a member found and not to what it found itself; the many-LUT pool
call looks at `home` before anything else, the other pool calls after their pointers).  TABLE below is written out by
hand from the checks in rs-tfhe_amd/csrc/tfhe_hip.hip and pool.hpp; nothing in it is computed by calling the library.

Only calls that are turned away BEFORE anything is launched appear here, plus count = 0 calls, which launch nothing.
Every pointer that is not the NULL under test is a real buffer of the full size the call would need.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 1024
OK, EINVAL, ENOKEY = 0, -1, -3
BIG = 4097  # above the largest bound the combining front end accepts (4096) and above a pool member's 256
NP = "null pointer"
D0 = "device 0: "
NOKEY = "cloud key not loaded"
HOME = "no such pool member (home)"
NLUTS = "n_luts must be 1, 2, 4 or 8"
NOTV = "many-LUT bootstrap needs a test vector"
GATE = "unknown gate"

ALL = ("ctx", "ctx_dev", "pool", "pool_dev")
MIXED = ("gates_mixed", "gates_mixed_nks")
KEYED = ("gate",) + MIXED + ("bootstrap", "lincomb_bootstrap", "lincomb_bootstrap_many", "mux", "blind_rotate")
EVERY = KEYED + ("tlwe_lincomb",)

# (operations, forms, cases, counts, return code, error text).  A case is `+`-joined: null:<operand>, gate:<code> (the
# scalar gate), code:<code> (the last entry of the per-ciphertext gate array), n_luts:<k>, no_testvec (many-LUT),
# home:<member> (pool device forms) and nokey (the handle without a cloud key).
TABLE = [
    # ---- gate (NAND: both operands are read) ----
    (("gate",), ("ctx",), ("null:a", "null:b", "null:out"), (1, BIG), EINVAL, NP),
    (("gate",), ("ctx",), ("gate:99", "gate:-1"), (1, BIG), EINVAL, GATE),
    (("gate",), ("ctx", "pool"), ("null:a", "null:b", "null:out", "gate:99"), (0,), OK, None),
    (("gate",), ("ctx_dev",), ("null:a", "null:out", "null:a+gate:99"), (1, BIG), EINVAL, NP),
    (("gate",), ("ctx_dev",), ("null:b",), (1, BIG), EINVAL, "second gate operand is NULL"),
    (("gate",), ("ctx_dev", "pool_dev"), ("gate:99", "gate:-1"), (0, 1, BIG), EINVAL, GATE),
    (("gate",), ("ctx_dev", "pool_dev"), ("null:a", "null:b", "null:out"), (0,), OK, None),
    (("gate",), ("pool",), ("null:a", "null:out", "null:a+gate:99"), (1, BIG), EINVAL, NP),
    (("gate",), ("pool",), ("null:b",), (1, BIG), EINVAL, D0 + NP),
    (("gate",), ("pool",), ("gate:99",), (1, BIG), EINVAL, D0 + GATE),
    (("gate",), ("pool_dev",), ("null:a", "null:b", "null:out", "null:a+home:1"), (1, BIG), EINVAL, NP),
    (("gate",), ("pool_dev",), ("gate:99+null:a", "gate:99+home:1"), (1,), EINVAL, GATE),
    # ---- per-ciphertext gates, with and without the key switch ----
    (MIXED, ALL, ("null:gates", "null:a", "null:b", "null:out"), (1, BIG), EINVAL, NP),
    (MIXED, ALL, ("null:gates", "null:a", "null:b", "null:out"), (0,), OK, None),
    (MIXED, ("ctx",), ("code:11", "code:255"), (1, BIG), EINVAL, GATE),
    (MIXED, ("pool",), ("code:11", "code:255"), (1, BIG), EINVAL, D0 + GATE),
    (MIXED, ("ctx", "pool"), ("null:a+code:11",), (1, BIG), EINVAL, NP),
    (MIXED, ("pool_dev",), ("null:a+home:1",), (1,), EINVAL, NP),
    # ---- bootstrap / blind_rotate (a NULL test vector is the key's own: legal) ----
    (("bootstrap", "blind_rotate"), ALL, ("null:in", "null:out"), (1, BIG), EINVAL, NP),
    (("bootstrap", "blind_rotate"), ALL, ("null:in", "null:out"), (0,), OK, None),
    (("bootstrap", "blind_rotate"), ("pool_dev",), ("null:in+home:1",), (1,), EINVAL, NP),
    # ---- tlwe_lincomb / lincomb_bootstrap (cb = 1: b is read) ----
    (("tlwe_lincomb", "lincomb_bootstrap"), ALL, ("null:a", "null:b", "null:out"), (1, BIG), EINVAL, NP),
    (("tlwe_lincomb", "lincomb_bootstrap"), ALL, ("null:a", "null:b", "null:out"), (0,), OK, None),
    (("tlwe_lincomb", "lincomb_bootstrap"), ("pool_dev",), ("null:b+home:1",), (1,), EINVAL, NP),
    # ---- many-LUT: n_luts, the test vector and b (cb = 1) are checked whatever the count ----
    (("lincomb_bootstrap_many",), ALL, ("n_luts:0", "n_luts:3", "n_luts:16", "n_luts:3+no_testvec", "n_luts:3+null:b"),
     (0, 1, BIG), EINVAL, NLUTS),
    (("lincomb_bootstrap_many",), ALL, ("no_testvec", "no_testvec+null:b", "no_testvec+null:a"), (0, 1, BIG), EINVAL, NOTV),
    (("lincomb_bootstrap_many",), ALL, ("null:b", "null:b+null:a"), (0, 1, BIG), EINVAL, NP),
    (("lincomb_bootstrap_many",), ALL, ("null:a", "null:out"), (1, BIG), EINVAL, NP),
    (("lincomb_bootstrap_many",), ALL, ("null:a", "null:out"), (0,), OK, None),
    (("lincomb_bootstrap_many",), ("pool_dev",), ("home:1+n_luts:3", "home:-1+no_testvec", "home:1+null:b", "home:1+null:a"),
     (0, 1, BIG), EINVAL, HOME),
    (("lincomb_bootstrap_many",), ("ctx", "ctx_dev"), ("nokey+n_luts:3", "nokey+no_testvec", "nokey+null:b"), (0, 1), ENOKEY, NOKEY),
    (("lincomb_bootstrap_many",), ("pool", "pool_dev"), ("nokey+n_luts:3",), (0, 1), EINVAL, NLUTS),
    # ---- mux ----
    (("mux",), ALL, ("null:a", "null:b", "null:c", "null:out"), (1, BIG), EINVAL, NP),
    (("mux",), ALL, ("null:a", "null:b", "null:c", "null:out"), (0,), OK, None),
    (("mux",), ("pool_dev",), ("null:c+home:1",), (1,), EINVAL, NP),
    # ---- no such home member: found after the pointers (many-LUT above: before them), at any count ----
    (EVERY, ("pool_dev",), ("home:-1", "home:1"), (0, 1, BIG), EINVAL, HOME),
    # ---- no cloud key: a context looks first and at any count; a pool leaves it to the member that runs a shard ----
    (KEYED, ("ctx", "ctx_dev"), ("nokey",), (0, 1, BIG), ENOKEY, NOKEY),
    (KEYED, ("pool", "pool_dev"), ("nokey",), (1, BIG), ENOKEY, D0 + NOKEY),
    (KEYED, ("pool", "pool_dev"), ("nokey",), (0,), OK, None),
    (("gate",) + MIXED + ("mux",), ("ctx", "ctx_dev"), ("nokey+null:a",), (BIG,), ENOKEY, NOKEY),
    (("gate",) + MIXED + ("mux",), ("pool", "pool_dev"), ("nokey+null:a",), (1, BIG), EINVAL, NP),
]

OPERANDS = {
    "gate": ("a", "b", "out"), "gates_mixed": ("gates", "a", "b", "out"), "gates_mixed_nks": ("gates", "a", "b", "out"),
    "bootstrap": ("in", "out"), "tlwe_lincomb": ("a", "b", "out"), "lincomb_bootstrap": ("a", "b", "out"),
    "lincomb_bootstrap_many": ("a", "b", "testvec", "out"), "mux": ("a", "b", "c", "out"), "blind_rotate": ("in", "out"),
}


class _Buffers:
    """One real buffer per operand name, host and device, each large enough for BIG rows of the largest shape."""

    def __init__(self, n):
        import torch

        rows = {"a": n + 1, "b": n + 1, "c": n + 1, "in": n + 1, "out": 2 * N, "testvec": 0, "gates": 0}
        self.host, self.dev = {}, {}
        for name, w in rows.items():
            words = BIG * w if w else (2 * N if name == "testvec" else (BIG + 3) // 4)
            self.host[name] = np.zeros(words, np.uint32)
            self.dev[name] = torch.zeros(words, dtype=torch.int32, device="cuda:0")

    def ptr(self, name, dev):
        return self.dev[name].data_ptr() if dev else self.host[name].ctypes.data


def _run(lib, handles, buf, op, form, case, count):
    """Make the call `case` describes; returns (return code, error text)."""
    dev, pool = form.endswith("_dev"), form.startswith("pool")
    p = {name: buf.ptr(name, dev) for name in OPERANDS[op]}
    gate, n_luts, home, keyed = 0, 2, 0, True  # NAND
    if "gates" in p:
        buf.host["gates"].view(np.uint8)[:] = 0
    for tok in case.split("+"):
        kind, _, val = tok.partition(":")
        if kind == "null":
            assert val in p, (op, tok)
            p[val] = None
        elif kind == "gate":
            gate = int(val)
        elif kind == "code":
            assert not dev and count > 0  # (a bad code in a DEVICE array is found by the kernel: not a check)
            buf.host["gates"].view(np.uint8)[count - 1] = int(val)
        elif kind == "n_luts":
            n_luts = int(val)
        elif kind == "no_testvec":
            p["testvec"] = None
        elif kind == "home":
            assert form == "pool_dev"
            home = int(val)
        elif kind == "nokey":
            keyed = False
        else:
            raise AssertionError(tok)
    h = handles[("pool" if pool else "ctx", keyed)]
    lin = (1, p.get("a"), 1, p.get("b"), 0x20000000)
    args = {
        "gate": (gate, p.get("a"), p.get("b"), p["out"]),
        "gates_mixed": (p.get("gates"), p.get("a"), p.get("b"), p["out"]),
        "gates_mixed_nks": (p.get("gates"), p.get("a"), p.get("b"), p["out"]),
        "bootstrap": (p.get("in"), None, 0, 1, p["out"]),
        "tlwe_lincomb": lin + (p["out"],),
        "lincomb_bootstrap": lin + (None, 0, 1, p["out"]),
        "lincomb_bootstrap_many": lin + (p.get("testvec"), 0, n_luts, 1, p["out"]),
        "mux": (0, p.get("a"), p.get("b"), p.get("c"), p["out"]),
        "blind_rotate": (p.get("in"), None, p["out"]),
    }[op]
    fn = getattr(lib, ("tfhe_hip_pool_batch_" if pool else "tfhe_hip_batch_") + op + ("_dev" if dev else ""))
    rc = fn(h, *((home,) if pool and dev else ()), *args, count, *((None,) if dev else ()))
    text = (lib.tfhe_hip_pool_last_error if pool else lib.tfhe_hip_last_error)(h)
    return rc, text.decode() if text else ""


def test_table_covers_every_operation_and_form():
    seen = {(op, form) for ops, forms, _, _, _, _ in TABLE for op in ops for form in forms}
    assert seen == {(op, form) for op in OPERANDS for form in ALL}


def test_batch_call_checks(golden):
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import SecurityParams

    n, l, bgbit, basebit, t = (int(v) for v in golden["toy"]["params"])
    P = SecurityParams("TOY_CHECKS", 0, n, l, bgbit, basebit, t, 2.0e-5, 2.0e-8)
    rng = np.random.default_rng(20)
    k0, k1 = rng.integers(0, 2, n).astype(np.uint32), rng.integers(0, 2, N).astype(np.uint32)
    eng, bare, pool, bare_pool = R.Engine(P, 0), R.Engine(P, 0), R.Pool(P, [0]), R.Pool(P, [0])
    eng.gen_cloud_key(k0, k1, seed=20)
    pool.gen_cloud_key(k0, k1, seed=20)
    handles = {("ctx", True): eng._ctx, ("ctx", False): bare._ctx, ("pool", True): pool._h, ("pool", False): bare_pool._h}
    lib, buf = eng._lib, _Buffers(n)
    wrong, cases = [], 0
    for ops, forms, tags, counts, rc, text in TABLE:
        for op in ops:
            for form in forms:
                for case in tags:
                    for count in counts:
                        got = _run(lib, handles, buf, op, form, case, count)
                        cases += 1
                        print(f"{op:24s} {form:8s} {case:24s} count={count:<5d} -> {got}")
                        if got[0] != rc or (text is not None and got[1] != text):
                            wrong.append((op, form, case, count, "want", (rc, text), "got", got))
    eng.synchronize()
    pool.synchronize()
    torch.cuda.synchronize()
    for h in (pool, bare_pool, eng, bare):
        h.close()
    assert not wrong, wrong
    assert cases >= 700
