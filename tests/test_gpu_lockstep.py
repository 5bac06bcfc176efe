"""The fused blind-rotation kernels (k_blind_rotate, k_blind_rotate_wide2, k_blind_rotate_pair) held to the exact integer
product STEP BY STEP (tests/lockstep.py; the harness itself is proven on the CPU in tests/test_lockstep_host.py): on every
reference parameter set through every forced kernel, through the default dispatch, in the LWE output forms, on two
custom shapes that run the general-rounding l = 2 / l = 3 instantiations, and on crafted keys whose pre-rounding values
reach 2^62.  The bar is the project's existing one: the device's error against the exact product is at
most twice the CPU f64 path's on the same step; where the product is exact, 0 LSB and the CPU path's words."""
import math
import os

import numpy as np
import pytest

import lockstep as LS
from conftest import oracle_keys, signed_diff
from test_gpu_parity import INEXACT_SETS, _cloud_key

pytestmark = pytest.mark.gpu
N = 1024
EXACT_SETS = ["SECURITY_128_BIT", "SECURITY_110_BIT", "SECURITY_80_BIT", "SECURITY_UINT1"]
KERNELS = list(LS.BR_KERNEL_ENVS)


def _record(line):
    """the measured figures, one line each, for DESIGN section 7: printed (pytest -s shows them), and appended to
    $TFHE_TEST_RECORD_DIR/lockstep_ratios.txt where that directory is given"""
    print(line)
    d = os.environ.get("TFHE_TEST_RECORD_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "lockstep_ratios.txt"), "a") as f:
            f.write(line + "\n")


def _set_keys(O, setname):
    # (the inexact sets: the key test_external_product_error_relative_to_the_cpu_path generates, shared through the cache)
    return oracle_keys(O, getattr(O, setname), seed=88, with_time=True) if setname in INEXACT_SETS else oracle_keys(
        O, getattr(O, setname), with_time=True)


def _chain_inputs(n, seed):
    pos = LS.mask_positions(n)
    ct = LS.make_ciphertext(n, pos, seed)
    tv = np.random.default_rng(seed + 1).integers(0, 2**32, (2, N), dtype=np.uint64).astype(np.uint32)
    return pos, ct, tv


def _forced_engine(monkeypatch, pk, name, count):
    import rs_tfhe_amd as R

    LS.with_br_kernel(monkeypatch, name)
    eng = R.Engine(pk.params, 0)
    eng.load_cloud_key(pk)
    assert f"blind_rotate={name}[0,{count})" in eng.describe_dispatch(count)
    return eng


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("setname", INEXACT_SETS + EXACT_SETS)
def test_lockstep_every_set_every_kernel(O, monkeypatch, setname, kernel):
    """One batch_blind_rotate call with the K + 1 prefix rows and a random test vector per (set, forced kernel), then
    check_chain: row 0 is the rotated test vector, every step within 2 x the CPU path's error of the exact product (0 LSB
    and the CPU path's words at bgbit <= 10); rotation amounts 1, N - 1, N, N + 1, 2N - 1 among the steps; key rows 0 and
    n - 1, eight consecutive rows in the middle."""
    sk, ck = _set_keys(O, setname)
    P = ck.params
    pos, ct, tv = _chain_inputs(P.n, 900)
    rows = LS.prefix_rows(ct, pos)
    eng = _forced_engine(monkeypatch, _cloud_key(ck), kernel, len(rows))
    assert eng.rounding_mode == ("fast" if P.bgbit == 6 else "general")
    states = eng.batch_blind_rotate(rows, tv)
    eng.close()
    pairs = LS.check_chain(O, ck, states, ct, pos, tv, LS.is_exact_regime(P), label=f"{setname} {kernel}")
    _record(f"lockstep {setname} {kernel}: worst e_dev/e_cpu {LS.worst_ratio(pairs):.3f} max e_dev {max(p[0] for p in pairs)} max e_cpu {max(p[1] for p in pairs)}")


@pytest.mark.parametrize("setname,count", [("SECURITY_UINT4", 1100), ("SECURITY_UINT3", 300)])
def test_lockstep_through_the_default_dispatch_and_the_lwe_forms(O, monkeypatch, setname, count):
    """The same chain with its rows scattered among random rows of ONE batch of the default dispatch -- 1,100 (the batch
    kernel and a latency-kernel tail; rows on both sides of the cut) and 300 (the pair kernel): the chain holds, the bits
    are those of the three forced kernels, and batch_bootstrap(keyswitch=False) returns sample_extract_index_2 of the
    checked accumulators word for word."""
    import rs_tfhe_amd as R

    sk, ck = _set_keys(O, setname)
    P = ck.params
    pk = _cloud_key(ck)
    pos, ct, tv = _chain_inputs(P.n, 900)
    rows = LS.prefix_rows(ct, pos)
    forced = {}
    for kernel in KERNELS:
        eng = _forced_engine(monkeypatch, pk, kernel, len(rows))
        forced[kernel] = eng.batch_blind_rotate(rows, tv)
        lwe = eng.batch_bootstrap(rows, tv, keyswitch=False)
        eng.close()
        assert np.array_equal(lwe, np.stack([O.sample_extract_index_2(s, 0, P.n) for s in forced[kernel]])), (setname, kernel)
    for kernel in KERNELS[1:]:
        assert np.array_equal(forced[kernel], forced[KERNELS[0]]), (setname, kernel)
    monkeypatch.delenv("TFHE_HIP_BR_KERNEL", raising=False)
    eng = R.Engine(pk.params, 0)
    eng.load_cloud_key(pk)
    plan = eng.describe_dispatch(count).split()[0]
    rng = np.random.default_rng(901)
    if count == 1100:
        assert plan.startswith("blind_rotate=batch[0,") and "+" in plan, plan
        cut = int(plan.split("[0,")[1].split(")")[0])
        where = np.sort(np.concatenate([rng.choice(cut, 8, replace=False), cut + rng.choice(count - cut, len(rows) - 8, replace=False)]))
    else:
        assert plan == f"blind_rotate=pair[0,{count})", plan
        where = np.sort(rng.choice(count, len(rows), replace=False))
    big = rng.integers(0, 2**32, (count, P.n + 1), dtype=np.uint64).astype(np.uint32)
    big[where] = rows
    states = eng.batch_blind_rotate(big, tv)[where]
    lwe = eng.batch_bootstrap(big, tv, keyswitch=False)[where]
    eng.close()
    pairs = LS.check_chain(O, ck, states, ct, pos, tv, False, label=f"{setname} default dispatch of {count}")
    assert np.array_equal(states, forced["batch"]), (setname, plan)
    assert np.array_equal(lwe, np.stack([O.sample_extract_index_2(s, 0, P.n) for s in states]))
    _record(f"lockstep {setname} default[{count}] {plan}: worst e_dev/e_cpu {LS.worst_ratio(pairs):.3f}")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shape", [(48, 2, 16, 61), (48, 3, 10, 62)], ids=lambda s: f"n{s[0]}_l{s[1]}_bg{s[2]}")
def test_lockstep_custom_shapes_general_rounding_l2_l3(O, monkeypatch, shape, kernel):
    """k_blind_rotate<2, false> / <3, false> and their latency-kernel counterparts, which no reference set runs where the
    product is inexact: (n, l, bgbit) = (48, 2, 16) -- inexact -- and (48, 3, 10), general rounding (6 * 1024 * 512 * 2^31
    > 2^51) with random operands far below the bound, so the CPU path is exact and the device must give its words."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import SecurityParams

    n, l, bgbit, seed = shape
    # the (near) noise-free key of test_extreme_parameter_shapes for the wide digit
    op = O.Params(f"LOCKSTEP_{n}_{l}_{bgbit}", n, l, bgbit, 2, 3, 2.0e-5, 2.0e-8 if bgbit <= 10 else 2.2e-16)
    sk, ck = oracle_keys(O, op, seed=seed, with_time=True)
    pp = SecurityParams(op.name, 0, n, l, bgbit, 2, 3, op.alpha_lv0, op.alpha_lv1)
    pk = R.CloudKey(pp, ck.bootstrapping_key, ck.key_switching_key, ck.decomposition_offset, ck.blind_rotate_testvec)
    pos, ct, tv = _chain_inputs(n, 910 + l)
    rows = LS.prefix_rows(ct, pos)
    eng = _forced_engine(monkeypatch, pk, kernel, len(rows))
    assert eng.rounding_mode == "general"
    states = eng.batch_blind_rotate(rows, tv)
    eng.close()
    pairs = LS.check_chain(O, ck, states, ct, pos, tv, LS.is_exact_regime(op), label=f"{op.name} {kernel}")
    _record(f"lockstep {op.name} {kernel}: worst e_dev/e_cpu {LS.worst_ratio(pairs):.3f} max e_cpu {max(p[1] for p in pairs)}")


# ---- crafted large magnitudes ------------------------------------------------------------------------------------------------
# One active step (b = 0: X^2N * testvec = testvec; a~ = N: X^N * c = MAX - c, quirk Q1, so d = -2c - 1 word by word) under a
# key whose time-domain polynomials are +-A everywhere.  With every digit of one sign and the key constant, coefficient j
# of a digit polynomial times a key polynomial is D * A * (2 (j + 1) - N): all N terms line up at j = N - 1, and the two
# rows of l = 1 add up.  A is chosen so that the largest pre-rounding value is 2^62 (bgbit 22 / 23) or 2^58 (bgbit 18):
# inside the |x| < 2^63 the kernels' rounding claims (fft512.hpp), 2^5 above what uniform inputs give.
class _CraftedKey:
    pass


def _crafted_key(O, n, bgbit, amp, alternate):
    from rs_tfhe_amd.params import SecurityParams
    import rs_tfhe_amd as R

    op = O.Params(f"CRAFTED_bg{bgbit}", n, 1, bgbit, 2, 3, 2.0e-5, 2.2e-16)
    sign = np.where(np.arange(N) % 2 == 1, -1, 1) if alternate else np.ones(N, np.int64)
    poly = ((amp * sign) % (1 << 32)).astype(np.uint32)
    ck = _CraftedKey()
    ck.params = op
    ck.decomposition_offset = O.gen_decomposition_offset(1, bgbit)
    ck.bootstrapping_key_time = np.broadcast_to(poly, (n, 2, 2, N)).copy()
    spec = O.klemsa_ifft(poly)
    ck.bootstrapping_key = np.broadcast_to(spec, (n, 2, 2, N)).copy()
    pp = SecurityParams(op.name, 0, n, 1, bgbit, 2, 3, op.alpha_lv0, op.alpha_lv1)
    pk = R.CloudKey(pp, ck.bootstrapping_key, np.zeros((N, 3, 4, n + 1), np.uint32), ck.decomposition_offset, np.zeros((2, N), np.uint32))
    return ck, pk


def _prerounding_max(O, ck, d):
    """max |x| of the integer (not wrapped) external product, in exact integers"""
    P = ck.params
    dec = O.decomposition(d, 1, P.bgbit, ck.decomposition_offset).astype(np.int32).astype(np.int64)  # [2][N] signed digits
    key = ck.bootstrapping_key_time[0].astype(np.int32).astype(np.int64)  # [2 rows][2 polys][N]
    # (int64 holds it: the sum of the |terms| of one coefficient is at most 2 N (Bg/2) max|key| <= 2^62)
    assert 2 * N * (1 << (P.bgbit - 1)) * int(np.abs(key).max()) <= 1 << 62
    worst = 0
    for poly in range(2):
        acc = np.zeros(N, np.int64)
        for r in range(2):
            full = np.convolve(dec[r], key[r, poly])  # [2N - 1], integer arithmetic
            acc += full[:N] - np.concatenate([full[N:], [0]])
        worst = max(worst, int(np.abs(acc).max()))
    return worst


CRAFTED = [(22, 1 << 30, 62), (23, 1 << 29, 62), (18, 1 << 30, 58)]  # (bgbit, key amplitude, log2 of the largest pre-rounding value)


@pytest.mark.parametrize("bgbit,amp,log2max", CRAFTED, ids=lambda v: str(v))
def test_lockstep_crafted_large_magnitudes(O, monkeypatch, bgbit, amp, log2max):
    """Digit patterns all -Bg/2, all +Bg/2 - 1, and two sign patterns that line the terms up at another coefficient, under
    constant and alternating keys: through each forced fused kernel (one active step, check_chain) and through
    batch_external_product.  Bound: e_dev <= 2 max(e_cpu, ulp) with ulp = 2^(floor(log2 |x|max) - 52): one ulp of the largest
    partial sum is the floor of ANY f64 evaluation of that sum."""
    n, p = 16, 5
    G = 1 << (32 - bgbit)
    d_min, d_max = 0x80000001, 0x7FFFFFFF  # d = -2c - 1 is odd: the odd words of the lowest / highest digit field
    j = np.arange(N)
    patterns = {
        "all_min": (np.full(N, d_min, np.uint32), False),
        "all_max": (np.full(N, d_max, np.uint32), False),
        "step_300": (np.where(j <= 300, d_max, d_min).astype(np.uint32), False),  # terms line up at coefficient 300
        "alternating": (np.where(j % 2 == 0, d_min, d_max).astype(np.uint32), True),  # ... at N - 1 under the alternating key
    }
    seen_max = 0
    for name, (dword, alternate) in patterns.items():
        ck, pk = _crafted_key(O, n, bgbit, amp, alternate)
        d = np.stack([dword, dword])
        c = (((-d.astype(np.int64) - 1) % (1 << 32)) >> 1).astype(np.uint32)  # d = -2c - 1
        dec = O.decomposition(d, 1, bgbit, ck.decomposition_offset).astype(np.int32)
        half = 1 << (bgbit - 1)
        assert set(np.unique(dec).tolist()) <= {-half, half - 1}
        if name == "all_min":
            assert (dec == -half).all() and G > 1
        if name == "all_max":
            assert (dec == half - 1).all()
        xmax = _prerounding_max(O, ck, d)
        assert xmax < (1 << 63)
        seen_max = max(seen_max, xmax)
        ulp = 1 << max(int(math.floor(math.log2(xmax))) - 52, 0)
        ct = np.zeros(n + 1, np.uint32)
        ct[p] = N << 21
        rows = LS.prefix_rows(ct, [p])
        for kernel in KERNELS:
            eng = _forced_engine(monkeypatch, pk, kernel, len(rows))
            states = eng.batch_blind_rotate(rows, c)
            stage = eng.batch_external_product(d[None], np.array([p], np.int32))[0]
            eng.close()
            assert np.array_equal((LS.rotate(O, states[0], N) - states[0]).astype(np.uint32), d)
            pairs = LS.check_chain(O, ck, states, ct, [p], c, False, floor=ulp, label=f"crafted bgbit {bgbit} {name} {kernel}")
            exact = O.external_product_exact(ck.bootstrapping_key_time[p], d, 1, bgbit, ck.decomposition_offset)
            cpu = O.external_product_fft(ck.bootstrapping_key[p], d, 1, bgbit, ck.decomposition_offset)
            e_stage, e_cpu = signed_diff(stage, exact), signed_diff(cpu, exact)
            _record(f"crafted bgbit {bgbit} {name} {kernel}: |x|max 2^{math.log2(xmax):.2f} ulp {ulp} fused e_dev {pairs[0][0]} stage e_dev {e_stage} e_cpu {e_cpu}")
            assert e_stage <= 2 * max(e_cpu, ulp), (bgbit, name, kernel, e_stage, e_cpu, ulp)
    assert seen_max == 1 << log2max, math.log2(seen_max)


def test_relative_twiddle_mutation_is_caught():
    """The suite must NOTICE a fused kernel whose floating-point error is above the reference's: the lock-step cases above,
    run as a child process against a mutation build (csrc/experiment.hpp TFHE_ABL_TW_REL: in the three fused blind-rotation
    kernels one pass-2 twiddle entry carries a relative error of 2^-47; `make -C rs-tfhe_amd/csrc mutation`), have to FAIL on
    every inexact set through all three kernels -- with assertion errors of check_chain, not for any other reason -- and
    still pass on SECURITY_128_BIT, where the same relative error moves no rounding."""
    import subprocess
    import sys
    import xml.etree.ElementTree as ET

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "rs-tfhe_amd", "libtfhe_v_tw_rel.so")
    subprocess.check_call(["make", "-C", os.path.join(root, "rs-tfhe_amd", "csrc"), "mutation"], stdout=subprocess.DEVNULL)
    assert os.path.exists(lib), "mutation build missing: make -C rs-tfhe_amd/csrc mutation"
    env = dict(os.environ, TFHE_HIP_LIB=lib, TFHE_HIP_ALLOW_EXPERIMENT="1")
    import tempfile

    tmp = tempfile.TemporaryDirectory()
    xml = os.path.join(tmp.name, "mutation_tw_rel_junit.xml")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_lockstep.py"), "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_lockstep_every_set_every_kernel", "--junitxml", xml], cwd=root, env=env,
                       capture_output=True, text=True, timeout=1500)
    out = p.stdout + p.stderr
    assert p.returncode == 1, out[-3000:]
    outcome, message = {}, {}
    for case in ET.parse(xml).getroot().iter("testcase"):
        fail, err = case.find("failure"), case.find("error")
        outcome[case.get("name")] = "error" if err is not None else ("failed" if fail is not None else "passed")
        message[case.get("name")] = (fail.get("message") or "") + (fail.text or "") if fail is not None else ""
    assert len(outcome) == 3 * (len(INEXACT_SETS) + len(EXACT_SETS)), outcome
    for setname in INEXACT_SETS:
        for kernel in KERNELS:
            k = f"test_lockstep_every_set_every_kernel[{setname}-{kernel}]"
            assert outcome[k] == "failed" and "AssertionError" in message[k] and "lockstep check_chain" in message[k] and "e_dev" in message[k], (
                k, outcome[k], message[k][-1500:])
    for kernel in KERNELS:
        assert outcome[f"test_lockstep_every_set_every_kernel[SECURITY_128_BIT-{kernel}]"] == "passed", (outcome, out[-3000:])
    assert "ImportError" not in out and "Error loading" not in out
    for k in sorted(outcome):  # the mutant's own figures, next to the unmutated kernels' in DESIGN section 7
        m = [ln for ln in message[k].splitlines() if "lockstep check_chain" in ln]
        _record(f"mutant tw_rel {k}: {outcome[k]} {m[0].strip()[:200] if m else ''}")
