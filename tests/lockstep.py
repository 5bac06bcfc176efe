"""Lock-step harness: hold every CMUX step of a blind rotation to the EXACT integer product (used by
tests/test_lockstep_host.py with the CPU f64 path standing in for the device, and by tests/test_gpu_lockstep.py on the
fused HIP kernels).  No device import.

Whole rotations cannot be compared sharply where the f64 product is inexact (bgbit >= 15): one flipped decomposition
digit makes the f64 rotation and the exact-integer rotation of the same ciphertext two different valid noise
realisations.  But a CMUX step whose mask word is 0 is an exact identity (trgsw.rs:198-226: a~ = 0, X^0 * acc - acc = 0,
the digits of 0 + offset are all 0, the f64 product of zeros is 0), so a ciphertext that keeps only the first k of an
ascending list of mask positions returns the accumulator after exactly k real steps.  Row k - 1 of such a family is the
INPUT of row k's last step: that step is recomputed from the device's own previous state with the exact integer
product and with the CPU f64 path, and the device's error against the exact product may be at most twice the CPU
path's (the bar of DESIGN section 7) -- per step, per word, with no divergence.
"""
import numpy as np

from conftest import signed_diff

N = 1024


def a_tilda(word):
    """(a +wrap 2^20) >> 21 (trgsw.rs:210-211)"""
    return ((int(word) + (1 << 20)) & 0xFFFFFFFF) >> 21


def b_tilda(body):
    """2N - ((b as usize + 2^20) >> 21), a non-wrapping add (trgsw.rs:202-203)"""
    return 2 * N - ((int(body) + (1 << 20)) >> 21)


# the three blind-rotation kernels, each forced at every batch size (TFHE_HIP_BR_KERNEL, include/tfhe_hip.h): eight waves
# per ciphertext (default up to #CUs), two ciphertexts per eight-wave workgroup (default for #CUs < count <= 2 #CUs),
# the batch kernel
BR_KERNEL_ENVS = {
    "single": {"TFHE_HIP_BR_KERNEL": "single"},
    "pair": {"TFHE_HIP_BR_KERNEL": "pair"},
    "batch": {"TFHE_HIP_BR_KERNEL": "batch"},
}


def with_br_kernel(monkeypatch, name):
    for k, v in BR_KERNEL_ENVS[name].items():
        monkeypatch.setenv(k, v)


FORCED_A_TILDA = (1, N - 1, N, N + 1, 2 * N - 1)
FORCED_STEPS = (1, 5, 8, 11, 13)  # which steps of the chain carry them: inside the consecutive run and outside it


def mask_positions(n):
    """Ascending (the rotation walks the mask in index order, so row k's new position must be its LAST active step):
    position 0, two spread ones, eight consecutive ones in the middle (the steady state of the loop and its cross-step
    prefetch), two spread ones, position n - 1.  K = 14."""
    mid = n // 2
    pos = [0, n // 9, n // 5] + list(range(mid - 4, mid + 4)) + [(3 * n) // 4, (7 * n) // 8, n - 1]
    assert all(x < y for x, y in zip(pos, pos[1:])) and pos[0] == 0 and pos[-1] == n - 1, (n, pos)
    return pos


def make_ciphertext(n, positions, seed):
    """[n + 1] u32: random words at `positions` and in the body, 0 elsewhere; the steps FORCED_STEPS carry the edge
    rotation amounts a~ = 1, N - 1, N, N + 1, 2N - 1 (a = a~ << 21).  No active step has a~ = 0."""
    rng = np.random.default_rng(seed)
    ct = np.zeros(n + 1, np.uint32)
    for i in positions:
        w = 0
        while a_tilda(w) == 0:
            w = int(rng.integers(0, 2**32))
        ct[i] = w
    for step, at in zip(FORCED_STEPS, FORCED_A_TILDA):
        ct[positions[step]] = at << 21
    ct[n] = int(rng.integers(0, 2**32))
    return ct


def prefix_rows(full_ct, positions):
    """[K + 1][n + 1]: row k keeps full_ct[n] and full_ct[positions[:k]]; every other mask word is 0."""
    full_ct = np.asarray(full_ct, np.uint32)
    rows = np.zeros((len(positions) + 1, len(full_ct)), np.uint32)
    rows[:, -1] = full_ct[-1]
    for k in range(1, len(positions) + 1):
        sel = list(positions[:k])
        rows[k, sel] = full_ct[sel]
    return rows


def rotate(O, trlwe, k):
    return np.stack([O.poly_mul_with_x_k(trlwe[0], k), O.poly_mul_with_x_k(trlwe[1], k)])


def step_products(O, ck, state, i, word):
    """(exact, cpu): the accumulator after the CMUX step of key row i and mask word `word` from `state`, with the exact
    integer product (bootstrapping_key_time) and with the CPU f64 path (bootstrapping_key)."""
    P = ck.params
    state = np.asarray(state, np.uint32)
    d = (rotate(O, state, a_tilda(word)) - state).astype(np.uint32)
    off = ck.decomposition_offset
    exact = (state + O.external_product_exact(ck.bootstrapping_key_time[i], d, P.l, P.bgbit, off)).astype(np.uint32)
    cpu = (state + O.external_product_fft(ck.bootstrapping_key[i], d, P.l, P.bgbit, off)).astype(np.uint32)
    return exact, cpu


def _worst_word(a, b):
    d = np.abs((np.asarray(a, np.uint32) - np.asarray(b, np.uint32)).astype(np.int32).astype(np.int64))
    j = int(d.argmax())
    return ("a" if j < N else "b", j % N, int(d.reshape(-1)[j]))


def check_chain(O, ck, states, full_ct, positions, testvec, exact_regime, floor=1, label=""):
    """states[k]: the device's TRLWE [2][N] for row k of prefix_rows(full_ct, positions).

    Row 0 must equal X^b~ * testvec exactly (an integer stage).  Every k >= 1, from the device's own states[k - 1]:
        e_dev = |states[k] - exact|,  e_cpu = |cpu - exact|   (max over the 2N words, wrapping)
        assert e_dev <= 2 * max(e_cpu, floor)                  (floor = 1 LSB unless the caller derives another)
    and in the exact regime e_dev == 0 and states[k] == cpu word for word.  Where the product is inexact at least 3/4 of
    the steps must have e_cpu > 0, or the bound would be the floor alone.  Returns the (e_dev, e_cpu) pairs."""
    states = np.asarray(states, np.uint32)
    testvec = np.asarray(testvec, np.uint32).reshape(2, N)
    K = len(positions)
    assert states.shape == (K + 1, 2, N), states.shape
    n = len(full_ct) - 1
    bt = b_tilda(full_ct[n])
    assert np.array_equal(states[0], rotate(O, testvec, bt)), f"lockstep check_chain {label}: row 0 is not X^{bt} * testvec"
    pairs = []
    for k in range(1, K + 1):
        i = positions[k - 1]
        word = int(full_ct[i])
        exact, cpu = step_products(O, ck, states[k - 1], i, word)
        e_dev, e_cpu = signed_diff(states[k], exact), signed_diff(cpu, exact)
        where = f"lockstep check_chain {label}: step {k} key row {i} a~ {a_tilda(word)} e_dev {e_dev} e_cpu {e_cpu} worst word {_worst_word(states[k], exact)}"
        assert e_dev <= 2 * max(e_cpu, floor), where
        if exact_regime:
            assert e_dev == 0, where
            assert np.array_equal(states[k], cpu), where
        pairs.append((e_dev, e_cpu))
    if not exact_regime:
        live = sum(e_cpu > 0 for _, e_cpu in pairs)
        assert 4 * live >= 3 * K, f"lockstep check_chain {label}: vacuous, only {live} of {K} steps have e_cpu > 0"
    return pairs


def worst_ratio(pairs, floor=1):
    return max(e_dev / max(e_cpu, floor) for e_dev, e_cpu in pairs)


def bsk_only_key(O, params, seed):
    """(secret key, cloud key) with the bootstrapping key in both domains and NO key-switching key (1.8 GB on
    SECURITY_UINT7 / 8, and no part of a blind rotation): orc_gen_bootstrapping_key as O.CloudKey calls it."""
    import ctypes as C

    sk = O.SecretKey(params, seed)
    ck = O.CloudKey.__new__(O.CloudKey)
    ck.params = params
    ck.decomposition_offset = O.gen_decomposition_offset(params.l, params.bgbit)
    ck.blind_rotate_testvec = O.gen_testvec()
    ck.bootstrapping_key = np.empty((params.n, 2 * params.l, 2, N), np.float64)
    ck.bootstrapping_key_time = np.empty((params.n, 2 * params.l, 2, N), np.uint32)
    ck.key_switching_key = np.zeros(1, np.uint32)  # never read by a blind rotation
    cp = params.c()
    O.lib().orc_gen_bootstrapping_key(C.c_uint64(seed * 2 + 1), C.byref(cp), sk.key_lv0.ctypes.data_as(C.c_void_p),
                                      sk.key_lv1.ctypes.data_as(C.c_void_p), ck.bootstrapping_key.ctypes.data_as(C.c_void_p),
                                      ck.bootstrapping_key_time.ctypes.data_as(C.c_void_p))
    return sk, ck


def is_exact_regime(params):
    """bgbit <= 10 in every reference set and test shape: the f64 product of the CPU path equals the integer product
    (measured: per-step CPU error 0 at bgbit 6 / 10, ~10 LSB at 18, 150-200 at 22, 300-450 at 23)."""
    return params.bgbit <= 10
