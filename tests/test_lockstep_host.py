"""The lock-step harness (tests/lockstep.py) proven on the CPU: the oracle's f64 blind rotation stands in for the device.
The chain passes on exact and inexact parameter sets, the identity-step premise holds word for word, and the harness
fails on a state moved just past the bound, on a step that used the neighbouring key row and on a rotation amount off
by one.  No device."""
import numpy as np
import pytest

import lockstep as LS

N = 1024
SETS = ["SECURITY_128_BIT", "SECURITY_UINT1", "SECURITY_UINT2", "SECURITY_UINT3", "SECURITY_UINT4", "SECURITY_UINT8"]
_CACHE = {}


def _case(O, setname):
    """key, ciphertext, positions, test vector and the CPU path's states for the K + 1 prefix rows (full-n rotations)"""
    if setname not in _CACHE:
        P = O.PARAM_SETS[setname]
        sk, ck = LS.bsk_only_key(O, P, 31)
        pos = LS.mask_positions(P.n)
        ct = LS.make_ciphertext(P.n, pos, 32)
        tv = np.random.default_rng(33).integers(0, 2**32, (2, N), dtype=np.uint64).astype(np.uint32)
        states = O.batch_blind_rotate(ck, LS.prefix_rows(ct, pos), tv)
        _CACHE[setname] = (P, ck, ct, pos, tv, states)
    return _CACHE[setname]


def test_positions_and_rows():
    for n in (48, 550, 687, 1160):
        pos = LS.mask_positions(n)
        assert len(pos) >= 14 and pos[0] == 0 and pos[-1] == n - 1
        run = max(len(r) for r in np.split(np.array(pos), np.where(np.diff(pos) != 1)[0] + 1))
        assert run >= 8
        ct = LS.make_ciphertext(n, pos, 5)
        assert [LS.a_tilda(ct[pos[s]]) for s in LS.FORCED_STEPS] == list(LS.FORCED_A_TILDA)
        assert all(LS.a_tilda(ct[i]) != 0 for i in pos)
        rows = LS.prefix_rows(ct, pos)
        assert rows.shape == (len(pos) + 1, n + 1) and (rows[:, n] == ct[n]).all()
        assert not rows[0, :n].any() and np.array_equal(rows[-1], ct)
        for k in range(1, len(pos) + 1):
            assert np.flatnonzero(rows[k, :n]).tolist() == pos[:k]


@pytest.mark.parametrize("setname", SETS)
def test_chain_passes_on_the_cpu_path_and_the_identity_premise_holds(O, setname):
    P, ck, ct, pos, tv, states = _case(O, setname)
    exact = LS.is_exact_regime(P)
    pairs = LS.check_chain(O, ck, states, ct, pos, tv, exact, label=setname)
    assert len(pairs) == len(pos) >= 14
    # the premise: the n - k steps with a zero mask word change NOTHING -- row 0 of a full n-step rotation is the rotated
    # test vector (check_chain) under the exact product too, and row k is row k - 1 plus ONE f64 step, word for word
    assert np.array_equal(O.blind_rotate(ck, LS.prefix_rows(ct, pos)[0], tv, exact=True), states[0])
    for k in range(1, len(pos) + 1):
        _, cpu = LS.step_products(O, ck, states[k - 1], pos[k - 1], ct[pos[k - 1]])
        assert np.array_equal(states[k], cpu), (setname, k)
    assert all(e_dev == e_cpu for e_dev, e_cpu in pairs)
    if exact:
        assert all(e_cpu == 0 for _, e_cpu in pairs)
    else:
        assert all(e_cpu > 0 for _, e_cpu in pairs), pairs
    print(setname, "per-step CPU error:", [e for _, e in pairs])


@pytest.mark.parametrize("setname", ["SECURITY_128_BIT", "SECURITY_UINT3", "SECURITY_UINT4"])
def test_harness_fails_on_a_state_past_the_bound(O, setname):
    P, ck, ct, pos, tv, states = _case(O, setname)
    exact = LS.is_exact_regime(P)
    pairs = LS.check_chain(O, ck, states, ct, pos, tv, exact)
    k = len(pos)  # the last state: no later step starts from it
    bad = states.copy()
    ex, cpu = LS.step_products(O, ck, states[k - 1], pos[k - 1], ct[pos[k - 1]])
    j = int(np.abs((cpu - ex).astype(np.int32).astype(np.int64)).argmax())  # the word where the CPU path errs most
    err = int((cpu - ex).astype(np.int32).reshape(-1)[j])
    sign = 1 if err >= 0 else -1
    bad.reshape(len(pos) + 1, -1)[k, j] = (int(ex.reshape(-1)[j]) + sign * (2 * max(pairs[k - 1][1], 1) + 1)) % 2**32
    with pytest.raises(AssertionError, match="lockstep check_chain"):
        LS.check_chain(O, ck, bad, ct, pos, tv, exact)
    # 2 e_cpu + 2 from the CPU's own value in one word of a middle state fails too (that step, or the one starting from it)
    bad = states.copy()
    bad[7, 1, 100] += np.uint32(2 * max(pairs[6][1], 1) + 2 + abs(int((states[7] - LS.step_products(O, ck, states[6], pos[6], ct[pos[6]])[0]).astype(np.int32)[1, 100])))
    with pytest.raises(AssertionError, match="lockstep check_chain"):
        LS.check_chain(O, ck, bad, ct, pos, tv, exact)


def _chain(O, ck, ct, pos, tv, row_of=lambda k, i: i, word_of=lambda k, w: w):
    """states built step by step with the CPU f64 path, with a hook to use another key row / mask word at some step"""
    states = [LS.rotate(O, tv, LS.b_tilda(ct[-1]))]
    for k in range(1, len(pos) + 1):
        i = pos[k - 1]
        states.append(LS.step_products(O, ck, states[-1], row_of(k, i), word_of(k, int(ct[i])))[1])
    return np.stack(states)


@pytest.mark.parametrize("setname", ["SECURITY_128_BIT", "SECURITY_UINT4"])
def test_harness_fails_on_the_wrong_key_row_and_on_a_rotation_off_by_one(O, setname):
    P, ck, ct, pos, tv, states = _case(O, setname)
    exact = LS.is_exact_regime(P)
    assert np.array_equal(_chain(O, ck, ct, pos, tv), states)
    for step in (1, 6, len(pos) - 1):  # (the last position is n - 1: no row n)
        bad = _chain(O, ck, ct, pos, tv, row_of=lambda k, i: i + 1 if k == step else i)
        with pytest.raises(AssertionError, match=f"step {step} key row {pos[step - 1]} "):
            LS.check_chain(O, ck, bad, ct, pos, tv, exact)
    for step in (2, 9, len(pos)):  # step 2 carries a~ = 1, step 9 a~ = N, the last 2N - 1: each one lower
        bad = _chain(O, ck, ct, pos, tv, word_of=lambda k, w: (w - (1 << 21)) % 2**32 if k == step else w)
        with pytest.raises(AssertionError, match=f"step {step} key row {pos[step - 1]} "):
            LS.check_chain(O, ck, bad, ct, pos, tv, exact)
    bad = states.copy()
    bad[0] = LS.rotate(O, tv, LS.b_tilda(ct[-1]) - 1)
    with pytest.raises(AssertionError, match="row 0"):
        LS.check_chain(O, ck, bad, ct, pos, tv, exact)
