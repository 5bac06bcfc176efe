"""The native circuit scheduler on the GPU (tfhe_hip_circuit_*): every wire word for word against the CPU oracle
evaluating the same nodes one by one (Circuit.run_reference), against the torch-scheduled path it replaces, through a
pool, and through the C++ binding.  These are hand-built circuits; seeded random DAGs, every scheduler path by name and
every dispatch regime word for word against the oracle are in tests/test_gpu_circuit_fuzz.py."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cloud_key(ck):
    import rs_tfhe_amd as R
    from rs_tfhe_amd import params as P

    if not hasattr(ck, "_product"):
        ck._product = R.CloudKey(P.PARAM_SETS[ck.params.name], ck.bootstrapping_key, ck.key_switching_key,
                                 ck.decomposition_offset, ck.blind_rotate_testvec)
    return ck._product


def _engine(ck):
    import rs_tfhe_amd as R

    pk = _cloud_key(ck)
    eng = R.bootstrap.engine_for(pk.params, 0)
    eng.ensure_key(pk)
    return eng


def _adder_inputs(sk, bits, xs, ys, cin, seed):
    planes = [(xs >> i) & 1 for i in range(bits)] + [(ys >> i) & 1 for i in range(bits)] + [cin]
    return np.stack([sk.encrypt_bool(p.astype(bool), seed + k) for k, p in enumerate(planes)])


def _decode_sum(sk, wires, sum_w, carry_w):
    total = np.zeros(wires.shape[1], np.int64)
    for i, w in enumerate(sum_w):
        total += sk.decrypt_bool(wires[w]).astype(np.int64) << i
    return total + (sk.decrypt_bool(wires[carry_w]).astype(np.int64) << len(sum_w))


@pytest.mark.parametrize("B", [1, 7, 4096])
def test_add16_native(O, keys128, B):
    """16-bit ripple-carry addition (examples/add_two_numbers.rs) at SECURITY_128_BIT: words equal the torch-scheduled
    path and, for B in {1, 7}, the oracle gate by gate (4096 x 80 CPU bootstraps would take the oracle an hour: the
    batch is held to the torch path and to the integer sums); decrypted sums equal integer sums."""
    import torch

    import rs_tfhe_amd as R

    sk, ck = keys128
    eng = _engine(ck)
    bits = 16
    rng = np.random.default_rng(7000 + B)
    xs, ys = rng.integers(0, 1 << bits, B), rng.integers(0, 1 << bits, B)
    cin = rng.integers(0, 2, B)
    c = R.Circuit(2 * bits + 1)
    sum_w, carry_w = c.add(list(range(bits)), list(range(bits, 2 * bits)), 2 * bits)
    inputs = _adder_inputs(sk, bits, xs, ys, cin, 7100 + B)
    wires = c.run(eng, inputs)
    assert np.array_equal(_decode_sum(sk, wires, sum_w, carry_w), xs + ys + cin)
    t = torch.from_numpy(inputs.view(np.int32)).to("cuda:0")
    nat = c.run_dev(eng, t)
    old = c._run_dev_torch(eng, t)
    torch.cuda.synchronize()
    nat, old = nat.cpu().numpy().view(np.uint32), old.cpu().numpy().view(np.uint32)
    assert np.array_equal(nat, old) and np.array_equal(nat, wires)
    if B <= 7:
        ref = c.run_reference(lambda op, a, b: O.batch_gate(ck, op, a, b), inputs)
        assert np.array_equal(wires, ref)


def test_mixed_node_kinds_80bit(O, keys80):
    """Every node kind at SECURITY_80_BIT: gates, mux chains, not, constant(false), a programmable bootstrap, a gate
    whose operand is a folded lincomb, one whose operand is materialised -- every wire against the oracle."""
    import rs_tfhe_amd as R

    sk, ck = keys80
    eng = _engine(ck)
    B = 5
    rng = np.random.default_rng(8000)
    bits = rng.integers(0, 2, (4, B)).astype(bool)
    inputs = np.stack([sk.encrypt_bool(bits[k], 8100 + k) for k in range(4)])
    c = R.Circuit(4)
    m1 = c.mux(0, 1, 2)
    m2 = c.mux(m1, 2, 3)             # a chain: level 2
    m3 = c.mux(3, m2, m1)            # level 3
    na = c.not_(m1)
    f = c.xor(na, 2)                 # folded: -m1 + 2*x2 + 1/4, a launch of its own
    g = c.and_(na, 3)                # folded onto and_ny(m1, x3): the gate launch
    k = c.constant(False)
    h = c.or_(k, 0)                  # one source wire, constant folded
    s3 = c.lincomb([(1, 0), (1, 1), (1, 2)])
    u = c.nand(s3, m2)               # materialised: three source wires
    gen = R.lut.Generator(2)
    lid = c.lut(gen.generate_lookup_table(lambda x: 1 - x).poly)
    p = c.pbs(1, m3, 1, u, 0, lid)
    out = c.mux(p, f, g)
    d = c.describe()
    assert any(lv["lincomb_launches"] for lv in d) and any(lv["lut_launches"] for lv in d)
    wires = c.run(eng, inputs)
    ref = c.run_reference(lambda op, a, b: O.batch_gate(ck, op, a, b), inputs,
                          mux_fn=lambda a, b, cc: O.batch_mux(ck, a, b, cc, naive=False),
                          pbs_fn=lambda tv, x: O.batch_bootstrap(ck, x, testvec=tv))
    bad = [w for w in range(c.n_wires) if not np.array_equal(wires[w], ref[w])]
    assert not bad, bad  # (Gates::mux's own formula does not decrypt to a ? b : c -- quirk Q5 -- the words are the claim)
    assert out == c.n_wires - 1 and h > 0


def _nibble_circuit(R):
    gen = R.lut.Generator(32)
    c = R.Circuit(4)
    mod16 = c.lut(gen.generate_lookup_table(lambda x: x % 16).poly)
    cry = c.lut(gen.generate_lookup_table(lambda x: 1 if x >= 16 else 0).poly)
    sl = c.pbs(1, 0, 1, 2, 0, mod16)
    cr = c.pbs(1, 0, 1, 2, 0, cry)
    sh = c.pbs(1, c.lincomb([(1, 1), (1, 3)]), 1, cr, 0, mod16)
    return c, (sl, sh, cr)


def test_nibble_adder_circuit(O, keys128, keys_uint4):
    """examples/lut_add_two_numbers.rs as pbs / lincomb nodes: the words of circuit.lut_add_u8_dev at SECURITY_128_BIT;
    at SECURITY_UINT4 the decrypted bytes are the plain sums."""
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd import circuit

    rng = np.random.default_rng(8200)
    a = rng.integers(0, 256, 33)
    b = rng.integers(0, 256, 33)
    for keys, seed in ((keys128, 8300), (keys_uint4, 8400)):
        sk, ck = keys
        eng = _engine(ck)
        cts = [sk.encrypt_lwe_message(v, 32, seed + k) for k, v in enumerate((a & 15, a >> 4, b & 15, b >> 4))]
        c, (sl, sh, cr) = _nibble_circuit(R)
        wires = c.run(eng, np.stack(cts))
        t = [torch.from_numpy(x.view(np.int32)).to("cuda:0") for x in cts]
        want = circuit.lut_add_u8_dev(eng, *t)
        torch.cuda.synchronize()
        want = [x.cpu().numpy().view(np.uint32) for x in want]
        assert np.array_equal(wires[sl], want[0]) and np.array_equal(wires[sh], want[1]) and np.array_equal(wires[cr], want[2])
        if keys is keys_uint4:
            got = sk.decrypt_lwe_message(wires[sl], 32) + (sk.decrypt_lwe_message(wires[sh], 32) << 4)
            assert np.array_equal(got, (a + b) % 256)


def test_pool_two_members_one_gpu(O, keys128):
    """The nibble adder and a 4-bit adder through R.Pool(params, [0, 0]) with home 0 and home 1: the engine's words."""
    import torch

    import rs_tfhe_amd as R

    sk, ck = keys128
    eng = _engine(ck)
    pool = R.Pool(eng.params, [0, 0])
    try:
        pool.load_cloud_key(_cloud_key(ck))
        rng = np.random.default_rng(8500)
        a, b = rng.integers(0, 256, 300), rng.integers(0, 256, 300)
        cts = np.stack([sk.encrypt_lwe_message(v, 32, 8600 + k) for k, v in enumerate((a & 15, a >> 4, b & 15, b >> 4))])
        c, _ = _nibble_circuit(R)
        want = c.run(eng, cts)
        assert np.array_equal(c.run(pool, cts), want)
        bits = 4
        xs, ys, cin = rng.integers(0, 16, 300), rng.integers(0, 16, 300), rng.integers(0, 2, 300)
        adder = R.Circuit(2 * bits + 1)
        sum_w, carry_w = adder.add(list(range(bits)), list(range(bits, 2 * bits)), 2 * bits)
        m = adder.mux(0, 1, 2)
        ins = _adder_inputs(sk, bits, xs, ys, cin, 8700)
        want_add = adder.run(eng, ins)
        for home in (0, 1):
            pool.home = home
            for circ, x, w in ((c, cts, want), (adder, ins, want_add)):
                got = circ.run_dev(pool, torch.from_numpy(x.view(np.int32)).to("cuda:0"))
                pool.synchronize()
                torch.cuda.synchronize()
                assert np.array_equal(got.cpu().numpy().view(np.uint32), w), (home, circ.n_wires)
        assert np.array_equal(_decode_sum(sk, want_add, sum_w, carry_w), xs + ys + cin) and m > 0
    finally:
        pool.close()


def test_batch_limit_and_missing_key(O, keys128):
    """slots x B >= 2^32 is refused; a context without a key is refused before anything runs."""
    import ctypes as C

    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi

    sk, ck = keys128
    eng = _engine(ck)
    import torch

    c = R.Circuit(3)
    c.xor(0, 1)
    h = c._native_handle()
    lib = _capi.lib()
    # a real (small) allocation as the store: whatever order the checks run in, nothing can be written outside it
    store = torch.zeros((c.slots, 1, eng.params.n + 1), dtype=torch.int32, device="cuda:0")
    big = 2 ** 32 // c.slots + 1
    assert lib.tfhe_hip_circuit_run_dev(eng._ctx, h, None, C.c_void_p(store.data_ptr()), big, None) == _capi.EINVAL
    bare = R.Engine(eng.params, 0)
    try:
        assert lib.tfhe_hip_circuit_run_dev(bare._ctx, h, None, C.c_void_p(store.data_ptr()), 1, None) == _capi.ENOKEY
    finally:
        bare.close()
    torch.cuda.synchronize()
    assert not store.any()


def test_cpp_circuit_program():
    """tests/cpp/test_circuit.cpp: rs_tfhe::Circuit::add over 8 bits, B = 7, against the oracle library it links."""
    import tempfile

    from test_circuit_host import build_cpp_circuit

    with tempfile.TemporaryDirectory() as d:
        exe = build_cpp_circuit(d)
        p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "test_circuit ok" in p.stdout


def test_concurrent_pool_runs_of_one_circuit(O, keys128):
    """Four threads run ONE circuit through one pool and a key view of it (same members, same key), host-array and
    device-resident runs on streams of their own, over and over: each gets its own words (the engine's).  Runs of a
    circuit through a pool share its staging; the library serialises them."""
    import threading

    import torch

    import rs_tfhe_amd as R

    sk, ck = keys128
    eng = _engine(ck)
    pool = R.Pool(eng.params, [0, 0])
    view = None
    try:
        pool.load_cloud_key(_cloud_key(ck))
        view = pool.new_key_view()
        view.load_cloud_key(_cloud_key(ck))
        bits, B = 4, 96
        c = R.Circuit(2 * bits + 1)
        c.add(list(range(bits)), list(range(bits, 2 * bits)), 2 * bits)
        c.mux(0, 1, 2)
        rng = np.random.default_rng(8800)
        ins = [_adder_inputs(sk, bits, rng.integers(0, 16, B), rng.integers(0, 16, B), rng.integers(0, 2, B), 8900 + 20 * k)
               for k in range(4)]
        want = [c.run(eng, x) for x in ins]
        errors = []

        def host(k, handle):
            try:
                for _ in range(3):
                    if not np.array_equal(c.run(handle, ins[k]), want[k]):
                        errors.append(f"host run {k} differs")
            except Exception as e:  # noqa: BLE001
                errors.append(repr(e))

        def dev(k, handle):
            try:
                s = torch.cuda.Stream(device=0)
                x = torch.from_numpy(ins[k].view(np.int32)).to("cuda:0")
                for _ in range(3):
                    with torch.cuda.stream(s):
                        got = c.run_dev(handle, x, stream=s)
                    s.synchronize()
                    handle.synchronize()
                    if not np.array_equal(got.cpu().numpy().view(np.uint32), want[k]):
                        errors.append(f"device run {k} differs")
            except Exception as e:  # noqa: BLE001
                errors.append(repr(e))

        threads = [threading.Thread(target=host, args=(0, pool)), threading.Thread(target=host, args=(1, view)),
                   threading.Thread(target=dev, args=(2, pool)), threading.Thread(target=dev, args=(3, view))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=600)
        assert not any(t.is_alive() for t in threads), "a run did not finish"
        assert not errors, errors
    finally:
        if view is not None:
            view.close()
        pool.close()
