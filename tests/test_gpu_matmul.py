"""Encrypted linear layers on the GPU: tfhe_hip_batch_tlwe_matmul and tfhe_hip_batch_trlwe_matmul equal the numpy models
of rs_tfhe_amd.linear word for word (np.array_equal, no tolerance) on every shape that takes another path of the kernel
(row, K and column tails, unaligned weight rows, more than 1024 columns, the accumulator bound at cols = 65,536), the
key-switched packed form equals the oracle's identity_key_switching of the model's rows under every key-switch kernel,
the _dev forms give the host forms' bits on a side stream, the error codes, and one neuron end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1024
KEY_SEED = 33
EDGES = (0, 0x80000000, 0xFFFFFFFF, 0x7F7F7F7F, 0x80808080, 0x00800080, 0x7FFFFFFF)  # carries between balanced byte planes
DENSE_SHAPES = ((1, 1, 1), (32, 32, 1), (33, 31, 2), (65, 100, 3), (5, 1025, 1))  # (rows, cols, groups)
PACKED_SHAPES = ((1, 1, 1), (33, 1, 2), (7, 1023, 1), (40, 1024, 3))
_CACHE = {}


def weights(rng, rows, cols):
    """Random in [-128, 127]; the first rows all -128, all 127, all 0."""
    w = rng.integers(-128, 128, (rows, cols)).astype(np.int8)
    for r, v in zip(range(rows), (-128, 127, 0)):
        w[r] = v
    return w


def plant(words):
    """EDGES in every group of [groups][rows][width] words: down column 0 and down the last column (as many rows as
    there are), and along the first and the last row's leading words (so that one-row inputs carry all of them)."""
    k = min(len(EDGES), words.shape[1])
    words[:, :k, 0] = EDGES[:k]
    words[:, :k, -1] = EDGES[:k]
    words[:, 0, 1:1 + len(EDGES)] = EDGES
    words[:, -1, -1 - len(EDGES):-1] = EDGES
    return words


def dense_case(p, rows, cols, groups, seed):
    rng = np.random.default_rng(seed)
    w = weights(rng, rows, cols)
    bias = rng.integers(0, 1 << 32, rows, dtype=np.uint32)
    cts = plant(rng.integers(0, 1 << 32, (groups, cols, p.n + 1), dtype=np.uint32))
    return w, bias, cts


def packed_case(rows, cols, groups, seed):
    rng = np.random.default_rng(seed)
    w = weights(rng, rows, cols)
    bias = rng.integers(0, 1 << 32, rows, dtype=np.uint32)
    trlwe = rng.integers(0, 1 << 32, (groups, 2, N), dtype=np.uint32)
    trlwe[:, :, :len(EDGES)] = EDGES  # slot 0 onwards of a and b ...
    trlwe[:, :, -len(EDGES):] = EDGES  # ... and the end of the rows, which the negated words of every slot read
    return w, bias, trlwe


@pytest.mark.parametrize("name", ["SECURITY_80_BIT", "SECURITY_128_BIT", "SECURITY_UINT8"])
def test_dense_equals_the_model(name):
    import rs_tfhe_amd as R
    from rs_tfhe_amd import linear as L
    from rs_tfhe_amd.params import PARAM_SETS

    p = PARAM_SETS[name]
    e = R.Engine(p, 0)  # no key: the dense form needs none
    try:
        for i, (rows, cols, groups) in enumerate(DENSE_SHAPES):
            w, bias, cts = dense_case(p, rows, cols, groups, 100 + i)
            got = e.batch_tlwe_matmul(w, cts, bias)
            assert got.shape == (groups, rows, p.n + 1) and got.dtype == np.uint32
            assert np.array_equal(got, L.matmul_model(p, w, cts, bias)), (rows, cols, groups)
        w, bias, cts = dense_case(p, 33, 31, 2, 7)
        assert np.array_equal(e.batch_tlwe_matmul(w, cts), L.matmul_model(p, w, cts))  # bias NULL
        assert e.batch_tlwe_matmul(w, cts[:0]).shape == (0, 33, p.n + 1)  # groups == 0
    finally:
        e.close()


def test_dense_dev_form_writes_every_tile_over_a_sentinel():
    """The _dev form into an output the caller filled with 0xA5A5A5A5, against the model: a tile the launch never computed
    keeps the sentinel, whatever the allocator handed out (the host form's staging buffer holds what it held).  Workgroup
    counts 5, 10 and 30 at n + 1 = 551 (five column blocks): none a multiple of the eight dies the tiles are dealt to,
    with one and with two row blocks."""
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd import linear as L
    from rs_tfhe_amd.params import SECURITY_80_BIT as p

    def dev(a):
        return torch.from_numpy(a.view(np.int8 if a.dtype == np.int8 else np.int32)).to("cuda:0")

    e = R.Engine(p, 0)
    try:
        for rows, cols, groups in ((1, 1, 1), (33, 31, 2), (65, 100, 3)):
            w, bias, cts = dense_case(p, rows, cols, groups, 600 + cols)
            want = L.matmul_model(p, w, cts, bias)
            assert not (want == 0xA5A5A5A5).any()
            out = torch.full((groups, rows, p.n + 1), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda:0")
            e.batch_tlwe_matmul_dev(dev(w), dev(cts), out, bias=dev(bias))  # torch's current stream
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want), (rows, cols, groups)
    finally:
        e.close()


def test_dense_accumulator_bound_at_65536_columns():
    """w all -128 against words 0x80808080 (plane bytes -128, -127, -127, -127): plane 0 accumulates 65,536 * 2^14 = 2^30,
    the bound the header states; a handful of rows are random."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import linear as L
    from rs_tfhe_amd.params import SECURITY_80_BIT as p

    cols = 65536
    rng = np.random.default_rng(8)
    w = np.full((1, cols), -128, np.int8)
    cts = np.full((1, cols, p.n + 1), 0x80808080, np.uint32)
    some = rng.choice(cols, 5, replace=False)
    cts[0, some] = rng.integers(0, 1 << 32, (5, p.n + 1), dtype=np.uint32)
    bias = np.array([0xDEADBEEF], np.uint32)
    e = R.Engine(p, 0)
    try:
        assert np.array_equal(e.batch_tlwe_matmul(w, cts, bias), L.matmul_model(p, w, cts, bias))
    finally:
        e.close()


@pytest.mark.parametrize("name", ["SECURITY_128_BIT", "SECURITY_UINT4"])
def test_packed_without_key_switch_equals_the_model(name):
    import rs_tfhe_amd as R
    from rs_tfhe_amd import linear as L
    from rs_tfhe_amd.params import PARAM_SETS

    p = PARAM_SETS[name]
    e = R.Engine(p, 0)  # no key loaded
    try:
        for i, (rows, cols, groups) in enumerate(PACKED_SHAPES):
            w, bias, trlwe = packed_case(rows, cols, groups, 200 + i)
            got = e.batch_trlwe_matmul(w, trlwe, bias, keyswitch=False)
            assert got.shape == (groups, rows, N + 1)
            assert np.array_equal(got, L.matmul_packed_model(p, w, trlwe, bias)), (rows, cols, groups)
        w, bias, trlwe = packed_case(33, 31, 2, 9)
        assert np.array_equal(e.batch_trlwe_matmul(w, trlwe, keyswitch=False), L.matmul_packed_model(p, w, trlwe))
        assert e.batch_trlwe_matmul(w, trlwe[:0], keyswitch=False).shape == (0, 33, N + 1)
    finally:
        e.close()


def _keyed_case(O, name):
    """(client secret key, oracle cloud key of the engine's generated key, per packed shape (w, bias, trlwe, the oracle's
    key switch of the model's lv1 rows)), made once per parameter set."""
    if name not in _CACHE:
        import rs_tfhe_amd as R
        from rs_tfhe_amd import linear as L
        from rs_tfhe_amd.client import SecretKey
        from rs_tfhe_amd.params import PARAM_SETS

        p = PARAM_SETS[name]
        sk = SecretKey.new(p, 31)
        e = R.Engine(p, 0)
        try:
            e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=KEY_SEED)
            ck = e.export_cloud_key()
        finally:
            e.close()
        ock = O.CloudKey.from_arrays(getattr(O, name), ck.bootstrapping_key, ck.key_switching_key, ck.decomposition_offset,
                                     ck.blind_rotate_testvec)
        cases = []
        for i, (rows, cols, groups) in enumerate(PACKED_SHAPES):
            w, bias, trlwe = packed_case(rows, cols, groups, 300 + i)
            lv1 = L.matmul_packed_model(p, w, trlwe, bias)
            want = O.batch_identity_key_switching(ock, lv1.reshape(-1, N + 1)).reshape(groups, rows, p.n + 1)
            cases.append((w, bias, trlwe, want))
        _CACHE[name] = (sk, ock, cases)
    return _CACHE[name]


def _engine(name):
    import rs_tfhe_amd as R

    sk = _CACHE[name][0]
    e = R.Engine(sk.params, 0)
    e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=KEY_SEED)  # the seeded generator: the key _keyed_case exported
    return e


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import rs_tfhe_amd as R
from rs_tfhe_amd.client import SecretKey
from rs_tfhe_amd.params import PARAM_SETS
name, kernel, path = sys.argv[2:5]
p = PARAM_SETS[name]
z = np.load(path)
sk = SecretKey.new(p, 31)
e = R.Engine(p, 0)
e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=int(z["key_seed"]))
assert ("key_switch=" + kernel) in e.describe_dispatch(120), e.describe_dispatch(120)
out = {}
for i in range(int(z["cases"])):
    out["out%d" % i] = e.batch_trlwe_matmul(z["w%d" % i], z["trlwe%d" % i], z["bias%d" % i], keyswitch=True)
np.savez(path + ".out.npz", **out)
e.close()
"""


@pytest.mark.parametrize("name,kernel", [
    ("SECURITY_128_BIT", "mfma"), ("SECURITY_128_BIT", "b4"), ("SECURITY_128_BIT", "generic"), ("SECURITY_128_BIT", "split"),
    ("SECURITY_UINT4", "sliced"), ("SECURITY_UINT4", "generic"), ("SECURITY_UINT4", "split"),
])
def test_packed_with_key_switch_under_every_key_switch_kernel(O, tmp_path, name, kernel):
    """TFHE_HIP_KS_KERNEL is read when a context is created: a fresh child process per value."""
    sk, ock, cases = _keyed_case(O, name)
    path = str(tmp_path / "case.npz")
    arrays = {"key_seed": KEY_SEED, "cases": len(cases)}
    for i, (w, bias, trlwe, _) in enumerate(cases):
        arrays.update({"w%d" % i: w, "bias%d" % i: bias, "trlwe%d" % i: trlwe})
    np.savez(path, **arrays)
    env = dict(os.environ, TFHE_HIP_KS_KERNEL=kernel)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name, kernel, path], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.load(path + ".out.npz")
    for i, (w, bias, trlwe, want) in enumerate(cases):
        assert np.array_equal(out["out%d" % i], want), PACKED_SHAPES[i]


def test_dev_forms_give_the_host_forms_bits(O):
    """torch tensors on a side stream; cols = 31 and 100 put the device rows of w off 16-byte boundaries."""
    import torch

    name = "SECURITY_128_BIT"
    sk, ock, cases = _keyed_case(O, name)
    p = sk.params
    e = _engine(name)
    try:
        side = torch.cuda.Stream(device=0)

        def dev(a):
            return torch.from_numpy(a.view(np.int8 if a.dtype == np.int8 else np.int32)).to("cuda:0")

        for rows, cols, groups in ((33, 31, 2), (65, 100, 3)):
            w, bias, cts = dense_case(p, rows, cols, groups, 400 + cols)
            host = e.batch_tlwe_matmul(w, cts, bias)
            tw, tb, tin = dev(w), dev(bias), dev(cts)
            out = torch.full((groups, rows, p.n + 1), -1, dtype=torch.int32, device="cuda:0")
            side.wait_stream(torch.cuda.current_stream(0))
            e.batch_tlwe_matmul_dev(tw, tin, out, bias=tb, stream=side)
            side.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), host), (rows, cols, groups)
            w, bias, trlwe = packed_case(rows, cols, groups, 500 + cols)
            tw, tb, tin = dev(w), dev(bias), dev(trlwe)
            for ks in (False, True):
                host = e.batch_trlwe_matmul(w, trlwe, bias, keyswitch=ks)
                out = torch.full((groups, rows, (p.n if ks else N) + 1), -1, dtype=torch.int32, device="cuda:0")
                side.wait_stream(torch.cuda.current_stream(0))
                e.batch_trlwe_matmul_dev(tw, tin, out, bias=tb, keyswitch=ks, stream=side)
                side.synchronize()
                assert np.array_equal(out.cpu().numpy().view(np.uint32), host), (rows, cols, groups, ks)
            out = torch.full((groups, rows, N + 1), -1, dtype=torch.int32, device="cuda:0")
            e.batch_trlwe_matmul_dev(tw, tin, out, keyswitch=False)  # bias None, torch's current stream
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), e.batch_trlwe_matmul(w, trlwe, keyswitch=False))
    finally:
        e.close()


def test_matmul_error_codes():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import SECURITY_80_BIT as p

    lib = _capi.lib()
    vp = _capi.C.c_void_p
    w = np.ones((3, 4), np.int8)
    cts = np.zeros((2, 4, p.n + 1), np.uint32)
    trlwe = np.zeros((2, 2, N), np.uint32)
    out = np.zeros((2, 3, N + 1), np.uint32)
    wp, ip, tp, op = (a.ctypes.data_as(vp) for a in (w, cts, trlwe, out))
    e = R.Engine(p, 0)
    try:
        dense, dense_dev = lib.tfhe_hip_batch_tlwe_matmul, lib.tfhe_hip_batch_tlwe_matmul_dev
        packed, packed_dev = lib.tfhe_hip_batch_trlwe_matmul, lib.tfhe_hip_batch_trlwe_matmul_dev
        for bad in ((None, None, 3, 4, ip, 2, op), (wp, None, 3, 4, None, 2, op), (wp, None, 3, 4, ip, 2, None),  # NULL w, in, out
                    (wp, None, 0, 4, ip, 2, op), (wp, None, 3, 0, ip, 2, op), (wp, None, 3, 65537, ip, 2, op),  # rows, cols
                    (wp, None, 1 << 16, 4, ip, 1 << 15, op), (wp, None, 1 << 31, 4, ip, 1, op)):                 # rows * groups
            assert dense(e._ctx, *bad) == _capi.EINVAL, bad
            assert dense_dev(e._ctx, *bad, None) == _capi.EINVAL, bad
        for bad in ((None, None, 3, 4, tp, 2, 0, op), (wp, None, 3, 4, None, 2, 0, op), (wp, None, 3, 4, tp, 2, 0, None),
                    (wp, None, 0, 4, tp, 2, 0, op), (wp, None, 3, 0, tp, 2, 0, op), (wp, None, 3, N + 1, tp, 2, 0, op),
                    (wp, None, 1 << 16, 4, tp, 1 << 15, 0, op)):
            assert packed(e._ctx, *bad) == _capi.EINVAL, bad
            assert packed_dev(e._ctx, *bad, None) == _capi.EINVAL, bad
        assert dense(e._ctx, None, None, 3, 4, None, 0, None) == _capi.OK  # groups == 0 writes nothing
        assert packed_dev(e._ctx, None, None, 3, 4, None, 0, 0, None, None) == _capi.OK
        assert dense(None, wp, None, 3, 4, ip, 2, op) == _capi.EINVAL
        # the key-switched packed form alone needs the cloud key
        assert packed(e._ctx, wp, None, 3, 4, tp, 2, 1, op) == _capi.ENOKEY
        assert packed_dev(e._ctx, wp, None, 3, 4, tp, 2, 1, op, None) == _capi.ENOKEY
        with pytest.raises(_capi.TfheHipError) as ei:
            e.batch_trlwe_matmul(w, trlwe)
        assert ei.value.code == _capi.ENOKEY
        assert e.batch_trlwe_matmul(w, trlwe, keyswitch=False).shape == (2, 3, N + 1)  # the handle still works
        sk = SecretKey.new(p, 61)
        e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=64)
        assert e.batch_trlwe_matmul(w, trlwe).shape == (2, 3, p.n + 1)
    finally:
        e.close()


def test_one_neuron_end_to_end_dense_and_packed():
    """y = f(W x + b) on SECURITY_UINT4, m = 16: 8 inputs in {0, 1} per group, 4 groups, non-negative weights with every
    row sum plus bias at most 15 (the sum stays in the table's non-negacyclic half).  The input noise (sigma 2.5e-6)
    grows by at most sqrt(8 * 15^2) ~ 42 against a decoding margin of 1/64: every one of the 32 outputs decodes."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.lut import Generator
    from rs_tfhe_amd.params import SECURITY_UINT4 as p

    m, groups, k = 16, 4, 8
    rng = np.random.default_rng(71)
    w = np.stack([rng.multinomial(12, np.full(k, 1.0 / k)) for _ in range(k)]).astype(np.int8)
    b = rng.integers(0, 4, k)
    assert w.min() >= 0 and (w.sum(axis=1) + b).max() <= m - 1
    x = rng.integers(0, 2, (groups, k))
    x[0], x[1] = 1, 0  # every input set, none set
    pre = x @ w.T.astype(np.int64) + b
    assert pre.max() <= m - 1
    f = lambda v: (3 * v + 1) % m  # noqa: E731
    want = f(pre).reshape(-1)
    bias = (b.astype(np.uint32) << np.uint32(32 - 5))  # b / (2 m) on the torus, m = 16
    tv = Generator(m).generate_lookup_table(f).poly
    sk = SecretKey.new(p, 72)
    e = R.Engine(p, 0)
    try:
        e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=73)
        cts = sk.encrypt_lwe_message(x.reshape(-1), m, seed=74).reshape(groups, k, p.n + 1)
        lin = e.batch_tlwe_matmul(w, cts, bias)
        assert np.array_equal(sk.decrypt_lwe_message(lin.reshape(-1, p.n + 1), m), pre.reshape(-1))  # (pre < m: no wrap)
        out = e.batch_bootstrap(lin.reshape(-1, p.n + 1), tv)
        assert np.array_equal(sk.decrypt_lwe_message(out, m), want)
        slots = np.zeros((groups, N), np.int64)
        slots[:, :k] = x
        packed = sk.encrypt_packed_lwe_message(slots.reshape(-1), m, seed=75)
        lin = e.batch_trlwe_matmul(w, packed, bias, keyswitch=True)
        out = e.batch_bootstrap(lin.reshape(-1, p.n + 1), tv)
        assert np.array_equal(sk.decrypt_lwe_message(out, m), want)
    finally:
        e.close()


def test_cpp_mirror_matmul(O):
    """tests/cpp/test_matmul.cpp: linear::matmul and linear::matmul_packed against the oracle library."""
    import tempfile

    from test_matmul_host import build_cpp_matmul

    with tempfile.TemporaryDirectory() as d:
        exe = build_cpp_matmul(d)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test_matmul ok" in r.stdout
