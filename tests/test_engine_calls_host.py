"""Engine (one context) and Pool (several) forward every batch call they share to the same C entry point -- prefixed
`tfhe_hip_` or `tfhe_hip_pool_` -- with the same arguments, and refuse the same malformed operands before anything
reaches the library.  No GPU and no library: the objects are built around a stand-in that records each call."""
import ctypes as C
import types

import numpy as np
import pytest

from rs_tfhe_amd import engine as E
from rs_tfhe_amd.params import N

P = types.SimpleNamespace(n=4, l=2, iks_t=2, base=4, alpha_lv0=1.5e-5, alpha_lv1=2.5e-8)  # small n: small arrays
W = P.n + 1  # words of one ciphertext
HANDLE = 0x5A5A0  # the context / pool handle (a plain value)
ENGINE_DEV, POOL_DEVS = 3, [5, 6]  # the engine's GPU; the pool members' GPUs
M32 = 0xFFFFFFFF


class _Lib:
    """Records (symbol, arguments) of every call and returns 0 (TFHE_HIP_OK); `hooks[symbol](args)` runs first."""

    def __init__(self):
        self.calls, self.hooks = [], {}

    def __getattr__(self, name):
        if not name.startswith("tfhe_hip_"):
            raise AttributeError(name)

        def fn(*args):
            if name in self.hooks:
                self.hooks[name](args)
            self.calls.append((name, tuple(_norm(x) for x in args)))
            return 0

        return fn


def _norm(x):
    if isinstance(x, C._SimpleCData):
        return x.value
    if type(x).__name__ == "CArgObject":  # C.byref(...)
        return "byref"
    return x


def _engine():
    e = E.Engine.__new__(E.Engine)
    e.params, e.device, e._lib, e._ctx = P, ENGINE_DEV, _Lib(), C.c_void_p(HANDLE)
    e._owner, e._parent, e._views, e._key = None, None, [], None
    return e


def _pool():
    p = E.Pool.__new__(E.Pool)
    p.params, p.devices, p._lib, p._h, p.home = P, list(POOL_DEVS), _Lib(), C.c_void_p(HANDLE), 0
    p._parent, p._views = None, []
    return p


@pytest.fixture(params=["engine", "pool"])
def obj(request):
    return _engine() if request.param == "engine" else _pool()


def _is_pool(o):
    return isinstance(o, E.Pool)


def _sym(o, name):
    return ("tfhe_hip_pool_" if _is_pool(o) else "tfhe_hip_") + name


def _lead(o, home=0):
    """Arguments ahead of a *_dev call's own: the handle, and on a pool the home member."""
    return (HANDLE, home) if _is_pool(o) else (HANDLE,)


def _one_call(o):
    assert len(o._lib.calls) == 1, o._lib.calls
    return o._lib.calls[0]


def _refuses(o, fn, *args, **kw):
    with pytest.raises(ValueError):
        fn(*args, **kw)
    assert o._lib.calls == []


def _cts(count, seed=0):
    return np.random.default_rng(seed).integers(0, 2**32, (count, W), dtype=np.uint32)


def _p(a):
    return a.ctypes.data


# -- device-side stand-ins -------------------------------------------------------------------------------------------
class _Dev:
    def __init__(self, index):
        self.index = index

    def __str__(self):
        return f"cuda:{self.index}"


class _T:
    """What _tptr, _dev_batch and the *_dev checks read of a torch CUDA tensor."""

    _next = 0x10000

    def __init__(self, shape, device, itemsize=4, contiguous=True, cuda=True):
        self.shape, self.device, self.is_cuda = tuple(shape), _Dev(device), cuda
        self._isz, self._contig = itemsize, contiguous
        _T._next += 0x1000
        self._ptr = _T._next

    def is_contiguous(self):
        return self._contig

    def element_size(self):
        return self._isz

    def data_ptr(self):
        return self._ptr

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))


class _S:
    def __init__(self, device, handle=0x777):
        self.device, self.cuda_stream = _Dev(device), handle


def _dev(o, home=0):
    return POOL_DEVS[home] if _is_pool(o) else ENGINE_DEV


def _home_kw(o, home):
    return {"home": home} if home else {}


# ==== host arrays ======================================================================================================
def test_batch_gate(obj):
    a, b = _cts(5, 1), _cts(5, 2)
    out = obj.batch_gate(3, a, b)
    assert _one_call(obj) == (_sym(obj, "batch_gate"), (HANDLE, 3, _p(a), _p(b), _p(out), 5))
    obj._lib.calls.clear()
    out = obj.batch_gate(0, a)  # b=None: a NULL second operand (COPY / NOT style gates)
    assert _one_call(obj) == (_sym(obj, "batch_gate"), (HANDLE, 0, _p(a), None, _p(out), 5))
    obj._lib.calls.clear()
    mine = np.empty_like(a)
    assert obj.batch_gate(1, a, b, out=mine) is mine
    assert _one_call(obj) == (_sym(obj, "batch_gate"), (HANDLE, 1, _p(a), _p(b), _p(mine), 5))


def test_batch_gate_refusals(obj):
    a = _cts(5)
    _refuses(obj, obj.batch_gate, 0, a, _cts(4))
    _refuses(obj, obj.batch_gate, 0, a, a, out=np.empty((4, W), np.uint32))
    _refuses(obj, obj.batch_gate, 0, a, a, out=np.empty((5, W), np.int64))


def test_batch_gates_mixed(obj):
    a, b = _cts(4, 1), _cts(4, 2)
    g = np.array([0, 1, 2, 3], np.uint8)
    out = obj.batch_gates_mixed(g, a, b)
    assert _one_call(obj) == (_sym(obj, "batch_gates_mixed"), (HANDLE, _p(g), _p(a), _p(b), _p(out), 4))
    obj._lib.calls.clear()
    out = obj.batch_gates_mixed(g, a, b, keyswitch=False)
    assert _one_call(obj) == (_sym(obj, "batch_gates_mixed_nks"), (HANDLE, _p(g), _p(a), _p(b), _p(out), 4))


def test_batch_gates_mixed_refusals(obj):
    a = _cts(4)
    _refuses(obj, obj.batch_gates_mixed, np.zeros(3, np.uint8), a, a)
    _refuses(obj, obj.batch_gates_mixed, np.zeros(4, np.uint8), a, _cts(3))


def test_batch_bootstrap(obj):
    cts = _cts(3)
    out = obj.batch_bootstrap(cts)
    assert _one_call(obj) == (_sym(obj, "batch_bootstrap"), (HANDLE, _p(cts), None, 0, 1, _p(out), 3))
    obj._lib.calls.clear()
    tv = np.zeros((2, N), np.uint32)
    out = obj.batch_bootstrap(cts, tv, keyswitch=False)
    assert _one_call(obj) == (_sym(obj, "batch_bootstrap"), (HANDLE, _p(cts), _p(tv), 0, 0, _p(out), 3))
    obj._lib.calls.clear()
    tvs = np.zeros((3, 2, N), np.uint32)  # one table per ciphertext
    out = obj.batch_bootstrap(cts, tvs)
    assert _one_call(obj) == (_sym(obj, "batch_bootstrap"), (HANDLE, _p(cts), _p(tvs), 1, 1, _p(out), 3))


def test_batch_bootstrap_refusals(obj):
    cts = _cts(3)
    _refuses(obj, obj.batch_bootstrap, cts, np.zeros((2, N - 1), np.uint32))
    _refuses(obj, obj.batch_bootstrap, cts, np.zeros((2, 2, N), np.uint32))


def test_batch_tlwe_lincomb(obj):
    a, b = _cts(4, 1), _cts(4, 2)
    out = obj.batch_tlwe_lincomb(2, a)
    assert _one_call(obj) == (_sym(obj, "batch_tlwe_lincomb"), (HANDLE, 2, _p(a), 0, None, 0, _p(out), 4))
    obj._lib.calls.clear()
    out = obj.batch_tlwe_lincomb(-1, a, -3, b, -(1 << 29))  # negative coefficients: masked to u32
    assert _one_call(obj) == (_sym(obj, "batch_tlwe_lincomb"),
                              (HANDLE, M32, _p(a), (-3) & M32, _p(b), (-(1 << 29)) & M32, _p(out), 4))


def test_batch_tlwe_lincomb_refusals(obj):
    a = _cts(4)
    _refuses(obj, obj.batch_tlwe_lincomb, 1, a, 1)
    _refuses(obj, obj.batch_tlwe_lincomb, 1, a, 1, _cts(3))


def test_batch_lincomb_bootstrap(obj):
    a, b = _cts(3, 1), _cts(3, 2)
    out = obj.batch_lincomb_bootstrap(1, a)
    assert _one_call(obj) == (_sym(obj, "batch_lincomb_bootstrap"),
                              (HANDLE, 1, _p(a), 0, None, 0, None, 0, 1, _p(out), 3))
    obj._lib.calls.clear()
    tv = np.zeros((2, N), np.uint32)
    out = obj.batch_lincomb_bootstrap(-2, a, 5, b, -7, tv, keyswitch=False)
    assert _one_call(obj) == (_sym(obj, "batch_lincomb_bootstrap"),
                              (HANDLE, (-2) & M32, _p(a), 5, _p(b), (-7) & M32, _p(tv), 0, 0, _p(out), 3))
    obj._lib.calls.clear()
    tvs = np.zeros((3, 2, N), np.uint32)
    out = obj.batch_lincomb_bootstrap(1, a, 1, b, 0, tvs)
    assert _one_call(obj) == (_sym(obj, "batch_lincomb_bootstrap"),
                              (HANDLE, 1, _p(a), 1, _p(b), 0, _p(tvs), 1, 1, _p(out), 3))


def test_batch_lincomb_bootstrap_refusals(obj):
    a = _cts(3)
    _refuses(obj, obj.batch_lincomb_bootstrap, 1, a, 1)
    _refuses(obj, obj.batch_lincomb_bootstrap, 1, a, 1, _cts(2))
    _refuses(obj, obj.batch_lincomb_bootstrap, 1, a, 0, None, 0, np.zeros((2, N + 1), np.uint32))
    _refuses(obj, obj.batch_lincomb_bootstrap, 1, a, 0, None, 0, np.zeros((2, 2, N), np.uint32))


def test_batch_lincomb_bootstrap_many(obj):
    a, b = _cts(3, 1), _cts(3, 2)
    tv = np.zeros((2, N), np.uint32)
    out = obj.batch_lincomb_bootstrap_many(1, a, 1, b, 0, tv, n_luts=4)
    assert out.shape == (4, 3, W)
    assert _one_call(obj) == (_sym(obj, "batch_lincomb_bootstrap_many"),
                              (HANDLE, 1, _p(a), 1, _p(b), 0, _p(tv), 0, 4, 1, _p(out), 3))
    obj._lib.calls.clear()
    tvs = np.zeros((3, 2, N), np.uint32)
    out = obj.batch_lincomb_bootstrap_many(-1, a, 0, None, -5, tvs, keyswitch=False)
    assert out.shape == (2, 3, W)
    assert _one_call(obj) == (_sym(obj, "batch_lincomb_bootstrap_many"),
                              (HANDLE, M32, _p(a), 0, None, (-5) & M32, _p(tvs), 1, 2, 0, _p(out), 3))
    obj._lib.calls.clear()
    # what only the library checks (n_luts, a NULL table, a missing second operand) is forwarded as it is
    out = obj.batch_lincomb_bootstrap_many(1, a, 1, None, 0, None, n_luts=3)
    assert out.shape == (1,)
    assert _one_call(obj) == (_sym(obj, "batch_lincomb_bootstrap_many"),
                              (HANDLE, 1, _p(a), 1, None, 0, None, 0, 3, 1, _p(out), 3))


def test_batch_lincomb_bootstrap_many_refusals(obj):
    a, tv = _cts(3), np.zeros((2, N), np.uint32)
    _refuses(obj, obj.batch_lincomb_bootstrap_many, 1, a, 1, _cts(2), 0, tv)
    _refuses(obj, obj.batch_lincomb_bootstrap_many, 1, a, 0, None, 0, np.zeros(2 * N - 1, np.uint32))
    _refuses(obj, obj.batch_lincomb_bootstrap_many, 1, a, 0, None, 0, np.zeros((2, 2, N), np.uint32))


def test_batch_mux(obj):
    a, b, c = _cts(4, 1), _cts(4, 2), _cts(4, 3)
    out = obj.batch_mux(a, b, c, True)
    assert _one_call(obj) == (_sym(obj, "batch_mux"), (HANDLE, 1, _p(a), _p(b), _p(c), _p(out), 4))
    obj._lib.calls.clear()
    out = obj.batch_mux(a, b, c, naive=False)
    assert _one_call(obj) == (_sym(obj, "batch_mux"), (HANDLE, 0, _p(a), _p(b), _p(c), _p(out), 4))


def test_batch_mux_refusals(obj):
    a = _cts(4)
    _refuses(obj, obj.batch_mux, a, _cts(3), a, False)
    _refuses(obj, obj.batch_mux, a, a, _cts(3), False)


def test_batch_blind_rotate(obj):
    cts = _cts(3)
    out = obj.batch_blind_rotate(cts)
    assert out.shape == (3, 2, N)
    assert _one_call(obj) == (_sym(obj, "batch_blind_rotate"), (HANDLE, _p(cts), None, _p(out), 3))
    obj._lib.calls.clear()
    tv = np.zeros((2, N), np.uint32)
    out = obj.batch_blind_rotate(cts, tv)
    assert _one_call(obj) == (_sym(obj, "batch_blind_rotate"), (HANDLE, _p(cts), _p(tv), _p(out), 3))


def test_batch_blind_rotate_refusals(obj):
    """The library stages 2 * N words of the table: a shorter one is refused on both classes."""
    cts = _cts(3)
    _refuses(obj, obj.batch_blind_rotate, cts, np.zeros((2, N - 1), np.uint32))
    _refuses(obj, obj.batch_blind_rotate, cts, np.zeros((3, 2, N), np.uint32))


# ==== device tensors ===================================================================================================
def test_batch_gate_dev(obj):
    homes = (None, 1) if _is_pool(obj) else (None,)
    for home in homes:
        d = _dev(obj, home or 0)
        a, b, out = _T((6, W), d), _T((6, W), d), _T((6, W), d)
        obj._lib.calls.clear()
        obj.batch_gate_dev(4, a, b, out, _S(d, 0x99), **_home_kw(obj, home))
        assert _one_call(obj) == (_sym(obj, "batch_gate_dev"),
                                  _lead(obj, home or 0) + (4, a._ptr, b._ptr, out._ptr, 6, 0x99))
        obj._lib.calls.clear()
        obj.batch_gate_dev(0, a, None, out, _S(d, 0), **_home_kw(obj, home))  # b=None; torch's null stream is named explicitly
        assert _one_call(obj) == (_sym(obj, "batch_gate_dev"), _lead(obj, home or 0) + (0, a._ptr, None, out._ptr, 6, 1))


def test_dev_home_member(obj):
    """`home`: None is the default member (the Engine's only GPU); anything else names a pool member or is refused."""
    d = _dev(obj)
    a, out = _T((2, W), d), _T((2, W), d)
    if _is_pool(obj):
        _refuses(obj, obj.batch_gate_dev, 0, a, a, out, _S(d), home=2)
        _refuses(obj, obj.batch_gate_dev, 0, a, a, out, _S(d), home=-1)
        obj.home = 1  # the pool's default home moves the default device
        d1 = POOL_DEVS[1]
        a1, o1 = _T((2, W), d1), _T((2, W), d1)
        obj.batch_gate_dev(0, a1, a1, o1, _S(d1, 5))
        assert _one_call(obj) == (_sym(obj, "batch_gate_dev"), (HANDLE, 1, 0, a1._ptr, a1._ptr, o1._ptr, 2, 5))
    else:
        _refuses(obj, obj.batch_gate_dev, 0, a, a, out, _S(d), home=0)
        _refuses(obj, obj.batch_gate_dev, 0, a, a, out, _S(d), home=1)
        obj.batch_gate_dev(0, a, a, out, _S(d, 5), home=None)
        assert _one_call(obj) == (_sym(obj, "batch_gate_dev"), (HANDLE, 0, a._ptr, a._ptr, out._ptr, 2, 5))


def test_dev_tensor_refusals(obj):
    d, other = _dev(obj), 7
    ok = _T((4, W), d)
    _refuses(obj, obj.batch_gate_dev, 0, ok, _T((3, W), d), ok, _S(d))  # count differs
    _refuses(obj, obj.batch_gate_dev, 0, ok, _T((4, W + 1), d), ok, _S(d))  # width differs
    _refuses(obj, obj.batch_gate_dev, 0, ok, _T((4 * W,), d), ok, _S(d))  # not [count][n+1]
    _refuses(obj, obj.batch_gate_dev, 0, ok, _T((4, W), other), ok, _S(d))  # another GPU
    _refuses(obj, obj.batch_gate_dev, 0, ok, ok, _T((4, W), d, contiguous=False), _S(d))
    _refuses(obj, obj.batch_gate_dev, 0, ok, ok, _T((4, W), d, itemsize=8), _S(d))
    _refuses(obj, obj.batch_gate_dev, 0, ok, ok, _T((4, W), d, cuda=False), _S(d))
    _refuses(obj, obj.batch_gate_dev, 0, ok, ok, ok, _S(other))  # the stream of another GPU


def test_batch_gates_mixed_dev(obj):
    home = 1 if _is_pool(obj) else 0
    d = _dev(obj, home)
    g, a, b, out = _T((3,), d, itemsize=1), _T((3, W), d), _T((3, W), d), _T((3, W), d)
    obj.batch_gates_mixed_dev(g, a, b, out, _S(d, 0x42), **_home_kw(obj, home))
    assert _one_call(obj) == (_sym(obj, "batch_gates_mixed_dev"),
                              _lead(obj, home) + (g._ptr, a._ptr, b._ptr, out._ptr, 3, 0x42))
    obj._lib.calls.clear()
    obj.batch_gates_mixed_dev(g, a, b, out, _S(d, 0x42), keyswitch=False, **_home_kw(obj, home))
    assert _one_call(obj) == (_sym(obj, "batch_gates_mixed_nks_dev"),
                              _lead(obj, home) + (g._ptr, a._ptr, b._ptr, out._ptr, 3, 0x42))


def test_batch_gates_mixed_dev_refusals(obj):
    d = _dev(obj)
    a = _T((3, W), d)
    _refuses(obj, obj.batch_gates_mixed_dev, _T((3,), d, itemsize=4), a, a, a, _S(d))
    _refuses(obj, obj.batch_gates_mixed_dev, _T((3,), d, itemsize=1, contiguous=False), a, a, a, _S(d))
    _refuses(obj, obj.batch_gates_mixed_dev, _T((3,), d, itemsize=1, cuda=False), a, a, a, _S(d))
    _refuses(obj, obj.batch_gates_mixed_dev, _T((3,), 7, itemsize=1), a, a, a, _S(d))
    _refuses(obj, obj.batch_gates_mixed_dev, _T((2,), d, itemsize=1), a, a, a, _S(d))


def test_batch_bootstrap_dev(obj):
    home = 1 if _is_pool(obj) else 0
    d = _dev(obj, home)
    cts, out, s = _T((3, W), d), _T((3, W), d), _S(d, 0x31)
    obj.batch_bootstrap_dev(cts, out, stream=s, **_home_kw(obj, home))
    assert _one_call(obj) == (_sym(obj, "batch_bootstrap_dev"),
                              _lead(obj, home) + (cts._ptr, None, 0, 1, out._ptr, 3, 0x31))
    obj._lib.calls.clear()
    tv = _T((2, N), d)
    obj.batch_bootstrap_dev(cts, out, tv, keyswitch=False, stream=s, **_home_kw(obj, home))
    assert _one_call(obj) == (_sym(obj, "batch_bootstrap_dev"),
                              _lead(obj, home) + (cts._ptr, tv._ptr, 0, 0, out._ptr, 3, 0x31))
    obj._lib.calls.clear()
    tvs = _T((3, 2, N), d)
    obj.batch_bootstrap_dev(cts, out, tvs, per_ct=True, stream=s, **_home_kw(obj, home))
    assert _one_call(obj) == (_sym(obj, "batch_bootstrap_dev"),
                              _lead(obj, home) + (cts._ptr, tvs._ptr, 1, 1, out._ptr, 3, 0x31))


def test_batch_bootstrap_dev_refusals(obj):
    d = _dev(obj)
    cts = _T((3, W), d)
    _refuses(obj, obj.batch_bootstrap_dev, cts, cts, _T((2, N - 1), d), stream=_S(d))
    _refuses(obj, obj.batch_bootstrap_dev, cts, cts, _T((2, N), d), per_ct=True, stream=_S(d))
    _refuses(obj, obj.batch_bootstrap_dev, cts, cts, _T((2, N), 7), stream=_S(d))
    _refuses(obj, obj.batch_bootstrap_dev, cts, _T((2, W), d), stream=_S(d))


def test_batch_tlwe_lincomb_dev(obj):
    home = 1 if _is_pool(obj) else 0
    d = _dev(obj, home)
    a, b, out, s = _T((2, W), d), _T((2, W), d), _T((2, W), d), _S(d, 0x51)
    obj.batch_tlwe_lincomb_dev(-1, a, 2, b, -3, out, s, **_home_kw(obj, home))
    assert _one_call(obj) == (_sym(obj, "batch_tlwe_lincomb_dev"),
                              _lead(obj, home) + (M32, a._ptr, 2, b._ptr, (-3) & M32, out._ptr, 2, 0x51))
    obj._lib.calls.clear()
    obj.batch_tlwe_lincomb_dev(1, a, 0, None, 0, out, s, **_home_kw(obj, home))
    assert _one_call(obj) == (_sym(obj, "batch_tlwe_lincomb_dev"),
                              _lead(obj, home) + (1, a._ptr, 0, None, 0, out._ptr, 2, 0x51))


def test_batch_lincomb_bootstrap_dev(obj):
    home = 1 if _is_pool(obj) else 0
    d = _dev(obj, home)
    a, b, out, s = _T((2, W), d), _T((2, W), d), _T((2, W), d), _S(d, 0x61)
    obj.batch_lincomb_bootstrap_dev(1, a, 0, None, 0, out, stream=s, **_home_kw(obj, home))
    assert _one_call(obj) == (_sym(obj, "batch_lincomb_bootstrap_dev"),
                              _lead(obj, home) + (1, a._ptr, 0, None, 0, None, 0, 1, out._ptr, 2, 0x61))
    obj._lib.calls.clear()
    tvs = _T((2, 2, N), d)
    obj.batch_lincomb_bootstrap_dev(-4, a, 3, b, -9, out, tvs, per_ct=True, keyswitch=False, stream=s,
                                    **_home_kw(obj, home))
    assert _one_call(obj) == (_sym(obj, "batch_lincomb_bootstrap_dev"),
                              _lead(obj, home) + ((-4) & M32, a._ptr, 3, b._ptr, (-9) & M32, tvs._ptr, 1, 0, out._ptr,
                                                  2, 0x61))


def test_batch_lincomb_bootstrap_dev_refusals(obj):
    d = _dev(obj)
    a = _T((2, W), d)
    _refuses(obj, obj.batch_lincomb_bootstrap_dev, 1, a, 1, _T((3, W), d), 0, a, stream=_S(d))
    _refuses(obj, obj.batch_lincomb_bootstrap_dev, 1, a, 0, None, 0, a, _T((2, N + 1), d), stream=_S(d))
    _refuses(obj, obj.batch_lincomb_bootstrap_dev, 1, a, 0, None, 0, a, _T((2, N), d), per_ct=True, stream=_S(d))


def test_batch_lincomb_bootstrap_many_dev(obj):
    home = 1 if _is_pool(obj) else 0
    d = _dev(obj, home)
    a, b, s = _T((2, W), d), _T((2, W), d), _S(d, 0x71)
    tv, out = _T((2, N), d), _T((4, 2, W), d)
    obj.batch_lincomb_bootstrap_many_dev(1, a, -1, b, 0, out, tv, n_luts=4, stream=s, **_home_kw(obj, home))
    assert _one_call(obj) == (_sym(obj, "batch_lincomb_bootstrap_many_dev"),
                              _lead(obj, home) + (1, a._ptr, M32, b._ptr, 0, tv._ptr, 0, 4, 1, out._ptr, 2, 0x71))
    obj._lib.calls.clear()
    tvs, out2 = _T((2, 2, N), d), _T((2 * 2, W), d)
    obj.batch_lincomb_bootstrap_many_dev(1, a, 0, None, 5, out2, tvs, per_ct=True, keyswitch=False, stream=s,
                                         **_home_kw(obj, home))
    assert _one_call(obj) == (_sym(obj, "batch_lincomb_bootstrap_many_dev"),
                              _lead(obj, home) + (1, a._ptr, 0, None, 5, tvs._ptr, 1, 2, 0, out2._ptr, 2, 0x71))


def test_batch_lincomb_bootstrap_many_dev_refusals(obj):
    d = _dev(obj)
    a, tv = _T((2, W), d), _T((2, N), d)
    _refuses(obj, obj.batch_lincomb_bootstrap_many_dev, 1, a, 0, None, 0, None, tv, stream=_S(d))
    _refuses(obj, obj.batch_lincomb_bootstrap_many_dev, 1, a, 0, None, 0, _T((3, 2, W), d), tv, stream=_S(d))
    _refuses(obj, obj.batch_lincomb_bootstrap_many_dev, 1, a, 0, None, 0, _T((2, 2, W), 7), tv, stream=_S(d))
    _refuses(obj, obj.batch_lincomb_bootstrap_many_dev, 1, a, 0, None, 0, _T((2, 2, W), d), _T((2, N - 1), d),
             stream=_S(d))
    _refuses(obj, obj.batch_lincomb_bootstrap_many_dev, 1, a, 0, None, 0, _T((2, 2, W), d), tv, per_ct=True,
             stream=_S(d))
    _refuses(obj, obj.batch_lincomb_bootstrap_many_dev, 1, a, 1, _T((3, W), d), 0, _T((2, 2, W), d), tv, stream=_S(d))


def test_batch_mux_dev(obj):
    home = 1 if _is_pool(obj) else 0
    d = _dev(obj, home)
    a, b, c, out, s = _T((2, W), d), _T((2, W), d), _T((2, W), d), _T((2, W), d), _S(d, 0x81)
    for naive in (True, False):
        obj._lib.calls.clear()
        obj.batch_mux_dev(a, b, c, out, naive, s, **_home_kw(obj, home))
        assert _one_call(obj) == (_sym(obj, "batch_mux_dev"),
                                  _lead(obj, home) + (int(naive), a._ptr, b._ptr, c._ptr, out._ptr, 2, 0x81))


def test_batch_mux_dev_refusals(obj):
    d = _dev(obj)
    a = _T((2, W), d)
    _refuses(obj, obj.batch_mux_dev, a, a, _T((1, W), d), a, False, _S(d))
    _refuses(obj, obj.batch_mux_dev, a, a, a, _T((2, W), 7), False, _S(d))


def test_batch_blind_rotate_dev(obj):
    home = 1 if _is_pool(obj) else 0
    d = _dev(obj, home)
    cts, out, s = _T((3, W), d), _T((3, 2, N), d), _S(d, 0x91)
    obj.batch_blind_rotate_dev(cts, out, stream=s, **_home_kw(obj, home))
    assert _one_call(obj) == (_sym(obj, "batch_blind_rotate_dev"), _lead(obj, home) + (cts._ptr, None, out._ptr, 3, 0x91))
    obj._lib.calls.clear()
    tv = _T((2, N), d)
    obj.batch_blind_rotate_dev(cts, out, tv, s, **_home_kw(obj, home))
    assert _one_call(obj) == (_sym(obj, "batch_blind_rotate_dev"),
                              _lead(obj, home) + (cts._ptr, tv._ptr, out._ptr, 3, 0x91))


def test_batch_blind_rotate_dev_refusals(obj):
    d = _dev(obj)
    cts = _T((3, W), d)
    _refuses(obj, obj.batch_blind_rotate_dev, cts, _T((2, 2, N), d), stream=_S(d))
    _refuses(obj, obj.batch_blind_rotate_dev, cts, _T((3, 2, N), d), _T((2, N - 1), d), stream=_S(d))
    _refuses(obj, obj.batch_blind_rotate_dev, cts, _T((3, 2, N), 7), stream=_S(d))


# ==== the cloud key ====================================================================================================
def _cloud_key():
    return types.SimpleNamespace(
        bootstrapping_key=np.zeros((P.n, 2 * P.l, 2, N), np.float64),
        key_switching_key=np.zeros((N, P.iks_t, P.base, P.n + 1), np.uint32),
        blind_rotate_testvec=np.zeros((2, N), np.uint32), decomposition_offset=-5)


def test_load_cloud_key(obj):
    ck = _cloud_key()
    obj.load_cloud_key(ck)
    assert _one_call(obj) == (_sym(obj, "load_cloud_key"), (HANDLE, _p(ck.bootstrapping_key), _p(ck.key_switching_key),
                                                             (-5) & M32, _p(ck.blind_rotate_testvec)))


def test_load_cloud_key_refusals(obj):
    for field, bad in (("bootstrapping_key", np.zeros(7, np.float64)), ("key_switching_key", np.zeros(7, np.uint32)),
                       ("blind_rotate_testvec", np.zeros(2 * N + 1, np.uint32))):
        ck = _cloud_key()
        setattr(ck, field, bad)
        _refuses(obj, obj.load_cloud_key, ck)


def _compressed_key(seed=bytes(range(32))):
    return types.SimpleNamespace(
        bsk_bodies=np.zeros((P.n, 2 * P.l, N), np.uint32), ksk_bodies=np.zeros((N, P.iks_t, P.base), np.uint32),
        blind_rotate_testvec=np.zeros((2, N), np.uint32), mask_seed=seed, decomposition_offset=9)


def test_load_compressed_cloud_key(obj):
    ck, seen = _compressed_key(), {}
    obj._lib.hooks[_sym(obj, "load_compressed_cloud_key")] = lambda args: seen.setdefault("seed", C.string_at(args[1], 32))
    obj.load_compressed_cloud_key(ck)
    name, args = _one_call(obj)
    assert name == _sym(obj, "load_compressed_cloud_key") and seen["seed"] == bytes(range(32))
    assert args[0] == HANDLE and args[2:] == (_p(ck.bsk_bodies), _p(ck.ksk_bodies), 9, _p(ck.blind_rotate_testvec))


def test_load_compressed_cloud_key_refusals(obj):
    _refuses(obj, obj.load_compressed_cloud_key, _compressed_key(bytes(31)))
    for field in ("bsk_bodies", "ksk_bodies", "blind_rotate_testvec"):
        ck = _compressed_key()
        setattr(ck, field, np.zeros(5, np.uint32))
        _refuses(obj, obj.load_compressed_cloud_key, ck)


def _secret():
    return np.arange(P.n, dtype=np.uint32) & 1, np.arange(N, dtype=np.uint32) & 1


def test_gen_cloud_key(obj):
    k0, k1 = _secret()
    obj.gen_cloud_key(k0, k1)
    assert _one_call(obj) == (_sym(obj, "gen_cloud_key_secure"), (HANDLE, _p(k0), _p(k1), P.alpha_lv0, P.alpha_lv1))
    obj._lib.calls.clear()
    obj.gen_cloud_key(k0, k1, seed=-1)  # an integer seed: reproducible, 64 bits
    assert _one_call(obj) == (_sym(obj, "gen_cloud_key"),
                              (HANDLE, _p(k0), _p(k1), P.alpha_lv0, P.alpha_lv1, 0xFFFFFFFFFFFFFFFF))


def test_gen_cloud_key_alphas_and_generator_key(obj):
    """The caller's noise levels and 32-byte generator key reach a pool's entry points as they reach a context's."""
    k0, k1 = _secret()
    obj.gen_cloud_key(k0, k1, seed=7, alpha_ksk=0.25, alpha_bsk=0.125)
    assert _one_call(obj) == (_sym(obj, "gen_cloud_key"), (HANDLE, _p(k0), _p(k1), 0.25, 0.125, 7))
    obj._lib.calls.clear()
    obj.gen_cloud_key(k0, k1, alpha_bsk=0.5)
    assert _one_call(obj) == (_sym(obj, "gen_cloud_key_secure"), (HANDLE, _p(k0), _p(k1), P.alpha_lv0, 0.5))
    obj._lib.calls.clear()
    seen = {}
    obj._lib.hooks[_sym(obj, "gen_cloud_key_with_key")] = lambda args: seen.setdefault("key", C.string_at(args[-1], 32))
    obj.gen_cloud_key(k0, k1, rng_key=bytes(range(1, 33)))
    name, args = _one_call(obj)
    assert name == _sym(obj, "gen_cloud_key_with_key") and seen["key"] == bytes(range(1, 33))
    assert args[:-1] == (HANDLE, _p(k0), _p(k1), P.alpha_lv0, P.alpha_lv1)


def test_gen_cloud_key_refusals(obj):
    k0, k1 = _secret()
    _refuses(obj, obj.gen_cloud_key, k0[:-1], k1)
    _refuses(obj, obj.gen_cloud_key, k0, k1[:-1])


def test_gen_cloud_key_generator_key_refusals(obj):
    k0, k1 = _secret()
    _refuses(obj, obj.gen_cloud_key, k0, k1, rng_key=bytes(31))
    _refuses(obj, obj.gen_cloud_key, k0, k1, seed=1, rng_key=bytes(32))


def test_export_cloud_key(obj):
    def fill(args):
        args[-2]._obj.value = 77  # the decomposition offset the library writes

    obj._lib.hooks[_sym(obj, "export_cloud_key")] = fill
    ck = obj.export_cloud_key()
    name, args = _one_call(obj)
    member = (0,) if _is_pool(obj) else ()
    assert name == _sym(obj, "export_cloud_key")
    assert args == (HANDLE,) + member + (_p(ck.bootstrapping_key), _p(ck.key_switching_key), "byref",
                                         _p(ck.blind_rotate_testvec))
    assert ck.decomposition_offset == 77 and ck.bootstrapping_key.shape == (P.n, 2 * P.l, 2, N)
    if _is_pool(obj):
        obj._lib.calls.clear()
        ck = obj.export_cloud_key(1)
        assert _one_call(obj)[1][:2] == (HANDLE, 1)


def test_engine_dev_home_must_be_none():
    e = _engine()
    a = _T((2, W), ENGINE_DEV)
    for call in (lambda: e.batch_bootstrap_dev(a, a, stream=_S(ENGINE_DEV), home=0),
                 lambda: e.batch_mux_dev(a, a, a, a, False, _S(ENGINE_DEV), home=0),
                 lambda: e.batch_blind_rotate_dev(a, _T((2, 2, N), ENGINE_DEV), stream=_S(ENGINE_DEV), home=0)):
        _refuses(e, call)
