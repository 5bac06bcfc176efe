"""Encrypted 2-D convolution on the GPU: tfhe_hip_batch_tlwe_conv2d equals linear.conv2d_model word for word
(np.array_equal, no tolerance: integer arithmetic) on every path of the loader -- one tap per fetch (in_c % 16 == 0),
taps and the end of K crossing inside a fetch, padding on every side, strides, a second row block --, padding reads zero
and not a neighbouring row or image, a 1 x 1 filter is the dense form, the _dev form gives the host form's bits on a side
stream, the launch seam inside one image, the error codes, one layer end to end into a programmable bootstrap, and the
C++ mirror."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDGES = (0, 0x80000000, 0xFFFFFFFF, 0x7F7F7F7F, 0x80808080, 0x00800080, 0x7FFFFFFF)  # carries between balanced byte planes
# (in_h, in_w, in_c, out_c, k_h, k_w, stride, padding), 2 groups each
LOADER_CASES = (
    (5, 5, 16, 3, 3, 3, (1, 1), (1, 1)),    # one tap per fetch; padding taps on every side
    (5, 5, 3, 3, 3, 3, (1, 1), (1, 1)),     # K = 27 < 32: taps cross inside the one fetch, which also ends K
    (5, 5, 20, 3, 3, 3, (1, 1), (1, 1)),    # K = 180: a K-step boundary inside a tap
    (5, 5, 32, 3, 1, 3, (1, 1), (0, 1)),    # 1 x 3
    (5, 5, 32, 3, 3, 1, (1, 1), (1, 0)),    # 3 x 1
    (7, 8, 5, 4, 3, 2, (2, 3), (0, 0)),     # strides
    (7, 8, 16, 4, 3, 2, (2, 3), (0, 0)),
    (2, 2, 16, 3, 3, 3, (1, 1), (2, 2)),    # pad = k - 1: most taps are padding
    (2, 2, 2, 3, 3, 3, (1, 1), (2, 2)),
    (3, 3, 16, 65, 3, 3, (1, 1), (1, 1)),   # a second row block with a one-row tail
)
_CACHE = {}


def weights(rng, shape):
    """Random in [-128, 127]; the first filters all -128, all 127, all 0."""
    w = rng.integers(-128, 128, shape).astype(np.int8)
    for r, v in zip(range(shape[0]), (-128, 127, 0)):
        w[r] = v
    return w


def plant(cts):
    """Into [groups][in_h][in_w][in_c][width] words: 0xFFFFFFFF / 0x80000000 alternating over the leading and trailing
    words of every border pixel, and on the first and last word of the first and last channel of every pixel -- a tap
    that wraps into the adjacent row or image instead of reading zero meets the largest words there are --; then the
    carry patterns between byte planes down the first and last word of the first ciphertexts of each group and along
    the first and the last ciphertext's words."""
    groups, in_h, in_w, in_c, width = cts.shape
    big = np.array([0xFFFFFFFF, 0x80000000] * 4, np.uint32)
    for iy in range(in_h):
        for ix in range(in_w):
            if iy in (0, in_h - 1) or ix in (0, in_w - 1):
                cts[:, iy, ix, :, :8] = big
                cts[:, iy, ix, :, -8:] = big[::-1]
    cts[:, :, :, 0, 0], cts[:, :, :, 0, -1] = 0xFFFFFFFF, 0x80000000
    cts[:, :, :, -1, 0], cts[:, :, :, -1, -1] = 0x80000000, 0xFFFFFFFF
    flat = cts.reshape(groups, -1, width)  # (a view: cts is contiguous)
    k = min(len(EDGES), flat.shape[1])
    flat[:, :k, 0] = EDGES[:k]
    flat[:, :k, -1] = EDGES[:k]
    flat[:, 0, 1:1 + len(EDGES)] = EDGES
    flat[:, -1, -1 - len(EDGES):-1] = EDGES
    return cts


def case(p, geom, groups, seed):
    """(w, bias, cts, stride, padding, the model's words), made once per (set, geometry, seed)."""
    key = (p.name, geom, groups, seed)
    if key not in _CACHE:
        from rs_tfhe_amd import linear as L

        in_h, in_w, in_c, out_c, k_h, k_w, stride, padding = geom
        rng = np.random.default_rng(seed)
        w = weights(rng, (out_c, k_h, k_w, in_c))
        bias = rng.integers(0, 1 << 32, out_c, dtype=np.uint32)
        cts = plant(rng.integers(0, 1 << 32, (groups, in_h, in_w, in_c, p.n + 1), dtype=np.uint32))
        _CACHE[key] = (w, bias, cts, stride, padding, L.conv2d_model(p, w, cts, bias, stride, padding))
    return _CACHE[key]


@pytest.mark.parametrize("name", ["SECURITY_80_BIT", "SECURITY_128_BIT", "SECURITY_UINT8"])
def test_every_path_of_the_loader_equals_the_model(name):
    import rs_tfhe_amd as R
    from rs_tfhe_amd import linear as L
    from rs_tfhe_amd.params import PARAM_SETS

    p = PARAM_SETS[name]
    assert p.n + 1 == {"SECURITY_80_BIT": 551, "SECURITY_128_BIT": 701, "SECURITY_UINT8": 1161}[name]
    e = R.Engine(p, 0)  # no key: the convolution needs none
    try:
        for i, geom in enumerate(LOADER_CASES):
            w, bias, cts, stride, padding, want = case(p, geom, 2, 100 + i)
            got = e.batch_tlwe_conv2d(w, cts, bias, stride, padding)
            assert got.shape == want.shape and got.dtype == np.uint32, geom
            assert np.array_equal(got, want), geom
        w, bias, cts, stride, padding, want = case(p, LOADER_CASES[2], 2, 102)
        assert np.array_equal(e.batch_tlwe_conv2d(w, cts, None, stride, padding), L.conv2d_model(p, w, cts, None, stride, padding))
        assert np.array_equal(e.batch_tlwe_conv2d(w, cts[1], bias, stride, padding), want[1:])  # four axes: one group
        assert e.batch_tlwe_conv2d(w, cts[:0], bias, stride, padding).shape == (0,) + want.shape[1:]  # groups == 0
    finally:
        e.close()


def test_padding_reads_zero_not_a_neighbour():
    """Two 3 x 4 images back to back with the largest words on their borders and channel ends, filters of all 127, all
    -128 and random: a tap that stepped into the next row, the next image or the previous one instead of the padding
    would add a word of magnitude 2^31 times 127.  The model with wrap-around padding differs from the definition on
    this input at every border position, so the comparison can tell."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import linear as L
    from rs_tfhe_amd.params import SECURITY_80_BIT as p

    e = R.Engine(p, 0)
    try:
        for in_c, k, pad in ((1, 3, 1), (16, 3, 1), (3, 3, 2), (16, 2, 1), (17, 3, 1)):
            geom = (3, 4, in_c, 4, k, k, (1, 1), (pad, pad))
            w, bias, cts, stride, padding, want = case(p, geom, 2, 200 + in_c)
            got = e.batch_tlwe_conv2d(w, cts, bias, stride, padding)
            assert np.array_equal(got, want), geom
            # what a loader that read the neighbouring ciphertext in memory would have computed
            flat = cts.reshape(-1, in_c, p.n + 1)
            ring = np.concatenate([flat[-16:], flat, flat[:16]])  # the memory around every image, cyclically
            wrong = np.zeros_like(want)
            out_h, out_w = want.shape[1:3]
            for g in range(2):
                for oy in range(out_h):
                    for ox in range(out_w):
                        rows = [ring[16 + (g * 3 + oy + ky - pad) * 4 + ox + kx - pad] for ky in range(k) for kx in range(k)]
                        wrong[g, oy, ox] = L.matmul_model(p, w.reshape(4, -1), np.concatenate(rows)[None], bias)[0]
            interior = np.zeros((out_h, out_w), bool)
            interior[pad:3 - k + 1 + pad, pad:4 - k + 1 + pad] = True
            assert np.array_equal(wrong[:, interior], want[:, interior])
            differs = (wrong != want).any(axis=(0, 3, 4))
            assert differs[~interior].all(), geom
    finally:
        e.close()


def test_one_by_one_filter_is_the_dense_form_on_the_same_memory():
    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    w, bias, cts, _, _, want = case(p, (3, 4, 20, 5, 1, 1, (1, 1), (0, 0)), 2, 300)
    e = R.Engine(p, 0)
    try:
        conv = e.batch_tlwe_conv2d(w, cts, bias)
        dense = e.batch_tlwe_matmul(w.reshape(5, 20), cts.reshape(2 * 3 * 4, 20, p.n + 1), bias)
        assert np.array_equal(conv.reshape(dense.shape), dense)
        assert np.array_equal(conv, want)
    finally:
        e.close()


def test_dev_form_gives_the_host_forms_bits():
    """torch tensors on a side stream, weights and bias on the device included; K = 27 and 180 put the device rows of w
    off 16-byte boundaries."""
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    e = R.Engine(p, 0)
    try:
        side = torch.cuda.Stream(device=0)

        def dev(a):
            return torch.from_numpy(a.view(np.int8 if a.dtype == np.int8 else np.int32)).to("cuda:0")

        for i in (0, 1, 2, 5):
            w, bias, cts, stride, padding, want = case(p, LOADER_CASES[i], 2, 100 + i)
            host = e.batch_tlwe_conv2d(w, cts, bias, stride, padding)
            assert np.array_equal(host, want)
            tw, tb, tin = dev(w), dev(bias), dev(cts)
            out = torch.full(want.shape, -1, dtype=torch.int32, device="cuda:0")
            side.wait_stream(torch.cuda.current_stream(0))
            e.batch_tlwe_conv2d_dev(tw, tin, out, bias=tb, stride=stride, padding=padding, stream=side)
            side.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), host), LOADER_CASES[i]
        out = torch.full(want.shape, -1, dtype=torch.int32, device="cuda:0")
        e.batch_tlwe_conv2d_dev(tw, tin, out, stride=stride, padding=padding)  # bias None, torch's current stream
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), e.batch_tlwe_conv2d(w, cts, None, stride, padding))
    finally:
        e.close()


def test_launch_seam_inside_one_image():
    """2^19 + 5 = 7 * 74,899 output positions of ONE image, one channel in and out, a 1 x 1 filter: the second launch
    starts at position 2^19, in the last row of the image.  1.2 GB in, 1.2 GB out, made and checked on the device:
    out = w * in (+ bias on the last word) in wrapping int32 arithmetic."""
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import SECURITY_80_BIT as p

    in_h, in_w, seam = 7, 74899, 1 << 19
    assert in_h * in_w == seam + 5
    width = p.n + 1
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    tin = torch.randint(-(1 << 31), 1 << 31, (1, in_h, in_w, 1, width), dtype=torch.int32, device="cuda:0", generator=gen)
    weight, bias = -77, 0x1ABCDEF0
    tw = torch.tensor([[[[weight]]]], dtype=torch.int8, device="cuda:0")
    tb = torch.tensor([bias], dtype=torch.int32, device="cuda:0")
    out = torch.full((1, in_h, in_w, 1, width), -1, dtype=torch.int32, device="cuda:0")
    e = R.Engine(p, 0)
    try:
        e.batch_tlwe_conv2d_dev(tw, tin, out, bias=tb)
        torch.cuda.synchronize()
    finally:
        e.close()
    want = tin * weight  # int32: wraps
    want[..., -1] += bias
    flat_out, flat_want = out.view(-1, width), want.view(-1, width)
    for pos in (0, seam - 2, seam - 1, seam, seam + 1, seam + 4):
        assert torch.equal(flat_out[pos], flat_want[pos]), pos
    assert torch.equal(out, want)


def test_conv2d_error_codes():
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi
    from rs_tfhe_amd.params import SECURITY_80_BIT as p

    lib = _capi.lib()
    C = _capi.C
    vp = C.c_void_p
    fields = ("in_h", "in_w", "in_c", "out_c", "k_h", "k_w", "stride_h", "stride_w", "pad_h", "pad_w")
    good = dict(zip(fields, (5, 5, 4, 3, 3, 3, 1, 1, 1, 1)))

    def shape(**kw):
        return C.pointer(_capi.Conv2dShape(**dict(good, **kw)))

    w = np.ones((3, 3, 3, 4), np.int8)
    cts = np.zeros((2, 5, 5, 4, p.n + 1), np.uint32)
    out = np.zeros((2, 5, 5, 3, p.n + 1), np.uint32)
    wp, ip, op = (a.ctypes.data_as(vp) for a in (w, cts, out))
    e = R.Engine(p, 0)
    try:
        host, dev = lib.tfhe_hip_batch_tlwe_conv2d, lib.tfhe_hip_batch_tlwe_conv2d_dev
        bad = [(None, wp, None, ip, 2, op)]                                                  # NULL shape
        bad += [(shape(**{f: 0}), wp, None, ip, 2, op) for f in fields[:8]]                  # a zero dimension or stride
        bad += [(shape(k_h=8), wp, None, ip, 2, op), (shape(k_w=8), wp, None, ip, 2, op),    # filter > padded map
                (shape(pad_h=(1 << 31) - 3), wp, None, ip, 2, op),                           # in_h + 2 pad_h > 2^31 - 1
                (shape(pad_w=(1 << 32) - 1), wp, None, ip, 2, op),
                (shape(in_c=65536 // 9 + 1), wp, None, ip, 2, op),                           # K = 65,538
                (shape(in_h=300, in_w=300, k_h=257, k_w=256, in_c=1), wp, None, ip, 2, op),  # K = 65,792
                (shape(), None, None, ip, 2, op), (shape(), wp, None, None, 2, op), (shape(), wp, None, ip, 2, None),  # NULL w, in, out
                (shape(), wp, None, ip, (1 << 31) // 75 + 1, op),                            # groups * 5 * 5 * 3 > 2^31 - 1
                (shape(out_c=1 << 31), wp, None, ip, 1, op),
                (shape(stride_h=5, stride_w=5, pad_h=0, pad_w=0, out_c=1), wp, None, ip, (1 << 31) // 100 + 1, op),  # the input side
                (shape(), wp, None, ip, 1 << 62, op)]                                        # groups * out_h * out_w wraps
        for args in bad:
            assert host(e._ctx, *args) == _capi.EINVAL, args
            assert dev(e._ctx, *args, None) == _capi.EINVAL, args
        assert host(e._ctx, shape(), None, None, None, 0, None) == _capi.OK  # groups == 0 writes nothing
        assert dev(e._ctx, shape(), None, None, None, 0, None, None) == _capi.OK
        assert host(e._ctx, shape(stride_h=0), None, None, None, 0, None) == _capi.EINVAL  # the shape comes first
        assert host(e._ctx, None, None, None, None, 0, None) == _capi.EINVAL
        assert host(None, shape(), wp, None, ip, 2, op) == _capi.EINVAL
        assert not out.any()
        with pytest.raises(_capi.TfheHipError) as ei:
            e._call("batch_tlwe_conv2d", shape(k_h=8), wp, None, ip, 2, op)
        assert ei.value.code == _capi.EINVAL and "filter" in str(ei.value)
        # the largest stride there is: one output position; and the handle still works
        assert host(e._ctx, shape(stride_h=(1 << 32) - 1, stride_w=(1 << 32) - 1), wp, None, ip, 2, op) == _capi.OK
        assert (out[:, 0, 0].reshape(-1) == 0).all()
        got = e.batch_tlwe_conv2d(w, cts + np.uint32(1), padding=1)
        assert got.shape == (2, 5, 5, 3, p.n + 1) and got[0, 0, 0, 0, 0] == 16 and got[1, 2, 2, 2, -1] == 36
    finally:
        e.close()


def test_one_convolutional_layer_end_to_end():
    """y = min(conv(x) + b, 3) on SECURITY_UINT4, m = 16: a 4 x 4 single-channel image of messages in {0, 1, 2}, one
    2 x 2 filter with weights in {0, 1}, stride 1, bias 1: every sum is at most 3 * 2 + 1 = 7 < 16 (the table's
    non-negacyclic half).  The input noise (sigma 2.5e-6) grows by at most sqrt(3) against a decoding margin of 1/64."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.lut import Generator
    from rs_tfhe_amd.params import SECURITY_UINT4 as p

    m, b = 16, 1
    img = np.array([[0, 1, 2, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 2, 2, 2]])
    k = np.array([[1, 0], [1, 1]])
    pre = np.array([[(img[oy:oy + 2, ox:ox + 2] * k).sum() + b for ox in range(3)] for oy in range(3)])
    assert pre.min() < 3 < pre.max() <= m - 1
    f = lambda v: min(v, 3)  # noqa: E731
    want = np.minimum(pre, 3).reshape(-1)
    bias = np.array([b], np.uint32) << np.uint32(32 - 5)  # b / (2 m) on the torus, m = 16
    tv = Generator(m).generate_lookup_table(f).poly
    sk = SecretKey.new(p, 81)
    e = R.Engine(p, 0)
    try:
        e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=82)
        cts = sk.encrypt_lwe_message(img.reshape(-1), m, seed=83).reshape(1, 4, 4, 1, p.n + 1)
        lin = e.batch_tlwe_conv2d(k.reshape(1, 2, 2, 1).astype(np.int8), cts, bias)
        assert lin.shape == (1, 3, 3, 1, p.n + 1)
        assert np.array_equal(sk.decrypt_lwe_message(lin.reshape(-1, p.n + 1), m), pre.reshape(-1))  # (pre < m: no wrap)
        out = e.batch_bootstrap(lin.reshape(-1, p.n + 1), tv)
        assert np.array_equal(sk.decrypt_lwe_message(out, m), want)
    finally:
        e.close()


def test_cpp_mirror_conv2d():
    """tests/cpp/test_conv2d.cpp: linear::conv2d against the definition's loops, and the refused shapes."""
    import tempfile

    from test_conv2d_host import build_cpp_conv2d

    with tempfile.TemporaryDirectory() as d:
        exe = build_cpp_conv2d(d)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test_conv2d ok" in r.stdout
