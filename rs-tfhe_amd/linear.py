"""Encrypted linear layers: y = W x + bias with a plaintext int8 matrix W and encrypted x ("encrypted linear layers",
include/tfhe_hip.h; csrc/matmul.hpp).

The inputs are LWE ciphertexts [groups][cols][n+1] (dense form) or the first `cols` slots of TRLWE lv1 ciphertexts
[groups][2][N] (packed form: what packing.pack wrote, or what a client encrypted with SecretKey.encrypt_packed_*).
Everything is integer arithmetic mod 2^32, so the numpy models here ARE the definition and the GPU equals them word for
word: the phase of output row r is sum_j w[r][j] * phase(input j) + bias[r] exactly, and the noise variance scales by
sum_j w[r][j]^2.  Under the (msg mod m) / (2m) encoding the messages add mod 2m on the torus: keep every row sum below m
when a programmable bootstrap follows, so that it stays in the table's non-negacyclic half.

The convolutional layer ("encrypted 2-D convolution" in the header) is the dense form over the taps of a filter:
conv2d_model is its definition, an explicit im2col into the same exact sum; conv2d is the server side.  Feature maps are
channels-last, [groups][in_h][in_w][in_c][n+1], on both sides of a layer.

The polynomial product ("plaintext polynomial products on packed ciphertexts" in the header) is the operation that keeps
a packed ciphertext packed: out(X) = sum_j w_j(X) * ct_j(X) + bias(X) mod X^N + 1, TRLWE in and TRLWE out.
polymul_model is its definition, polymul the server side, monomial the slot rotation +-X^k, and conv2d_packed_plan /
conv2d_packed_weights the encoding under which it is a convolution of a whole feature map held in ONE ciphertext.
"""
from __future__ import annotations

import numpy as np

from .params import N, SecurityParams

MAX_COLS = 65536  # dense form: each byte-plane accumulator of the kernel stays at or below cols * 2^14 <= 2^30


def _weights(w, bias, max_cols: int):
    """(w as [rows][cols] int64, bias as [rows] u32 or None) after the header's shape checks."""
    w = np.asarray(w)
    if w.ndim != 2 or w.shape[0] < 1 or not 1 <= w.shape[1] <= max_cols:
        raise ValueError(f"w must be [rows][cols] with rows >= 1 and 1 <= cols <= {max_cols}")
    if not np.issubdtype(w.dtype, np.integer) or w.min() < -128 or w.max() > 127:
        raise ValueError("weights must be integers in [-128, 127]")
    if bias is not None:
        bias = np.ascontiguousarray(bias, dtype=np.uint32).reshape(-1)
        if len(bias) != w.shape[0]:
            raise ValueError("bias must be [rows]")
    return w.astype(np.int64), bias


def _product(w, rows_in, bias) -> np.ndarray:
    """[groups][cols][width] u32 -> [groups][rows][width]: sum_j w[r][j] * in[g][j] mod 2^32, + bias on the last word.
    The words are split in 16-bit halves so that the int64 sums stay below 2^40."""
    x = rows_in.astype(np.int64)
    lo = np.matmul(w, x & 0xFFFF)
    hi = np.matmul(w, x >> 16)
    out = ((lo + (hi << 16)) & 0xFFFFFFFF).astype(np.uint32)
    if bias is not None:
        out[..., -1] += bias
    return out


def matmul_model(params: SecurityParams, w, cts, bias=None) -> np.ndarray:
    """The dense form's definition: w [rows][cols] int8, cts [groups][cols][width] (or [cols][width]: one group), bias
    [rows] torus words or None -> [groups][rows][width] u32.  width is n + 1 for lv0 ciphertexts; N + 1 (lv1 rows) is
    accepted too, which is how matmul_packed_model uses it."""
    w, bias = _weights(w, bias, MAX_COLS)
    cts = np.asarray(cts, np.uint32)
    if cts.ndim == 2:
        cts = cts[None]
    if cts.ndim != 3 or cts.shape[1] != w.shape[1] or cts.shape[2] not in (params.n + 1, N + 1):
        raise ValueError(f"cts must be [groups][{w.shape[1]}][{params.n + 1}]")
    return _product(w, cts, bias)


def extract_rows_exact(trlwe, slots) -> np.ndarray:
    """The lv1 extraction of slot s = G N + j for every s in `slots`, with the exact wrapping negation:
    r[i] = a_G[j - i] for i <= j, 0 - a_G[N + j - i] for i > j, r[N] = b_G[j]: [len(slots)][N+1] u32.
    (packing.extract_rows has the reference's Torus::MAX - a instead: one LSB lower in every negated word.)"""
    trlwe = np.asarray(trlwe, np.uint32).reshape(-1, 2, N)
    s = np.asarray(slots, np.int64).reshape(-1)
    if len(s) and (s.min() < 0 or s.max() >= len(trlwe) * N):
        raise ValueError("slot out of range")
    G, j = s // N, s % N
    i = np.arange(N)
    out = np.empty((len(s), N + 1), np.uint32)
    r = np.take_along_axis(trlwe[G, 0], (j[:, None] - i[None, :]) % N, axis=1)
    out[:, :N] = np.where(i[None, :] > j[:, None], np.uint32(0) - r, r)
    out[:, N] = trlwe[G, 1, j]
    return out


def matmul_packed_model(params: SecurityParams, w, trlwe, bias=None) -> np.ndarray:
    """The packed form's definition without the key switch: matmul_model on extract_rows_exact of slots 0 .. cols-1 of
    every group of trlwe [groups][2][N] -> [groups][rows][N+1] lv1 rows.  The key-switched result is
    packing.key_switch_model(params, ksk, rows) of these rows."""
    wi, bias = _weights(w, bias, N)
    trlwe = np.asarray(trlwe, np.uint32).reshape(-1, 2, N)
    cols = wi.shape[1]
    slots = (np.arange(len(trlwe))[:, None] * N + np.arange(cols)[None, :]).reshape(-1)
    return matmul_model(params, wi, extract_rows_exact(trlwe, slots).reshape(len(trlwe), cols, N + 1), bias)


def _pair(v, name: str, least: int):
    """stride / padding as (vertical, horizontal): an int for both or a pair, each at least `least`."""
    pair = (v, v) if isinstance(v, (int, np.integer)) else tuple(v) if isinstance(v, (tuple, list, np.ndarray)) else ()
    if len(pair) != 2 or any(not isinstance(x, (int, np.integer)) or x < least for x in pair):
        raise ValueError(f"{name} must be an int or a pair of ints, each at least {least}")
    return int(pair[0]), int(pair[1])


def conv2d_out_shape(in_h: int, in_w: int, k_h: int, k_w: int, stride=1, padding=0):
    """(out_h, out_w) = ((in_h + 2 pad_h - k_h) // stride_h + 1, likewise) of the header's definition; the filter must
    fit the padded map."""
    (sh, sw), (ph, pw) = _pair(stride, "stride", 1), _pair(padding, "padding", 0)
    if min(in_h, in_w, k_h, k_w) < 1 or k_h > in_h + 2 * ph or k_w > in_w + 2 * pw:
        raise ValueError("the filter must be at least 1 x 1 and no larger than the padded map")
    return (in_h + 2 * ph - k_h) // sh + 1, (in_w + 2 * pw - k_w) // sw + 1


def _filters(w, bias):
    """(w as [out_c][k_h][k_w][in_c] int64, bias as [out_c] u32 or None): _weights on the im2col matrix [out_c][K]."""
    w = np.asarray(w)
    if w.ndim != 4 or 0 in w.shape:
        raise ValueError("w must be [out_c][k_h][k_w][in_c] with every dimension at least 1")
    w2, bias = _weights(w.reshape(w.shape[0], -1), bias, MAX_COLS)
    return w2.reshape(w.shape), bias


def conv2d_model(params: SecurityParams, w, cts, bias=None, stride=1, padding=0) -> np.ndarray:
    """The convolution's definition ("encrypted 2-D convolution", include/tfhe_hip.h): w [out_c][k_h][k_w][in_c] int8,
    cts [groups][in_h][in_w][in_c][n+1] (or [in_h][in_w][in_c][n+1]: one group), bias [out_c] torus words or None ->
    [groups][out_h][out_w][out_c][n+1] u32.  An explicit im2col of the zero-padded map, one output row at a time, into
    _product: the same exact sum as the dense form."""
    w, bias = _filters(w, bias)
    out_c, k_h, k_w, in_c = w.shape
    cts = np.asarray(cts, np.uint32)
    if cts.ndim == 4:
        cts = cts[None]
    if cts.ndim != 5 or cts.shape[3] != in_c or cts.shape[4] != params.n + 1:
        raise ValueError(f"cts must be [groups][in_h][in_w][{in_c}][{params.n + 1}]")
    groups, in_h, in_w, _, width = cts.shape
    (sh, sw), (ph, pw) = _pair(stride, "stride", 1), _pair(padding, "padding", 0)
    out_h, out_w = conv2d_out_shape(in_h, in_w, k_h, k_w, (sh, sw), (ph, pw))
    padded = np.zeros((groups, in_h + 2 * ph, in_w + 2 * pw, in_c, width), np.uint32)
    padded[:, ph:ph + in_h, pw:pw + in_w] = cts
    ix = (np.arange(out_w) * sw)[:, None] + np.arange(k_w)[None, :]  # [out_w][k_w]
    w2 = w.reshape(out_c, k_h * k_w * in_c)
    out = np.empty((groups, out_h, out_w, out_c, width), np.uint32)
    for oy in range(out_h):
        rows = padded[:, oy * sh:oy * sh + k_h]                      # [groups][k_h][padded w][in_c][width]
        cols = rows[:, :, ix].transpose(0, 2, 1, 3, 4, 5)            # [groups][out_w][k_h][k_w][in_c][width]
        out[:, oy] = _product(w2, cols.reshape(groups, out_w, k_h * k_w * in_c, width), bias)
    return out


# ---- plaintext polynomial products on packed ciphertexts ("plaintext polynomial products", include/tfhe_hip.h) ----------
MAX_POLY_COLS = MAX_COLS // N  # K = cols * N weights per output word: the dense form's accumulator bound, cols <= 64


def _polys(w, bias):
    """(w as C-contiguous [rows][cols][N] int8, bias as [rows][N] u32 or None) after the header's shape checks; a single
    polynomial [N] is rows = cols = 1."""
    w = np.asarray(w)
    if w.ndim == 1:
        w = w[None, None]
    if w.ndim != 3 or w.shape[0] < 1 or not 1 <= w.shape[1] <= MAX_POLY_COLS or w.shape[2] != N:
        raise ValueError(f"w must be [rows][cols][{N}] with rows >= 1 and 1 <= cols <= {MAX_POLY_COLS}")
    if not np.issubdtype(w.dtype, np.integer) or w.min() < -128 or w.max() > 127:
        raise ValueError("weights must be integers in [-128, 127]")
    if bias is not None:
        bias = np.ascontiguousarray(bias, dtype=np.uint32)
        if bias.shape == (N,) and w.shape[0] == 1:
            bias = bias[None]
        if bias.shape != (w.shape[0], N):
            raise ValueError(f"bias must be [rows][{N}]")
    return np.ascontiguousarray(w, dtype=np.int8), bias


def _packed_inputs(trlwe, cols: int) -> np.ndarray:
    """trlwe as [groups][cols][2][N] u32.  Accepted besides: [cols][2][N] (one group) and, for cols == 1, what the
    packers and SecretKey.encrypt_packed_* return: [groups][2][N] or [2][N]."""
    t = np.ascontiguousarray(trlwe, dtype=np.uint32)
    if cols == 1 and t.ndim in (2, 3) and t.shape[-2:] == (2, N):
        t = t.reshape(-1, 1, 2, N)
    elif t.ndim == 3:
        t = t[None]
    if t.ndim != 4 or t.shape[1:] != (cols, 2, N):
        raise ValueError(f"trlwe must be [groups][{cols}][2][{N}]")
    return t


def polymul_model(w, trlwe, bias=None) -> np.ndarray:
    """The polynomial product's definition: w [rows][cols][N] int8 (or [N]), trlwe [groups][cols][2][N] (the forms of
    _packed_inputs), bias [rows][N] torus words or None -> [groups][rows][2][N] u32 with
    out[g][r](X) = sum_j w[r][j](X) * trlwe[g][j](X) mod X^N + 1 on both components, + bias[r](X) on b.  Exact: for each
    input polynomial the N rotated and sign-flipped rows X^m * p (row m holds ext_p[i - m], negated with the wrapping
    0 - p where it wrapped) are summed with the weights w[r][j][m].  The sums run as float64 matrix products over the
    16-bit halves of the words: N * 128 * 65,535 < 2^40, exact."""
    w8, bias = _polys(w, bias)
    rows, cols = w8.shape[:2]
    t = _packed_inputs(trlwe, cols)
    groups = len(t)
    out = np.zeros((groups, rows, 2, N), np.uint32)
    for j in range(cols):
        p = t[:, j]                                                        # [groups][2][N]
        ext = np.concatenate([np.uint32(0) - p, p], axis=-1)               # ext[t] at index t + N
        rot = np.lib.stride_tricks.sliding_window_view(ext, N, axis=-1)[:, :, N:0:-1]  # [groups][2][m][i] = ext[i - m]
        used = np.flatnonzero(w8[:, j].any(axis=0))                        # a monomial or a filter uses few of the N rows
        wj = w8[:, j, used].astype(np.float64)                             # [rows][m]
        for c in range(2):
            rc = rot[:, c][:, used]
            lo = np.matmul(wj, (rc & 0xFFFF).astype(np.float64)).astype(np.int64)
            hi = np.matmul(wj, (rc >> 16).astype(np.float64)).astype(np.int64)
            out[:, :, c] += ((lo + (hi << 16)) & 0xFFFFFFFF).astype(np.uint32)
    if bias is not None:
        out[:, :, 1] += bias
    return out


def monomial(k: int, sign: int = 1) -> np.ndarray:
    """The one-hot int8 polynomial sign * X^k, 0 <= k < N, sign +1 or -1: polymul with it rotates the slots, slot i
    moving to i + k and the slots that pass N coming back at the bottom negated (X^N = -1)."""
    if not isinstance(k, (int, np.integer)) or not 0 <= k < N or sign not in (1, -1):
        raise ValueError(f"monomial: 0 <= k < {N} and sign +1 or -1")
    w = np.zeros(N, np.int8)
    w[k] = sign
    return w


class PackedConvPlan:
    """The packed-convolution encoding of conv2d_packed_plan: where the client puts the map, where conv2d_packed_weights
    puts the filters, and `slots` [out_h][out_w] u32, the coefficients of the product that hold the outputs."""

    def __init__(self, in_c, in_h, in_w, k_h, k_w, stride):
        (sh, sw) = _pair(stride, "stride", 1)
        dims = (in_c, in_h, in_w, k_h, k_w)
        if any(not isinstance(x, (int, np.integer)) or x < 1 for x in dims) or k_h > in_h or k_w > in_w:
            raise ValueError("every dimension must be at least 1 and the filter no larger than the map")
        if in_c * in_h * in_w > N:
            raise ValueError(f"in_c * in_h * in_w = {in_c * in_h * in_w} values do not fit one ciphertext of {N} slots")
        self.in_c, self.in_h, self.in_w, self.k_h, self.k_w = (int(x) for x in dims)
        self.stride = (sh, sw)
        self.offset = (self.in_c - 1) * self.in_h * self.in_w + (self.k_h - 1) * self.in_w + (self.k_w - 1)
        self.out_h, self.out_w = (self.in_h - self.k_h) // sh + 1, (self.in_w - self.k_w) // sw + 1
        oy, ox = np.arange(self.out_h) * sh, np.arange(self.out_w) * sw
        self.slots = (self.offset + oy[:, None] * self.in_w + ox[None, :]).astype(np.uint32)

    def encode(self, fmap) -> np.ndarray:
        """A map [in_c][in_h][in_w] -> its N slot values (zeros above): value (c, y, x) at index c H W + y W + x."""
        fmap = np.asarray(fmap)
        if fmap.shape != (self.in_c, self.in_h, self.in_w):
            raise ValueError(f"the map must be [{self.in_c}][{self.in_h}][{self.in_w}]")
        out = np.zeros(N, fmap.dtype)
        out[:fmap.size] = fmap.reshape(-1)
        return out


def conv2d_packed_plan(in_c: int, in_h: int, in_w: int, k_h: int, k_w: int, stride=1) -> PackedConvPlan:
    """The packed form of the convolution: a whole feature map of in_c * in_h * in_w <= N values in ONE TRLWE, each
    filter one plaintext polynomial, every output of the valid (unpadded) convolution one coefficient of their product.
      * the map: value (c, y, x) at coefficient c H W + y W + x  (plan.encode; padding is the client's affair: it packs
        an already padded map);
      * filter oc (conv2d_packed_weights): f[oc][ky][kx][c] at coefficient O - (c H W + ky W + kx),
        O = (C - 1) H W + (k_h - 1) W + (k_w - 1)  (plan.offset);
      * output (oy, ox) of the stride-1 convolution: coefficient O + oy W + ox of the product; a stride only picks fewer
        of them.  plan.slots [out_h][out_w] holds them: Engine.unpack(product, slots=plan.slots) gives the lv0
        ciphertexts in [out_h][out_w] order.
    Safe because a product term lands at O + (map index) - (filter index): the wanted slots are at most
    O + (H - k_h) W + (W - k_w) = C H W - 1 < N, and a term that wraps past N comes back at an index below
    O + C H W - N <= O, under every wanted slot.  The other coefficients of the product hold sums nobody asked for.
    ValueError if the map does not fit."""
    return PackedConvPlan(in_c, in_h, in_w, k_h, k_w, stride)


def conv2d_packed_weights(w, plan: PackedConvPlan) -> np.ndarray:
    """Filters [out_c][k_h][k_w][in_c] int8 (the layout of conv2d) -> [out_c][1][N] int8 polynomials for polymul, by
    `plan`'s encoding."""
    w = np.asarray(w)
    if w.ndim != 4 or w.shape[0] < 1 or w.shape[1:] != (plan.k_h, plan.k_w, plan.in_c):
        raise ValueError(f"w must be [out_c][{plan.k_h}][{plan.k_w}][{plan.in_c}]")
    if not np.issubdtype(w.dtype, np.integer) or w.min() < -128 or w.max() > 127:
        raise ValueError("weights must be integers in [-128, 127]")
    c, ky, kx = np.meshgrid(np.arange(plan.in_c), np.arange(plan.k_h), np.arange(plan.k_w), indexing="ij")
    at = plan.offset - (c * plan.in_h * plan.in_w + ky * plan.in_w + kx)   # [in_c][k_h][k_w]
    out = np.zeros((w.shape[0], 1, N), np.int8)
    out[:, 0, at.reshape(-1)] = w.transpose(0, 3, 1, 2).reshape(w.shape[0], -1)
    return out


def polymul(w, packed, cloud_key, bias=None, device: int = 0) -> np.ndarray:
    """The server side of the polynomial product: [groups][cols][2][N] TRLWE lv1 ciphertexts (the forms of
    _packed_inputs) -> [groups][rows][2][N] on the GPU (Engine.batch_trlwe_polymul on the shared context of
    `cloud_key`'s parameter set; the product itself uses no key)."""
    from .bootstrap import keyed_engine

    w8, bias = _polys(w, bias)
    packed = _packed_inputs(packed, w8.shape[1])
    with keyed_engine(cloud_key, device) as view:
        return view.batch_trlwe_polymul(w8, packed, bias)


def _checked(w, bias, max_cols: int):
    """(w as int8, bias as u32 or None): what the user-level calls check before they touch the library."""
    w, bias = _weights(w, bias, max_cols)
    return w.astype(np.int8), bias


def matmul(w, cts, cloud_key, bias=None, device: int = 0) -> np.ndarray:
    """The server side, dense form: [groups][cols][n+1] ciphertexts -> [groups][rows][n+1] on the GPU
    (Engine.batch_tlwe_matmul on the shared context of `cloud_key`'s parameter set; the product itself uses no key)."""
    from .bootstrap import keyed_engine

    p = cloud_key.params
    w8, bias = _checked(w, bias, MAX_COLS)
    cts = np.ascontiguousarray(cts, dtype=np.uint32)
    if cts.ndim not in (2, 3) or cts.shape[-2:] != (w8.shape[1], p.n + 1):
        raise ValueError(f"cts must be [groups][{w8.shape[1]}][{p.n + 1}]")
    with keyed_engine(cloud_key, device) as view:
        return view.batch_tlwe_matmul(w8, cts, bias)


def matmul_packed(w, packed, cloud_key, bias=None, keyswitch: bool = True, device: int = 0) -> np.ndarray:
    """The server side, packed form: slots 0 .. cols-1 of [groups][2][N] TRLWE lv1 ciphertexts -> [groups][rows][n+1]
    lv0 ciphertexts under `cloud_key`'s key-switching key (keyswitch=False: [groups][rows][N+1] lv1 rows)."""
    from .bootstrap import keyed_engine

    w8, bias = _checked(w, bias, N)
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    if packed.ndim not in (2, 3) or packed.shape[-2:] != (2, N):
        raise ValueError(f"packed must be [groups][2][{N}]")
    with keyed_engine(cloud_key, device) as view:
        return view.batch_trlwe_matmul(w8, packed, bias, keyswitch)


def conv2d(w, cts, cloud_key, bias=None, stride=1, padding=0, device: int = 0) -> np.ndarray:
    """The server side of a convolutional layer: [groups][in_h][in_w][in_c][n+1] ciphertexts (or one group without the
    leading axis) -> [groups][out_h][out_w][out_c][n+1] on the GPU (Engine.batch_tlwe_conv2d on the shared context of
    `cloud_key`'s parameter set; the convolution itself uses no key)."""
    from .bootstrap import keyed_engine

    p = cloud_key.params
    w, bias = _filters(w, bias)
    cts = np.ascontiguousarray(cts, dtype=np.uint32)
    if cts.ndim not in (4, 5) or cts.shape[-2:] != (w.shape[3], p.n + 1):
        raise ValueError(f"cts must be [groups][in_h][in_w][{w.shape[3]}][{p.n + 1}]")
    conv2d_out_shape(cts.shape[-4], cts.shape[-3], w.shape[1], w.shape[2], stride, padding)
    with keyed_engine(cloud_key, device) as view:
        return view.batch_tlwe_conv2d(w.astype(np.int8), cts, bias, stride, padding)
