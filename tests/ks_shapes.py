"""Shape sweep of the integer key-switch family (used by tests/test_ks_shapes_host.py on the CPU and by
tests/test_gpu_ks_shapes.py on the HIP kernels).  No tests here and no device import.

tfhe_hip_ctx_create accepts n in 1..1279, basebit in 1..10, t >= 1 with basebit t <= 31; the reference parameter sets
are eleven points of that box.  The tables below are small shapes of the box chosen by what they make the kernels do
(which k_key_switch_mfma<NT> runs, with an even or an odd tile count; how many 64-column slices the sliced kernel has;
whether a 32-coefficient block of the packing walk is partial), every one carrying the kernels it is swept on.  The
conditions they are chosen for are asserted by tests/test_ks_shapes_host.py through the mirrors of the launch
arithmetic below, whose constants are read out of the headers: a retune that moves a shape to another instantiation
fails there, not silently.

All of it is exact integer arithmetic: the expected words are packing.key_switch_model / pack_model / table_model /
unpack_model (the host file holds key_switch_model to the C oracle on every table shape first), compared with
np.array_equal.  The keys are random words, not keys of a secret: the identities hold word for word under any key.
"""
import os
import re
from collections import namedtuple

import numpy as np

N = 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs-tfhe_amd", "csrc")
# carries between balanced byte planes (the words tests/test_gpu_matmul.py plants: test_ks_shapes_host.py compares)
EDGES = (0, 0x80000000, 0xFFFFFFFF, 0x7F7F7F7F, 0x80808080, 0x00800080, 0x7FFFFFFF)
KERNELS = ("mfma", "sliced", "b4", "generic", "split")  # TFHE_HIP_KS_KERNEL
DISTINCT = 96  # distinct lv1 rows per shape
MASK_SEED = bytes(range(100, 132))  # the packing keys' public mask seed


# ---- constants of the launch arithmetic, read from the sources ---------------------------------------------------------
def _read_constants():
    text = "\n".join(open(os.path.join(CSRC, f)).read()
                     for f in ("key_switch_mfma.hpp", "key_switch.hpp", "packing.hpp", "tfhe_hip.hip"))
    out = {}
    for name in ("kKmWaves", "kKmFrags", "kKmColBlocks", "kKmMaxTiles", "kPkNT", "kKsG", "kKsRingSlots", "kKsStage"):
        found = re.findall(r"constexpr\s+int\s+%s\s*=\s*([^;]+);" % name, text)
        assert len(found) == 1, (name, found)
        expr = found[0].strip()
        assert re.fullmatch(r"[\w\s/*+()-]+", expr), (name, expr)
        out[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(out)))  # earlier constants only
    return out


C = _read_constants()
kKmRows = 32 * C["kKmFrags"] * C["kKmWaves"]  # ciphertexts per workgroup of the matrix-core kernel


# ---- mirrors of key_switch_mfma.hpp / packing.hpp / tfhe_hip.hip ---------------------------------------------------------
def ks_mfma_total_tiles(n):
    return (n + 1 + 31) // 32


def ks_mfma_nt(n):
    """ks_mfma_tiles: tiles of the widest column block, the kernel's NT"""
    return -(-ks_mfma_total_tiles(n) // C["kKmColBlocks"])


def ks_mfma_block_tiles(n, cb):
    tiles = ks_mfma_total_tiles(n)
    return tiles // C["kKmColBlocks"] + (1 if cb < tiles % C["kKmColBlocks"] else 0)


def ks_mfma_tpw(nt):
    return -(-nt // C["kKmWaves"])


def ks_mfma_col_blocks(n):
    """launch_key_switch: grid.y = min(tiles, kKmColBlocks)"""
    return min(ks_mfma_total_tiles(n), C["kKmColBlocks"])


def ks_mfma_runs_short_block(n):
    """whether a launched column block has NT - 1 tiles: k_key_switch_mfma's run(std::false_type{})"""
    return any(ks_mfma_block_tiles(n, cb) == ks_mfma_nt(n) - 1 for cb in range(ks_mfma_col_blocks(n)))


def ks_mfma_unsplit_count(n, cus):
    """The smallest count whose launch does not cut K (plan_key_switch: the walk is cut while row blocks x column
    blocks x 4 planes x chunks stay below two workgroups per CU)."""
    rb = -(-2 * cus // (ks_mfma_col_blocks(n) * 4))
    return (rb - 1) * kKmRows + 1


def ks_sliced_slices(n):
    return (n + 1 + 63) // 64


def pk_blocks(n):
    return (n + 31) // 32


def available(n, basebit, t):
    """ks_kind_possible: the kernels TFHE_HIP_KS_KERNEL may name for a parameter set (the others fail creation)."""
    out = {"generic", "split"}
    if basebit == 2 and 6 <= t <= 13 and 1 <= ks_mfma_nt(n) <= C["kKmMaxTiles"]:
        out.add("mfma")
    if 4 <= basebit <= 7:  # (the ring of every one of these bases fits a CU's LDS)
        out.add("sliced")
    waves = (((((n + 1 + 3) & ~3) >> 2) + 63) & ~63) >> 6
    if basebit == 2 and C["kKsRingSlots"] * 4 * waves * 1024 + C["kKsG"] * C["kKsStage"] * 4 <= 64 * 1024:
        out.add("b4")  # n <= 1023: the ring of five waves (n up to 1279) does not fit 64 KiB
    return out


# ---- the tables ------------------------------------------------------------------------------------------------------------
Shape = namedtuple("Shape", "n basebit t kernels")


def shape_id(s):
    return f"n{s.n}_b{s.basebit}_t{s.t}"


# k_key_switch_mfma<NT>: every NT = 1 .. 12, with an even and with an odd tile count (odd: the second column block has
# NT - 1 tiles), one column block (n + 1 <= 32), a tile that holds the body column alone (n + 1 = 32 k + 1), t = 6 .. 13
MFMA_SHAPES = tuple(Shape(n, 2, t, ("mfma",)) for n, t in (
    (1, 6), (31, 13), (32, 6), (64, 13), (127, 7), (150, 10), (160, 11), (200, 12), (255, 6), (256, 13), (300, 8), (330, 6),
    (400, 9), (447, 7), (470, 8), (500, 6), (530, 9), (600, 8), (660, 6), (710, 13), (767, 7),
    # 12, 18, 20 and 22 tiles: the even counts of NT = 6, 9, 10 and 11 (the last three are the reference sets' counts)
    (370, 10), (560, 11), (639, 12), (703, 9)))
# base 4 without the matrix cores; (1279, 2, 5) is refused by k_key_switch_b4 (five waves: its ring passes 64 KiB)
B4_SHAPES = (Shape(1, 2, 1, ("b4", "generic", "split")), Shape(3, 2, 15, ("b4", "generic", "split")),
             Shape(4, 2, 6, ("b4", "generic", "split")), Shape(1279, 2, 5, ("generic", "split")))
GENERIC_SHAPES = tuple(Shape(n, b, t, ("generic", "split")) for n, b, t in (
    (3, 10, 3), (7, 9, 3), (15, 8, 3), (33, 1, 31), (100, 3, 10), (1279, 1, 1)))
SLICED_SHAPES = tuple(Shape(n, b, t, ("sliced", "generic", "split")) for n, b, t in (
    (1, 4, 1), (62, 4, 7), (63, 5, 6), (64, 6, 5), (63, 7, 4), (64, 7, 1), (640, 5, 1), (1279, 4, 2)))
# automatic dispatch at count 200: whether the matrix-core kernel runs (its bounds: n <= 767, 6 <= t <= 13)
SELECTOR_SHAPES = (Shape(767, 2, 8, ("mfma",)), Shape(768, 2, 8, ()), Shape(700, 2, 5, ()), Shape(700, 2, 14, ()))
SELECTOR_COUNT = 200
IDENTITY_SHAPES = MFMA_SHAPES + B4_SHAPES + GENERIC_SHAPES + SLICED_SHAPES
IDENTITY_CASES = tuple((s, k) for s in IDENTITY_SHAPES for k in s.kernels)
IDENTITY_COUNTS = (1, 33, 127, 128, 129, 515)
UNSPLIT_SHAPES = ((31, 2, 13), (447, 2, 7))  # mfma shapes that also run the smallest count whose launch does not cut K
PINNED_CASE = ((100, 3, 10), "split", (1, 63, 300))  # the pinned-host-output form: (shape, kernel, counts)

# packing / table key switch (k_box_mfma, k_pack_planes, PackDigits): (n, basebit, t)
PACK_SHAPES = ((1, 1, 1), (15, 2, 9), (16, 3, 10), (17, 7, 4), (31, 4, 7), (32, 5, 6), (33, 6, 5), (64, 1, 31), (129, 2, 13),
               (1279, 2, 2), (1279, 7, 4))
PACK_COUNTS = (1, 31, 32, 33, 1024, 1025)
TABLE_MS = (2, 4, 32, 512)  # 512 = the widest table the library takes
TABLE_M_REFUSED = 1024      # W = N / m = 1 has no half-box rotation: refused ("m must be a power of two in [2, 512]")
TABLE_COUNT = 3


def pack_id(s):
    return f"n{s[0]}_b{s[1]}_t{s[2]}"


# ---- parameters ------------------------------------------------------------------------------------------------------------
def product_params(n, basebit, t):
    """l = 1, bgbit = 10: the blind rotation's side of the set is not what is swept (its key is zeros)."""
    from rs_tfhe_amd.params import SecurityParams

    return SecurityParams(f"KS_n{n}_b{basebit}_t{t}", 0, n, 1, 10, basebit, t, 2.0e-5, 2.2e-16)


def oracle_params(O, n, basebit, t):
    return O.Params(f"KS_n{n}_b{basebit}_t{t}", n, 1, 10, basebit, t, 2.0e-5, 2.2e-16)


def _seed(n, basebit, t):
    return (n * 64 + basebit) * 64 + t


# ---- keys ------------------------------------------------------------------------------------------------------------------
def edge_columns(width):
    """Columns 0, width - 2, width - 1 (a key-switching key row: 0, n - 1, n) and both sides of every 32-column
    boundary (every other one of them a 64-column boundary) of a row of `width` words."""
    cols = {0, width - 1}
    if width >= 2:
        cols.add(width - 2)
    for b in range(32, width, 32):
        cols.update((b - 1, b))
    return sorted(cols)


def _plant(rows, cols):
    """EDGES down every column of `cols`, on every other row (the rows between keep their random words)."""
    r = np.arange(0, len(rows), 2)
    edges = np.array(EDGES, np.uint32)
    for q, c in enumerate(cols):
        rows[r, c] = edges[(r // 2 + q) % len(EDGES)]


def build_ksk(n, basebit, t):
    """[N][t][base][n+1] random u32 with the carry patterns planted; the k = 0 rows are zero (the engine layout's)."""
    rng = np.random.default_rng(_seed(n, basebit, t))
    ksk = rng.integers(0, 1 << 32, (N, t, 1 << basebit, n + 1), dtype=np.uint32)
    _plant(ksk.reshape(-1, n + 1), edge_columns(n + 1))
    ksk[:, :, 0, :] = 0
    return ksk


def build_pack_bodies(n, basebit, t):
    """[n][t][N] random u32 with the carry patterns planted (the a halves of the rows come from MASK_SEED)."""
    rng = np.random.default_rng(_seed(n, basebit, t) + 1)
    bodies = rng.integers(0, 1 << 32, (n, t, N), dtype=np.uint32)
    _plant(bodies.reshape(-1, N), edge_columns(N))
    return bodies


# ---- rows ------------------------------------------------------------------------------------------------------------------
def special_words(basebit, t):
    """a = 0 (every digit 0), 0xFFFFFFFF, every digit base - 1, and the words at and one below the rounding carry."""
    bt = basebit * t
    prec = 1 << (31 - bt)
    m = 0xFFFFFFFF
    return (0, m, ((((1 << bt) - 1) << (32 - bt)) - prec) & m, (0 - prec) & m, (0 - prec - 1) & m)


def _fill_specials(a, basebit, t):
    """`a` [rows][width] random words: rows 1, 3, .. take one special word each throughout, the row after them takes
    them in turn along the row (so row 0, all a batch of one holds, stays random)."""
    sp = np.array(special_words(basebit, t), np.uint32)
    for q, w in enumerate(sp):
        if 2 * q + 1 < len(a):
            a[2 * q + 1] = w
    if 2 * len(sp) + 1 < len(a):
        a[2 * len(sp) + 1] = sp[np.arange(a.shape[1]) % len(sp)]


def build_rows(n, basebit, t, distinct=DISTINCT):
    """The distinct lv1 rows [distinct][N+1] of a shape: random, and the special words (the bodies stay random)."""
    rng = np.random.default_rng(_seed(n, basebit, t) + 2)
    rows = rng.integers(0, 1 << 32, (distinct, N + 1), dtype=np.uint32)
    _fill_specials(rows[:, :N], basebit, t)
    return rows


def batch_index(count, distinct, seed=0):
    """Which distinct row every row of a batch of `count` is: every one present once count reaches `distinct` (then
    in a shuffled order, with repetitions), the first `count` of them below."""
    rng = np.random.default_rng(1000 + seed + count)
    idx = np.concatenate([np.arange(min(count, distinct)), rng.integers(0, distinct, max(count - distinct, 0))])
    if count > distinct:
        rng.shuffle(idx)
    return idx


def build_tlwe(n, basebit, t, count, seed):
    """[count][n+1] lv0 inputs of the packing side: random, with the special words as in build_rows."""
    rng = np.random.default_rng(_seed(n, basebit, t) + 3 + seed)
    cts = rng.integers(0, 1 << 32, (count, n + 1), dtype=np.uint32)
    _fill_specials(cts[:, :n], basebit, t)
    return cts


def build_trlwe(n, basebit, t, groups=2):
    """[groups][2][N] for unpacking: random, EDGES at both ends of every row (what slots 0 and N - 1 read first)."""
    rng = np.random.default_rng(_seed(n, basebit, t) + 4)
    trlwe = rng.integers(0, 1 << 32, (groups, 2, N), dtype=np.uint32)
    trlwe[:, :, :len(EDGES)] = EDGES
    trlwe[:, :, -len(EDGES):] = EDGES
    return trlwe


def unpack_slots(n, basebit, t, groups=2):
    rng = np.random.default_rng(_seed(n, basebit, t) + 5)
    return np.concatenate([[0, 1, N - 1, N, groups * N - 1], rng.integers(0, groups * N, 7)]).astype(np.int64)


# ---- one shape's key, rows and expected words (the last shape asked for is kept: the cases of a shape run in a row) -------
class Case:
    def __init__(self, n, basebit, t):
        from rs_tfhe_amd import packing as PK

        self.shape = (n, basebit, t)
        self.params = product_params(n, basebit, t)
        self.ksk = build_ksk(n, basebit, t)
        self.rows = build_rows(n, basebit, t)
        self.expected = PK.key_switch_model(self.params, self.ksk, self.rows)
        self._unpack = None

    def oracle_key(self, O):
        n, basebit, t = self.shape
        return O.CloudKey.from_arrays(oracle_params(O, n, basebit, t), np.zeros((n, 2, 2, N)), self.ksk, 0,
                                      np.zeros((2, N), np.uint32))

    def cloud_key(self, testvec=None):
        """The product's CloudKey: this key-switching key beside an all-zero bootstrapping key."""
        import rs_tfhe_amd as R

        n = self.shape[0]
        tv = np.zeros((2, N), np.uint32) if testvec is None else testvec
        return R.CloudKey(self.params, np.zeros((n, 2, 2, N)), self.ksk, None, tv)

    def unpack_case(self):
        """(trlwe, slots, expected) of the unpacking call"""
        if self._unpack is None:
            from rs_tfhe_amd import packing as PK

            trlwe, slots = build_trlwe(*self.shape), unpack_slots(*self.shape)
            self._unpack = (trlwe, slots, PK.unpack_model(self.params, self.ksk, trlwe, slots=slots))
        return self._unpack


_LAST = {}


def case(shape):
    key = tuple(shape[:3])
    if key not in _LAST:
        _LAST.clear()
        _LAST[key] = Case(*key)
    return _LAST[key]
