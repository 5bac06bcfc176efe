"""The key-switch shape sweep on the host, no GPU (tests/ks_shapes.py; the kernels run in tests/test_gpu_ks_shapes.py):
the coverage conditions the tables are chosen for, asserted through the mirrors of the launch arithmetic so that a table
edit or a retune of the kernels cannot quietly cover less; the two references (packing.key_switch_model and the C oracle's
identity_key_switching) agree on every table shape before either judges the GPU; no comparison can pass by default; the
keys and batches stay small."""
import re

import numpy as np
import pytest

import ks_shapes as S

N = S.N
ALL_SHAPES = S.IDENTITY_SHAPES + S.SELECTOR_SHAPES


def test_constants_are_read_from_the_sources():
    """The mirrors at the reference sets: 22 / 20 / 18 tiles in two column blocks, NT = 11 / 10 / 9, three tiles a
    wave; eight tiles a wave in the packing walk."""
    assert S.C["kKmColBlocks"] >= 1 and S.C["kKmWaves"] >= 1 and S.C["kKmFrags"] >= 1 and S.C["kPkNT"] >= 1
    assert S.C["kKmMaxTiles"] * S.C["kKmFrags"] == 12 and S.kKmRows == 32 * S.C["kKmFrags"] * S.C["kKmWaves"]
    for n in (550, 630, 700):
        tiles = S.ks_mfma_total_tiles(n)
        assert tiles == -(-(n + 1) // 32)
        assert sum(S.ks_mfma_block_tiles(n, cb) for cb in range(S.C["kKmColBlocks"])) == tiles
        assert S.ks_mfma_nt(n) == max(S.ks_mfma_block_tiles(n, cb) for cb in range(S.C["kKmColBlocks"]))
    assert [S.pk_blocks(n) for n in (1, 32, 33, 1279)] == [1, 1, 2, 40]
    assert S.available(700, 2, 9) == {"mfma", "b4", "generic", "split"}
    assert S.available(820, 5, 3) == {"sliced", "generic", "split"}


def test_edges_are_the_matmul_tests_words():
    text = open(S.ROOT + "/tests/test_gpu_matmul.py").read()
    found = re.search(r"^EDGES = \(([^)]*)\)", text, flags=re.M)
    assert found and tuple(int(w, 0) for w in found.group(1).split(",")) == S.EDGES


def test_every_entry_is_accepted_and_carries_available_kernels():
    seen = set()
    for s in ALL_SHAPES:
        assert 1 <= s.n <= 1279 and 1 <= s.basebit <= 10 and s.t >= 1 and s.basebit * s.t <= 31, s
        assert set(s.kernels) <= S.available(s.n, s.basebit, s.t), s
        assert s[:3] not in seen, s
        seen.add(s[:3])
    for s in S.MFMA_SHAPES:
        assert "mfma" in s.kernels
    for s in S.SLICED_SHAPES:
        assert {"sliced", "generic", "split"} <= set(s.kernels)
    for s in S.B4_SHAPES + S.GENERIC_SHAPES:
        assert {"generic", "split"} <= set(s.kernels)
    # the one listed b4 shape the kernel cannot take (five waves: its ring passes 64 KiB) is swept as a refusal
    assert [s[:3] for s in S.B4_SHAPES if "b4" not in s.kernels] == [(1279, 2, 5)]
    assert "b4" not in S.available(1279, 2, 5) and "b4" in S.available(1023, 2, 5)
    for n, b, t in S.PACK_SHAPES:
        assert 1 <= n <= 1279 and 1 <= b <= 7 and b * t <= 31
    assert {tuple(u) for u in S.UNSPLIT_SHAPES} <= {s[:3] for s in S.MFMA_SHAPES}
    assert S.PINNED_CASE[1] in {s[:3]: s for s in S.IDENTITY_SHAPES}[S.PINNED_CASE[0]].kernels


def test_mfma_table_coverage():
    shapes = S.MFMA_SHAPES
    nts = {S.ks_mfma_nt(s.n) for s in shapes}
    assert nts == set(range(1, S.C["kKmMaxTiles"] + 1)) == set(range(1, 13))
    for nt in range(2, 13):
        parities = {S.ks_mfma_total_tiles(s.n) % 2 for s in shapes if S.ks_mfma_nt(s.n) == nt}
        assert parities == {0, 1}, nt
        # an odd count is what runs the branch whose last tile is skipped
        assert any(S.ks_mfma_runs_short_block(s.n) for s in shapes if S.ks_mfma_nt(s.n) == nt), nt
    assert {S.ks_mfma_tpw(S.ks_mfma_nt(s.n)) for s in shapes} == {1, 2, 3}
    one_block = [s for s in shapes if S.ks_mfma_col_blocks(s.n) == 1]
    assert any(s.n + 1 < 32 for s in one_block) and any(s.n + 1 == 32 for s in one_block)
    assert any((s.n + 1) % 32 == 1 and s.n + 1 > 32 for s in shapes)  # a tile that holds the body column alone
    assert {6, 13} <= {s.t for s in shapes} and {s.t for s in shapes} == set(range(6, 14))
    for u in S.UNSPLIT_SHAPES:
        assert S.ks_mfma_unsplit_count(u[0], 256) * (N + 1) * 4 < 100e6
    assert {S.ks_mfma_col_blocks(u[0]) for u in S.UNSPLIT_SHAPES} == {1, 2}


def test_generic_split_table_coverage():
    shapes = [s for s in S.IDENTITY_SHAPES if {"generic", "split"} <= set(s.kernels)]
    assert {s.basebit for s in shapes} == set(range(1, 11))
    assert {30, 31} <= {s.basebit * s.t for s in shapes}
    assert 1279 in {s.n for s in shapes} and 1 in {s.n for s in shapes}


def test_sliced_table_coverage():
    shapes = S.SLICED_SHAPES
    assert {s.basebit for s in shapes} == {4, 5, 6, 7}
    assert {1, 2, 20} <= {S.ks_sliced_slices(s.n) for s in shapes}
    assert {63, 64, 65} <= {s.n + 1 for s in shapes}


def test_packing_table_coverage():
    shapes = S.PACK_SHAPES
    assert {b for _, b, _ in shapes} == set(range(1, 8))
    assert {28, 30, 31} <= {b * t for _, b, t in shapes}
    assert {1, 15, 16, 17, 31, 32, 33, 1279} <= {n for n, _, _ in shapes}
    assert {1, 31} <= {t for _, _, t in shapes}
    assert 1 in {S.pk_blocks(n) for n, _, _ in shapes}  # one coefficient block: no K cut
    assert S.TABLE_M_REFUSED == 1024 and set(S.TABLE_MS) >= {2, 4, 32}


def test_selector_edges():
    runs = {s[:3]: "mfma" in S.available(s.n, s.basebit, s.t) for s in S.SELECTOR_SHAPES}
    assert runs == {(767, 2, 8): True, (768, 2, 8): False, (700, 2, 5): False, (700, 2, 14): False}
    for s in S.SELECTOR_SHAPES:
        assert ("mfma" in s.kernels) == runs[s[:3]]


def test_memory_bounds():
    cus = 256
    for s in ALL_SHAPES:
        assert N * s.t * (1 << s.basebit) * (s.n + 1) * 4 < 200e6, s
        counts = list(S.IDENTITY_COUNTS) + [S.SELECTOR_COUNT]
        if s[:3] in S.UNSPLIT_SHAPES:
            counts.append(S.ks_mfma_unsplit_count(s.n, cus))
        for count in counts:
            assert count * (N + 1) * 4 < 100e6 and count * (s.n + 1) * 4 < 100e6, (s, count)
    for n, b, t in S.PACK_SHAPES:
        assert n * t * 2 * N * 4 < 200e6 and max(max(S.PACK_COUNTS), max(S.TABLE_MS) * S.TABLE_COUNT) * (n + 1) * 4 < 100e6


def test_rows_and_batches():
    for b, t in ((2, 9), (1, 31), (10, 3), (7, 4), (2, 1)):
        rows = S.build_rows(5, b, t)
        assert len(rows) <= 96 and len(np.unique(rows, axis=0)) == len(rows)
        bt, base = b * t, 1 << b
        abar = rows[:, :N] + np.uint32(1 << (31 - bt))
        dig = np.stack([(abar >> np.uint32(32 - (j + 1) * b)) & np.uint32(base - 1) for j in range(t)], axis=2)
        assert (dig[1] == 0).all() and (rows[1, :N] == 0).all()      # a = 0
        assert (rows[3, :N] == 0xFFFFFFFF).all()
        assert (dig[5] == base - 1).all()                            # every digit base - 1
        assert (dig[7] == 0).all() and (rows[7, :N] != 0).all()      # at the rounding carry: a_bar wraps to 0
        assert (dig[9] == base - 1).all()                            # one below it
        assert len({int(w) for w in rows[11, :N]}) == len(set(S.special_words(b, t)))
    for count in S.IDENTITY_COUNTS + (8065,):
        idx = S.batch_index(count, S.DISTINCT)
        assert len(idx) == count and idx.min() >= 0 and idx.max() < S.DISTINCT
        assert len(set(idx.tolist())) == min(count, S.DISTINCT)


def test_keys_carry_the_planted_words():
    ksk = S.build_ksk(70, 2, 3)
    assert not ksk[:, :, 0].any() and ksk[:, :, 1:].any()
    assert S.edge_columns(71) == [0, 31, 32, 63, 64, 69, 70]
    flat = ksk.reshape(-1, 71)
    for c in S.edge_columns(71):
        assert set(S.EDGES) - {0} <= {int(w) for w in flat[:, c]}
    bodies = S.build_pack_bodies(3, 2, 2)
    assert bodies.shape == (3, 2, N) and {0, 31, 32, 63, 64, N - 2, N - 1} <= set(S.edge_columns(N))


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=S.shape_id)
def test_model_equals_the_oracle_and_no_column_is_trivial(O, shape):
    """packing.key_switch_model and the oracle's identity_key_switching (trgsw.rs:332-360) are independent; the GPU is
    held to words both agree on.  No expected column is identically zero over the distinct rows."""
    case = S.case(shape)
    assert case.ksk.nbytes < 200e6 and not case.ksk[:, :, 0].any()
    ref = O.batch_identity_key_switching(case.oracle_key(O), case.rows)
    assert np.array_equal(case.expected, ref)
    assert case.expected.shape == (S.DISTINCT, shape.n + 1) and case.expected.any(axis=0).all()
    trlwe, slots, exp = case.unpack_case()
    rows = np.stack([O.sample_extract_index(trlwe[s // N], s % N) for s in slots])
    assert np.array_equal(exp, O.batch_identity_key_switching(case.oracle_key(O), rows))
    assert exp.any(axis=0).all()
