"""The integer key-switch family over the box of shapes tfhe_hip_ctx_create accepts, not just the reference sets
(tests/ks_shapes.py holds the tables, the keys and the rows; tests/test_ks_shapes_host.py what they cover and that the
two references agree).  One case per (shape, kernel): its own Engine with TFHE_HIP_KS_KERNEL set before creation, the
kernel asserted in describe_dispatch, every word compared with np.array_equal against packing.key_switch_model /
unpack_model / pack_model / table_model.  A shape the library accepts computes the model's words, or the forced selector
(or the call) refuses it: a refusal where the table says available, or the other way round, fails the case.

Swept: k_key_switch_mfma<1 .. 12> with even and odd tile counts (the second column block one tile short), one column
block, a tile with the body column alone, t = 6 .. 13, with K cut and not cut; k_key_switch_b4 / k_key_switch /
k_key_switch_split at basebit 1 .. 10, basebit t = 30 and 31, n = 1 and 1279; k_key_switch_sliced at basebit 4 .. 7 with
1, 2, 11 and 20 slices; k_box_mfma / k_pack_planes / PackDigits at n around 16 and 32 and at 1279, basebit 1 .. 7, t = 1
and 31; the bounds of the automatic choice of the matrix-core kernel."""
import ctypes as C

import numpy as np
import pytest

import ks_shapes as S

pytestmark = pytest.mark.gpu
N = S.N


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("shape,kernel", S.IDENTITY_CASES, ids=[f"{S.shape_id(s)}-{k}" for s, k in S.IDENTITY_CASES])
def test_identity_key_switch_and_unpack_equal_the_model(monkeypatch, shape, kernel):
    import rs_tfhe_amd as R

    case = S.case(shape)
    monkeypatch.setenv("TFHE_HIP_KS_KERNEL", kernel)
    eng = R.Engine(case.params, 0)  # (refused where the table says available: the case fails)
    try:
        eng.load_cloud_key(case.cloud_key())
        counts = S.IDENTITY_COUNTS
        if kernel == "mfma" and shape[:3] in S.UNSPLIT_SHAPES:
            unsplit = S.ks_mfma_unsplit_count(shape.n, _cus())
            assert "key_switch=mfma(k=1)" in eng.describe_dispatch(unsplit)
            assert "key_switch=mfma(k=2)" in eng.describe_dispatch(unsplit - 1)  # ... and it is the smallest such count
            counts += (unsplit,)
        for count in counts:
            assert f"key_switch={kernel}" in eng.describe_dispatch(count)
            idx = S.batch_index(count, len(case.rows))
            got = eng.batch_identity_key_switch(case.rows[idx])
            assert np.array_equal(got, case.expected[idx]), (shape, kernel, count)
        trlwe, slots, exp = case.unpack_case()
        assert f"key_switch={kernel}" in eng.describe_dispatch(len(slots))
        assert np.array_equal(eng.unpack(trlwe, slots=slots), exp), (shape, kernel, "unpack")
    finally:
        eng.close()


def test_selectors_the_tables_do_not_carry_are_refused(monkeypatch):
    """Every kernel a swept parameter set cannot run fails creation with "not available" (ks_kind_possible), before
    anything is allocated -- (1279, 2, 5) on b4 among them."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi

    refused = 0
    for s in S.IDENTITY_SHAPES + S.SELECTOR_SHAPES:
        for kernel in set(S.KERNELS) - S.available(s.n, s.basebit, s.t):
            assert kernel not in s.kernels
            monkeypatch.setenv("TFHE_HIP_KS_KERNEL", kernel)
            with pytest.raises(_capi.TfheHipError, match="not available"):
                R.Engine(S.product_params(*s[:3]), 0)
            refused += 1
    assert refused >= len(S.IDENTITY_SHAPES)  # (no set runs all five)


@pytest.mark.parametrize("shape", S.SELECTOR_SHAPES, ids=S.shape_id)
def test_automatic_choice_at_the_matrix_core_kernels_bounds(monkeypatch, shape):
    """basebit 2, 200 ciphertexts: n = 767 (24 tiles, NT = 12) and t = 6 .. 13 are the last shapes the matrix-core
    kernel takes; one column or one digit further the automatic choice is another kernel, and forcing it is refused."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi

    monkeypatch.delenv("TFHE_HIP_KS_KERNEL", raising=False)
    case = S.case(shape)
    eng = R.Engine(case.params, 0)
    try:
        eng.load_cloud_key(case.cloud_key())
        plan = eng.describe_dispatch(S.SELECTOR_COUNT)
        assert ("key_switch=mfma" in plan) == ("mfma" in shape.kernels), plan
        idx = S.batch_index(S.SELECTOR_COUNT, len(case.rows))
        assert np.array_equal(eng.batch_identity_key_switch(case.rows[idx]), case.expected[idx]), plan
    finally:
        eng.close()
    if "mfma" not in shape.kernels:
        monkeypatch.setenv("TFHE_HIP_KS_KERNEL", "mfma")
        with pytest.raises(_capi.TfheHipError, match="not available"):
            R.Engine(case.params, 0)


def test_atomic_kernel_with_pinned_host_output(monkeypatch):
    """The pinned-operand form of tfhe_hip_batch_bootstrap (in place, the atomic key switch through a device buffer
    and one copy: test_gpu_dispatch.py) on a swept shape.  Under the all-zero bootstrapping key every CMUX step is the
    identity, so the key switch's input is the sample extract of the rotated test vector -- random words here."""
    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.engine import pinned_copy, pinned_empty

    shape, kernel, counts = S.PINNED_CASE
    case = S.case(shape)
    tv = np.random.default_rng(77).integers(0, 1 << 32, (2, N), dtype=np.uint32)
    monkeypatch.setenv("TFHE_HIP_KS_KERNEL", kernel)
    eng = R.Engine(case.params, 0)
    try:
        eng.load_cloud_key(case.cloud_key(testvec=tv))
        for count in counts:
            assert f"key_switch={kernel}" in eng.describe_dispatch(count)
            cts = S.build_tlwe(*shape, count, 6)
            pin, pout = pinned_copy(cts), pinned_empty(cts.shape)
            pout[...] = 0xDEADBEEF
            rc = eng._lib.tfhe_hip_batch_bootstrap(eng._ctx, pin.ctypes.data_as(C.c_void_p), None, 0, 1,
                                                   pout.ctypes.data_as(C.c_void_p), count)
            assert rc == 0, eng._lib.tfhe_hip_last_error(eng._ctx)
            rotated = eng.batch_blind_rotate(cts)
            exp = PK.key_switch_model(case.params, case.ksk, PK.extract_rows(rotated, np.arange(count) * N))
            assert rotated[:, 0].any() and exp[:, :shape[0]].any()
            assert np.array_equal(pout, exp), count
            assert np.array_equal(eng.batch_bootstrap(cts), exp), count  # pageable arrays: device staging
    finally:
        eng.close()


@pytest.mark.parametrize("shape", S.PACK_SHAPES, ids=S.pack_id)
def test_pack_and_table_key_switch_equal_the_models(shape):
    import rs_tfhe_amd as R
    from rs_tfhe_amd import _capi, packing as PK

    n, basebit, t = shape
    p = S.product_params(n, basebit, t)
    pk = PK.PackingKey(p, S.MASK_SEED, S.build_pack_bodies(n, basebit, t))
    rows = PK.key_rows(p, pk.mask_seed, pk.bodies)
    eng = R.Engine(p, 0)
    try:
        eng.load_packing_key(pk)
        cts = S.build_tlwe(n, basebit, t, max(S.PACK_COUNTS), 0)
        full = PK.pack_model(p, pk.mask_seed, pk.bodies, cts, rows=rows)  # [2][2][N]: a whole group and one of one input
        for count in S.PACK_COUNTS:
            # a group's words depend on its own inputs alone: the first whole group of the longest batch is shared
            exp = full[:count // N] if count % N == 0 else full if count == len(cts) else \
                PK.pack_model(p, pk.mask_seed, pk.bodies, cts[:count], rows=rows)
            got = eng.pack(cts[:count])
            assert got.shape == (-(-count // N), 2, N) and exp.any()
            assert np.array_equal(got, exp), (shape, count)
        for m in S.TABLE_MS:
            stage1 = S.build_tlwe(n, basebit, t, m * S.TABLE_COUNT, m).reshape(m, S.TABLE_COUNT, n + 1)
            exp = PK.table_model(p, pk.mask_seed, pk.bodies, stage1, m, rows=rows)
            assert np.array_equal(eng.pack_table(stage1, m), exp), (shape, m)
        with pytest.raises(_capi.TfheHipError, match="power of two"):  # W = 1: no half-box rotation
            eng.pack_table(np.zeros((S.TABLE_M_REFUSED, 1, n + 1), np.uint32), S.TABLE_M_REFUSED)
        # bodies 0x80000000 (every byte plane at its extreme), every digit -B/2: the largest accumulators of the shape
        adv = PK.PackingKey(p, bytes(range(40, 72)), np.full((n, t, N), 0x80000000, np.uint32))
        bt, half = basebit * t, (1 << basebit) // 2
        off = sum(half << (basebit * q) for q in range(t))
        word = (((1 << bt) - off) % (1 << bt)) << (32 - bt)  # a_bar + off = 0 (mod 2^bt)
        assert (PK.digits(p, np.array([word], np.uint32)) == -half).all()
        acts = np.full((N + 3, n + 1), word, np.uint32)
        acts[:, n] = 0x80000000
        eng.load_packing_key(adv)
        assert np.array_equal(eng.pack(acts), PK.pack_model(p, adv.mask_seed, adv.bodies, acts)), (shape, "adversarial")
    finally:
        eng.close()
