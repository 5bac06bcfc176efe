"""Every buffer, arena and timing event a context makes goes back with it (csrc/resources.hpp, on the GPU): the
create / use / destroy cycle of test_gpu_parity.py::test_contexts_views_and_pools_give_their_memory_back, extended to the
buffers that test never allocates -- the key switch's device output and digit scratch, the tree bootstrap's two
scratches, the public key and its selector scratch, the staged secrets -- with profiling on and the timing pairs never
collected."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1024


def _words(shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def _cycle(P, k0, k1, cts):
    import rs_tfhe_amd as R
    from rs_tfhe_amd.engine import NAND, XOR, _ptr, pinned_empty

    w = P.n + 1
    eng = R.Engine(P, 0)
    eng.set_profiling(True)  # (an event pair per launch; nobody collects them)
    eng.gen_cloud_key(k0, k1, seed=20)
    # one workgroup per ciphertext, two, the batch kernel; at basebit 4 the last one runs the column-sliced key switch
    # on its digit scratch (from 384 ciphertexts up)
    for count in (1, 300, 1100):
        eng.batch_gate(NAND, cts[0][:count], cts[1][:count])
    # every operand pinned: the kernels write the caller's memory, and a key switch that merges partial sums does so
    # through the context's device output
    pa, pb, po = pinned_empty((300, w)), pinned_empty((300, w)), pinned_empty((300, w))
    pa[:], pb[:] = cts[0][:300], cts[1][:300]
    eng.batch_gate(NAND, pa, pb, out=po)
    lv1, ks = pinned_empty((300, N + 1)), pinned_empty((300, w))
    lv1[:] = _words((300, N + 1), 3)
    eng._chk(eng._lib.tfhe_hip_batch_identity_key_switch(eng._ctx, _ptr(lv1), _ptr(ks), 300))
    # tree bootstrap, m = 2 on 3 ciphertexts (its two scratches; the packing key)
    eng.gen_packing_key(k0, k1, rng_key=bytes(range(32)), download=False)
    eng.batch_bootstrap_bivariate(cts[0][:3], cts[1][:3], _words((2, 2, N), 4), 2)
    # public key and its selector scratch; symmetric encryption (the staged secrets)
    eng.gen_public_key(k0, rng_key=bytes(range(1, 33)), download=False)
    eng.batch_pk_encrypt(_words(5, 5), P.alpha_lv0, bytes(range(2, 34)))
    eng.batch_encrypt(k0, _words(5, 6), rng_key=bytes(range(3, 35)), mask_seed=bytes(range(4, 36)))
    view = eng.new_key_view()
    view.gen_cloud_key(k0, k1, seed=21)
    view.batch_gate(XOR, cts[0][:5], cts[1][:5])
    view.close()
    eng.close()


@pytest.mark.parametrize("basebit", [None, 4], ids=["toy", "toy-basebit4"])
def test_a_context_gives_every_buffer_back(golden, basebit):
    import torch

    from rs_tfhe_amd.params import SecurityParams

    n, l, bgbit, bb, t = (int(v) for v in golden["toy"]["params"])
    P = SecurityParams("TOY_RESOURCES", 0, n, l, bgbit, bb if basebit is None else basebit, t, 2.0e-5, 2.0e-8)
    rng = np.random.default_rng(20)
    k0, k1 = rng.integers(0, 2, n).astype(np.uint32), rng.integers(0, 2, N).astype(np.uint32)
    cts = _words((2, 1100, n + 1), 7)
    _cycle(P, k0, k1, cts)  # first use pays for lazily created runtime state (streams, module load)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    for _ in range(3):
        _cycle(P, k0, k1, cts)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(0)
    print(f"free before {free0}, after {free1}: {free0 - free1} bytes not returned")
    assert free0 - free1 < 8 << 20, f"{(free0 - free1) >> 20} MiB not returned after three create/destroy cycles"
