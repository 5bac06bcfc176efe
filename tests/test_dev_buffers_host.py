"""The framing harness of tests/dev_buffers.py proved on the CPU, and the coverage check of tests/test_gpu_dev_buffers.py.

Stand-in "kernels" written in torch on CPU tensors run through the same Framed operands the GPU file uses: a correct one
passes under every offset plan, and four planted defects -- a store one word past the end, one before the start, a last
word left unwritten, a neighbouring input word added into the result -- are each caught, with the side and the distance
in the message.  The coverage check parses include/tfhe_hip.h: every device-pointer entry point of a context must be a
key of the GPU file's CALLS table, so a later `_dev` call that nobody framed fails here."""
import os
import re

import numpy as np
import pytest

import dev_buffers as DB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, WIDTH = 5, 67  # rows of 67 words: they start at every word of a 16-byte chunk


def _operands(seed=3):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 32, (ROWS, WIDTH), dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, (ROWS, WIDTH), dtype=np.uint64).astype(np.uint32)
    w = rng.integers(-128, 128, (ROWS,)).astype(np.int8)
    with np.errstate(over="ignore"):
        want = (a * np.uint32(3) + b + w.astype(np.int32).view(np.uint32)[:, None]).astype(np.uint32)
    return {"a": a, "b": b, "w": w}, want


def _flat_from(view, count, back=0):
    """`count` elements of the storage from `back` elements before the view's first: how a defective kernel reaches
    outside its operand"""
    import torch

    return torch.as_strided(view, (count,), (1,), view.storage_offset() - back)


def standin(f, defect=None):
    """out = 3 a + b + w[row] (wrapping) on the framed views"""
    a, b, w, out = f.views["a"], f.views["b"], f.views["w"], f.out
    res = a * 3 + b + w.to(a.dtype)[:, None]
    if defect == "neighbour":  # the last word also takes the input word behind the operand
        res.view(-1)[-1] += _flat_from(a, a.numel() + 1)[-1]
    if defect == "unwritten":
        out.view(-1)[:-1] = res.view(-1)[:-1]
        return
    out.copy_(res)
    if defect == "past_end":
        _flat_from(out, out.numel() + 1)[-1] = 7
    if defect == "before_start":
        _flat_from(out, 1, back=1)[0] = 7


@pytest.mark.parametrize("plan", DB.PLANS, ids=DB.plan_id)
def test_a_correct_standin_passes_under_every_plan(plan):
    inputs, want = _operands()
    f = DB.Framed(inputs, want, plan, device="cpu")
    assert f.out.data_ptr() % 16 == (4 * plan.out) % 16 and f.views["a"].data_ptr() % 16 == (4 * plan.words) % 16
    assert f.views["w"].data_ptr() % 16 == plan.bytes8 % 16
    assert (f.output_words() == DB.SENTINEL).all()  # the output itself starts as the sentinel
    standin(f)
    f.check(want, "stand-in")


@pytest.mark.parametrize("plan", DB.WORD_PLANS, ids=DB.plan_id)
@pytest.mark.parametrize("defect,said", [
    ("past_end", r"output: 1 element\(s\) AFTER the end touched, the nearest 1 past the last element of the view \(at \+1\)"),
    ("before_start", r"output: 1 element\(s\) BEFORE the start touched, the nearest 1 before the first element of the view \(at -1\)"),
    ("unwritten", r"1 of 335 output words differ from the CPU's \(1 still hold the sentinel\), first at \[\[4, 66\]\]"),
    ("neighbour", r"1 of 335 output words differ from the CPU's \(0 still hold the sentinel\), first at \[\[4, 66\]\]"),
])
def test_each_planted_defect_is_caught(plan, defect, said):
    inputs, want = _operands()
    f = DB.Framed(inputs, want, plan, device="cpu")
    standin(f, defect)
    with pytest.raises(AssertionError, match=said):
        f.check(want, "stand-in")


def test_far_stores_and_changed_inputs_are_reported():
    """a store 2048 elements out, on both sides at once, and a kernel that writes its input"""
    inputs, want = _operands()
    f = DB.Framed(inputs, want, DB.PLANS[1], device="cpu")
    standin(f)
    start, size = DB.span(f.out_big, f.out)
    f.out_big[0] = 1
    f.out_big[start + size + 9] = 1
    f.out_big[-1] = 1
    msg = DB.check_frame(f.out_big, (start, size), "sentinel", "output")
    assert f"1 element(s) BEFORE the start touched, the nearest {start} before" in msg
    assert f"2 element(s) AFTER the end touched, the nearest 10 past the last element of the view (at +10, +{DB.PAD})" in msg
    f.views["b"][2, 3] += 1
    a_big = f.frames["a"]
    a_big[DB.span(a_big, f.views["a"])[0] - 2] = 0
    with pytest.raises(AssertionError, match=r"input a: 1 element\(s\) BEFORE the start touched, the nearest 2 before.*"
                                             r"input b: the operand itself was changed"):
        f.check(want, "stand-in")


def test_a_refused_call_must_leave_everything():
    inputs, want = _operands()
    f = DB.Framed(inputs, want, DB.PLANS[2], device="cpu")
    f.check_untouched("refused")
    f.out[0, 0] = 1
    with pytest.raises(AssertionError, match="output \\(refused call\\)"):
        f.check_untouched("refused")


def test_poison_is_the_conv2d_plant_pattern():
    big, view = DB.frame(np.zeros(3, np.uint32), 1, pad=4, device="cpu")
    assert big.numpy().view(np.uint32).tolist() == [0xFFFFFFFF, 0x80000000, 0xFFFFFFFF, 0x80000000, 0xFFFFFFFF, 0, 0, 0,
                                                    0xFFFFFFFF, 0x80000000, 0xFFFFFFFF, 0x80000000]
    big8, view8 = DB.frame(np.ones((2, 2), np.int8), 3, pad=2, device="cpu")
    assert big8.numpy().tolist() == [-128, 127, -128, 127, -128, 1, 1, 1, 1, 127, -128] and view8.shape == (2, 2)


# ---- coverage: every device-pointer entry point of a context is framed ----------------------------------------------------
def dev_entry_points():
    """tfhe_hip_*_dev prototypes of include/tfhe_hip.h that are not a pool's, the circuit's two among them"""
    text = open(os.path.join(ROOT, "include", "tfhe_hip.h")).read()
    names = set(re.findall(r"^int (tfhe_hip_\w+_dev)\s*\(", text, re.M))
    return sorted(n for n in names if not n.startswith("tfhe_hip_pool_") and "_pool_" not in n)


def test_every_dev_entry_point_is_in_the_gpu_files_table():
    from test_gpu_dev_buffers import CALLS  # (importing the GPU file opens no device)

    names = dev_entry_points()
    assert len(names) >= 30 and "tfhe_hip_circuit_run_dev" in names and "tfhe_hip_circuit_gather_dev" in names
    assert "tfhe_hip_batch_gate_dev" in names and not any("pool" in n for n in names)
    missing = [n for n in names if n not in CALLS]
    assert not missing, f"device-pointer entry points without a framed case in tests/test_gpu_dev_buffers.py: {missing}"
    stale = [n for n in CALLS if n not in names]
    assert not stale, f"CALLS names what the header does not declare: {stale}"
