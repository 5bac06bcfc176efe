"""Framed operands for the device-pointer calls (used by tests/test_dev_buffers_host.py on the CPU, by
tests/test_gpu_dev_buffers.py on the HIP kernels and by tests/test_gpu_sym_encrypt.py).  No tests here and no device
import: torch is imported inside the functions, and a frame lives wherever `device` says.

A call's operand usually sits at the start of a fresh allocation: 512-byte aligned, exactly sized, with whatever the
allocator left behind it.  A frame puts it `offset` elements into a larger buffer instead, between two pads of PAD
elements, so that

  * the operand starts at any word of a 16-byte chunk (any byte, for an int8 operand);
  * an OUTPUT frame holds SENTINEL in both pads and in the output itself: a store outside the output changes a pad, a
    word the call leaves unwritten (or a kernel that adds into an output it takes for zero) shows in the comparison
    with the expected words;
  * an INPUT frame holds POISON in both pads (0xFFFFFFFF / 0x80000000 alternating, -128 / 127 for bytes: the words
    tests/test_gpu_conv2d.plant uses): a read outside the operand that is USED moves the result by 2^31 times a
    coefficient.  A read that is not used cannot be seen, and is not looked for.

PAD is one TRLWE: wider than any tile or vector store in the tree.
"""
from collections import namedtuple

import numpy as np

PAD = 2048
SENTINEL = 0x5A5AA5A5
POISON = (0xFFFFFFFF, 0x80000000)
POISON8 = (-128, 127)
SHOWN = 4  # positions a report lists

# One run's offsets, in elements of the operand: every 32-bit operand of a run starts `words` (inputs) / `out` (the
# output) words into a 16-byte chunk, an int8 operand (weights, gate codes) `bytes8` bytes.  Every operand at the same
# word 0 .. 3, one mixed run, and one with the bytes alone off by one.
Plan = namedtuple("Plan", "name words out bytes8")
PLANS = (Plan("all0", 0, 0, 0), Plan("all1", 1, 1, 5), Plan("all2", 2, 2, 10), Plan("all3", 3, 3, 15),
         Plan("in1_out3", 1, 3, 7), Plan("bytes1", 0, 0, 1))
WORD_PLANS = PLANS[:5]  # what a call without an int8 operand runs


def plan_id(p):
    return p.name


def _torch_dtype(dtype):
    import torch

    return {1: torch.int8, 4: torch.int32}[np.dtype(dtype).itemsize]


def fill_pattern(count, fill, itemsize, first=0):
    """`count` elements of a fill as the signed numpy type a torch tensor of that width holds, element i of the big
    buffer being entry `first` + i of the pattern"""
    if itemsize == 1:
        lo, hi = (np.int8(POISON8[0]), np.int8(POISON8[1])) if fill == "poison" else (np.int8(0x5A), np.int8(0x5A))
        return np.where((np.arange(count) + first) % 2 == 0, lo, hi).astype(np.int8)
    lo, hi = POISON if fill == "poison" else (SENTINEL, SENTINEL)
    return np.where((np.arange(count) + first) % 2 == 0, np.uint32(lo), np.uint32(hi)).astype(np.uint32).view(np.int32)


def frame(array, offset, pad=PAD, fill="poison", device="cuda"):
    """(big, view): `big` a 1-D tensor of pad + offset + size + pad elements of `array`'s width on `device`, 16-byte
    aligned; `view` the contiguous view of array's shape that starts pad + offset elements in.  fill "poison": an
    input frame, the view holds array's values; fill "sentinel": an output frame, every element of big (the view's
    included) is the sentinel and `array` gives the shape and the width alone."""
    import torch

    array = np.asarray(array)
    itemsize = array.dtype.itemsize
    assert itemsize in (1, 4) and fill in ("poison", "sentinel") and offset >= 0
    size, start = array.size, pad + offset
    host = fill_pattern(pad + offset + size + pad, fill, itemsize)
    if fill == "poison":
        host[start:start + size] = np.ascontiguousarray(array).reshape(-1).view(host.dtype)
    big = torch.from_numpy(host).to(device)
    assert big.data_ptr() % 16 == 0 and big.dtype == _torch_dtype(array.dtype)
    view = big[start:start + size].view(array.shape)
    assert view.data_ptr() == big.data_ptr() + start * itemsize and view.is_contiguous()
    return big, view


def host_words(big):
    """The elements of a frame (a tensor anywhere, or a numpy array in pinned memory) as a flat signed numpy array"""
    if isinstance(big, np.ndarray):
        a = big.reshape(-1)
        return a.view(np.int8 if a.dtype.itemsize == 1 else np.int32)
    return big.detach().cpu().numpy().reshape(-1)


def view_words(big, view_span, dtype=np.uint32):
    """The view's elements out of a frame, flat, as `dtype`"""
    start, size = view_span
    return host_words(big)[start:start + size].copy().view(dtype)


def check_frame(big, view_span, fill, name="frame"):
    """What of `big` outside the view (start, size) differs from `fill`: "" when nothing does, else a message with the
    number of elements, the side that was touched, how far from the view's edge the nearest one lies, and the first few
    positions relative to that edge."""
    start, size = view_span
    words = host_words(big)
    want = fill_pattern(len(words), fill, words.dtype.itemsize)
    said = []
    before = np.flatnonzero(words[:start] != want[:start])
    if len(before):
        dist = start - before  # 1 = the element just before the view's first
        said.append(f"{len(before)} element(s) BEFORE the start touched, the nearest {int(dist.min())} before the first "
                    f"element of the view (at -{', -'.join(str(int(d)) for d in dist[::-1][:SHOWN])})")
    end = start + size
    after = np.flatnonzero(words[end:] != want[end:])
    if len(after):
        dist = after + 1  # 1 = the element just past the view's last
        said.append(f"{len(after)} element(s) AFTER the end touched, the nearest {int(dist.min())} past the last "
                    f"element of the view (at +{', +'.join(str(int(d)) for d in dist[:SHOWN])})")
    return f"{name}: " + "; ".join(said) if said else ""


def span(big, view):
    """(start, size) of a view inside its frame, in elements"""
    itemsize = view.element_size()
    start = (view.data_ptr() - big.data_ptr()) // itemsize
    return int(start), int(view.numel())


class Framed:
    """The operands of one call under one plan: inputs by name (numpy arrays, None left out) in poison frames, the
    output in a sentinel frame -- or several outputs, as a dict name -> array of the shape.  `views` is what the call
    takes (inputs), `out` the output view (`outs[name]` with several); check() is the four assertions.  `at` names
    operands ("out", or an output's name) whose offset is given in elements instead of taken from the plan."""

    def __init__(self, inputs, out_like, plan, device="cuda", pad=PAD, at=None):
        at = at or {}
        self.inputs = {k: np.ascontiguousarray(v) for k, v in inputs.items() if v is not None}
        self.frames, self.views = {}, {k: None for k in inputs}
        for k, v in self.inputs.items():
            off = at.get(k, plan.bytes8 if v.dtype.itemsize == 1 else plan.words)
            self.frames[k], self.views[k] = frame(v, off, pad, "poison", device)
        self.single = not isinstance(out_like, dict)
        self.out_frames, self.outs = {}, {}
        for k, like in ({"out": out_like} if self.single else out_like).items():
            self.out_frames[k], self.outs[k] = frame(like, at.get(k, plan.out), pad, "sentinel", device)
        self.out_big, self.out = next(iter(self.out_frames.values())), next(iter(self.outs.values()))
        self.plan = plan

    def output_words(self, dtype=np.uint32, name=None):
        name = next(iter(self.outs)) if name is None else name
        big, view = self.out_frames[name], self.outs[name]
        return view_words(big, span(big, view), dtype).reshape(tuple(view.shape))

    def damage(self):
        """every frame's report: pads of the outputs, pads of the inputs, the inputs themselves"""
        said = [check_frame(big, span(big, self.outs[k]), "sentinel", "output" if self.single else f"output {k}")
                for k, big in self.out_frames.items()]
        for k, big in self.frames.items():
            sp = span(big, self.views[k])
            said.append(check_frame(big, sp, "poison", f"input {k}"))
            if not np.array_equal(view_words(big, sp, self.inputs[k].dtype), self.inputs[k].reshape(-1)):
                said.append(f"input {k}: the operand itself was changed")
        return [s for s in said if s]

    def check(self, expected, label=""):
        """the output views hold `expected` (an array, or a dict by output name), and nothing else moved"""
        for k, want in ({next(iter(self.outs)): expected} if self.single else expected).items():
            want = np.asarray(want)
            got = self.output_words(want.dtype, k)
            differing = int((got != want).sum())
            unwritten = int((got.view(np.uint32) == np.uint32(SENTINEL)).sum()) if got.dtype.itemsize == 4 else 0
            assert differing == 0, (f"{label} [{self.plan.name}]: {differing} of {got.size} output words differ from the CPU's "
                                    f"({unwritten} still hold the sentinel), first at {np.argwhere(got != want)[:SHOWN].tolist()}")
        said = self.damage()
        assert not said, f"{label} [{self.plan.name}]: " + " | ".join(said)

    def check_untouched(self, label=""):
        """after a refused call: the outputs still hold the sentinel everywhere, and nothing else moved"""
        said = [check_frame(big, (span(big, self.outs[k])[0], 0), "sentinel", "output (refused call)")
                for k, big in self.out_frames.items()] + self.damage()
        said = [s for s in said if s]
        assert not said, f"{label} [{self.plan.name}]: " + " | ".join(said)
