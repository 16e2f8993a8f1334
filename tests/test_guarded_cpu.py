"""The guarded-buffer helper (tests/guarded.py) on CPU tensors: that it places arrays where it says, and that it catches what
tests/test_gpu_guarded_buffers.py relies on it to catch — a store one word before or after an array, and a read of one
element too many.  The stray accesses are plain torch operations on the arena; no kernel of the library is involved."""
import numpy as np
import pytest
import torch

from guarded import FILLS, FLOAT_WORDS, GUARD, SKEWS, TAIL, Arena, Plain, placements, worst_residue


def _arena(skew="aligned", fill=0, nbytes=1 << 16):
    return Arena(nbytes, "cpu", skew, fill)


def _place_some(a):
    x = a.place("x", np.arange(771, dtype=np.float32))
    idx = a.place("idx", np.arange(65, dtype=np.int32), guard=(0, 64))
    mask = a.place("mask", np.ones(63, np.uint8), guard=(0, 1))
    tot = a.place("total", (1,), torch.int64, align=8, role="out")
    rot = a.place("rot", np.ones((257, 4), np.float32), align=16)
    y = a.place("y", (3, 5), torch.float32, role="out")
    return dict(x=x, idx=idx, mask=mask, total=tot, rot=rot, y=y)


def test_alignment_classes_of_place():
    for fill in FILLS:
        a = _arena("aligned", fill)
        for name in _place_some(a):
            assert a.address_of(name) % 16 == 0, name
        w = _arena("worst", fill)
        t = _place_some(w)
        assert w.address_of("x") % 16 == 4          # 4-byte elements, no documented requirement
        assert w.address_of("idx") % 16 == 4
        assert w.address_of("mask") % 2 == 1        # a uint8 mask: an odd address
        assert w.address_of("total") % 16 == 8      # 8 bytes documented: exactly that and no more
        assert w.address_of("rot") % 32 == 16       # 16 bytes documented: exactly that and no more
        assert w.address_of("y") % 16 == 4
        for name, v in t.items():
            assert v.data_ptr() == w.address_of(name) and v.is_contiguous()
    assert worst_residue(4) == (16, 4) and worst_residue(8) == (16, 8) and worst_residue(1) == (16, 1)
    assert worst_residue(4, 16) == (32, 16) and worst_residue(4, 8) == (16, 8) and worst_residue(8, 8) == (16, 8)
    # an explicit skew on one placement overrides the arena's
    a = _arena("worst")
    a.place("p", (5,), torch.float32, skew="aligned")
    assert a.address_of("p") % 16 == 0


def test_layout_guards_touch_the_data_and_the_end_is_not_rounded():
    for skew in SKEWS:
        a = _arena(skew, 1)
        a.place("x", np.zeros(771, np.float32))
        a.place("m", np.zeros(63, np.uint8), guard=(0, 1))
        rx, rm = a.records
        assert rx["end"] - rx["start"] == 3084 and rm["end"] - rm["start"] == 63
        raw = a.mem.numpy()
        # the byte right after the 771st float, and the one right before the first, are guard
        word = np.frombuffer(raw[rx["end"]:rx["end"] + 4].tobytes(), np.uint32)[0]
        assert word == FLOAT_WORDS[1]
        assert np.frombuffer(raw[rx["start"] - 4:rx["start"]].tobytes(), np.uint32)[0] == FLOAT_WORDS[1]
        assert raw[rm["end"]] == 1 and raw[rm["start"] - 1] == 1
        assert rx["start"] - rx["lo"] >= GUARD and rx["hi"] - rx["end"] >= GUARD
        assert rm["start"] - rx["end"] >= 2 * GUARD        # each array has guards of its own
        assert a.nbytes - rm["hi"] >= TAIL                 # the arena's own tail
        assert a.check() == []
    with pytest.raises(RuntimeError):
        _arena(nbytes=4096).place("big", (2000,), torch.float32)


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("fill", FILLS)
def test_store_one_word_past_and_one_word_before_is_reported(skew, fill):
    a = _arena(skew, fill)
    t = _place_some(a)
    assert a.check() == []
    r = next(r for r in a.records if r["name"] == "x")
    words = a.mem[r["start"] - 4:r["end"] + 4].view(torch.float32)   # the array as a kernel with a wrong bound sees it
    words[1 + 771] = 5.0                                            # x[771]: one word past the end
    assert a.check() == [dict(name="x", side="after", offset=3084, words=1)]
    a.mem[r["end"]:r["end"] + 4] = torch.from_numpy(a.host[r["end"]:r["end"] + 4].copy())   # repair
    assert a.check() == []
    words[0] = 5.0                                                  # x[-1]: one word before the first
    assert a.check() == [dict(name="x", side="before", offset=-4, words=1)]
    a.mem[r["start"] - 4:r["start"]] = torch.from_numpy(a.host[r["start"] - 4:r["start"]].copy())
    # a byte mask written one byte too far, and a three-word overrun of the 16-byte aligned rows
    m = next(r for r in a.records if r["name"] == "mask")
    a.mem[m["end"]] = 7
    q = next(r for r in a.records if r["name"] == "rot")
    a.mem[q["end"] + 8:q["end"] + 20] = 0x11
    assert a.check() == [dict(name="mask", side="after", offset=63, words=1),
                         dict(name="rot", side="after", offset=257 * 16 + 8, words=3)]
    # the data itself is never a finding
    t["x"].fill_(9.0)
    t["y"].fill_(1.0)
    assert [d["name"] for d in a.check()] == ["mask", "rot"]


def test_store_into_the_arena_tail_is_reported():
    a = _arena()
    _place_some(a)
    a.mem[a.nbytes - 8] = 0
    found = a.check()
    assert len(found) == 1 and found[0]["name"] == "<arena tail>"


@pytest.mark.parametrize("skew", SKEWS)
def test_reduction_over_one_element_too_many_differs_between_the_fills(skew):
    """What makes an over-READ visible: the two guard fills give different bits, float and integer alike; the slice of the
    right length does not."""
    res = {}
    for fill in FILLS:
        a = _arena(skew, fill)
        t = _place_some(a)
        rx = next(r for r in a.records if r["name"] == "x")
        ri = next(r for r in a.records if r["name"] == "idx")
        x_long = a.mem[rx["start"]:rx["end"] + 4].view(torch.float32)        # 772 elements of a 771-element array
        i_long = a.mem[ri["start"]:ri["end"] + 4].view(torch.int32)          # 66 of 65
        i_before = a.mem[ri["start"] - 4:ri["end"]].view(torch.int32)        # starts one element early
        assert int(i_long[-1]) == (0, 64)[fill] and int(i_before[0]) == (0, 64)[fill]   # in range, never a poison word
        res[fill] = dict(ok=t["x"].sum().view(torch.int32).item(), long=x_long.max().view(torch.int32).item(),
                         iok=int(t["idx"].sum()), ilong=int(i_long.sum()), ibefore=int(i_before.sum()))
        assert a.check() == []
        a.assert_inputs_unchanged()
    assert res[0]["ok"] == res[1]["ok"] and res[0]["iok"] == res[1]["iok"]
    assert res[0]["long"] != res[1]["long"]
    assert res[0]["ilong"] != res[1]["ilong"] and res[0]["ibefore"] != res[1]["ibefore"]


def test_untouched_arena_reports_nothing_and_inputs_are_watched():
    for p in placements(1 << 16, "cpu"):
        t = _place_some(p)
        t["y"].fill_(3.0)            # outputs may be written
        t["total"].fill_(12)
        assert p.check() == []
        p.assert_inputs_unchanged()
        t["idx"][64] = 3             # ... a const input may not
        with pytest.raises(AssertionError, match="idx"):
            p.assert_inputs_unchanged()
    assert isinstance(next(iter(placements(1 << 12, "cpu"))), Plain)


def test_inout_buffers_are_not_held_to_their_first_contents():
    a = _arena("worst", 1)
    v = a.place("theta", np.ones(65, np.float32), role="inout")
    v.mul_(2.0)
    a.assert_inputs_unchanged()
    assert a.check() == []
