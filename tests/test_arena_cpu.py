"""The guarded-buffer checker of tests/arena.py on numpy arenas: it can fail.  One element written into a guard is reported, one
body element left alone is reported, a clean fill passes -- for every output dtype, in front of and behind the body."""
import numpy as np
import pytest

from arena import GUARD, SENTINELS, Arena, ArenaAllocator, Frame, bits, check_guards, check_untouched, check_written, input_arena, output_arena

DTYPES = [np.float32, np.float64, np.int32, np.int64, np.uint8]


def _value(dtype):
    return np.arange(1, 38).astype(dtype) if np.dtype(dtype).kind != "f" else np.linspace(-3.0, 3.0, 37).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_guard_size_and_alignment(dtype):
    a = output_arena((37,), dtype)
    assert a.lo >= GUARD and a.raw.size - a.hi >= GUARD
    assert a.body_address % 16 == 0 and a.body.ctypes.data == a.body_address
    assert a.body.shape == (37,) and a.body.dtype == np.dtype(dtype)
    assert (a.ints() == SENTINELS[np.dtype(dtype)][1]).all()           # body and guards
    shifted = output_arena((37,), dtype, shift=1)
    assert shifted.body_address % 16 == np.dtype(dtype).itemsize % 16 and shifted.lo >= GUARD
    two = output_arena((5, 3), dtype)
    assert two.body.shape == (5, 3) and two.hi - two.lo == 15


def test_float_sentinels_are_quiet_nans_with_a_payload():
    for dt in (np.float32, np.float64):
        a = output_arena((4,), dt)
        assert np.isnan(a.body).all()
        assert not (bits(a.body) == bits(np.full(4, np.nan, dtype=dt))).any()      # not the NaN arithmetic produces


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_clean_fill_passes(dtype):
    a = output_arena((37,), dtype)
    a.body[:] = _value(dtype)
    check_guards(a)
    check_written(a)
    assert np.array_equal(a.host(), _value(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["front", "behind", "far_front", "far_behind"])
def test_one_element_written_into_a_guard_is_reported(dtype, where):
    a = output_arena((37,), dtype)
    a.body[:] = _value(dtype)
    i = {"front": a.lo - 1, "behind": a.hi, "far_front": 0, "far_behind": a.raw.size - 1}[where]
    a.raw[i] = 1
    check_written(a)
    with pytest.raises(AssertionError, match="guard elements"):
        check_guards(a, "case")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("index", [0, 17, 36])
def test_one_unwritten_body_element_is_reported(dtype, index):
    a = output_arena((37,), dtype)
    v = _value(dtype)
    keep = np.ones(37, dtype=bool)
    keep[index] = False
    a.body[keep] = v[keep]
    check_guards(a)
    with pytest.raises(AssertionError, match=f"never written; first \\[{index}\\]"):
        check_written(a, "case")
    check_written(a, "case", defined=keep)                              # ... unless the contract leaves that element out


def test_a_nan_result_is_written_and_the_sentinel_is_not():
    a = output_arena((8,), np.float64)
    a.body[:] = np.nan                                                  # what a failed group's rows hold: a NaN, not the sentinel
    check_written(a)


def test_a_rejected_call_leaves_everything():
    a = output_arena((8,), np.float32)
    check_untouched(a)
    a.body[3] = 0.0
    with pytest.raises(AssertionError, match="rejected call"):
        check_untouched(a)


def test_input_arena_and_frame_guards():
    x = np.linspace(0.0, 1.0, 11)
    a = input_arena(x, np.nan)
    assert np.array_equal(a.body, x) and np.isnan(a.raw[:a.lo]).all() and np.isnan(a.raw[a.hi:]).all()
    a.fill_guards(7.0)
    assert np.array_equal(a.body, x) and (a.raw[:a.lo] == 7.0).all() and (a.raw[a.hi:] == 7.0).all()
    fr = Frame(x, [x + 1, x + 2], [0, 4, 11], w=x + 3, valid=np.ones(11, dtype=np.uint8), extra={"z": [x + 4]}, device=False)
    assert all(np.isnan(c.raw[:c.lo]).all() for c in fr.floats()) and (fr._valid.raw[:fr._valid.lo] == 0).all()
    fr.guards(7.0)
    assert all((c.raw[c.hi:] == 7.0).all() for c in fr.floats()) and (fr._valid.raw[fr._valid.hi:] == 1).all()
    assert np.array_equal(fr.cols[1], x + 2) and np.array_equal(fr.extra("z")[0], x + 4) and np.array_equal(fr.w, x + 3)
    assert all(c.body_address % 16 == 0 for c in fr.floats() + [fr._valid])


def test_allocator_hands_the_same_arenas_to_the_next_call():
    al = ArenaAllocator()
    al.begin()
    c = al(False, np.float64, (3, 2))
    s = al(False, np.int32, (3,))
    c[:] = 1.0
    with pytest.raises(AssertionError, match="never written"):           # status was left alone
        al.check("first")
    s[:] = 0
    al.check("first")
    al.begin()
    c2, s2 = al(False, np.float64, (3, 2)), al(False, np.int32, 3)
    assert c2.ctypes.data == c.ctypes.data and s2.ctypes.data == s.ctypes.data
    with pytest.raises(AssertionError, match="never written"):           # re-armed: the previous call's values are gone
        al.check("second")


def test_allocator_as_an_instance_attribute():
    """an ArenaAllocator assigned to the instance shadows the class's method and is called without self, as arena_engine() relies on"""
    al = ArenaAllocator()

    class Probe:                                                        # what Engine.plan_least_squares does with self._alloc
        _alloc = None

        def outputs(self, G, N, kt):
            return self._alloc(False, np.float64, (G, kt), None), self._alloc(False, np.float64, (N,), None)

    p = Probe()
    p._alloc = al
    al.begin()
    coef, pred = p.outputs(2, 9, 3)
    coef[:], pred[:] = 0.0, 0.0
    al.check()
    pred[-1:] = al.arenas[1].raw[al.arenas[1].hi:al.arenas[1].hi + 1]    # the sentinel copied back in: reported
    with pytest.raises(AssertionError, match="never written"):
        al.check()
