"""What a reach-eligible run clears in front of its first launch (PvAmdHostWindowClear, csrc/pv_core.cpp planClear) against a python
restatement, over every combination of its inputs.  No device."""
import itertools

NONE, RECT, ALL = 0, 1, 2
WIN = (4, 2, 7, 3)  # tile rows 4, 5 x tile columns 7, 8, 9
PREVIOUS = {"same": WIN, "other_origin": (3, 2, 7, 3), "other_size": (4, 2, 7, 2), "empty": (0, 0, 0, 0)}


def restated(window_run, win, prev, planes_dirty, swept_dirty, split_planes):
    if planes_dirty or swept_dirty:
        return ALL  # something other than the previous reach-eligible run wrote the planes
    if window_run and not split_planes and tuple(win) == tuple(prev) and win[1] > 0 and win[3] > 0:
        return NONE  # the resident kernel overwrites every cell of its window before it reads it
    return RECT  # (an empty rectangle: nothing to launch)


def test_every_combination(pvlib):
    none = []
    for (name, prev), planes_dirty, swept_dirty, split, window_run in itertools.product(PREVIOUS.items(), *[(False, True)] * 4):
        got = pvlib.host_window_clear(window_run, WIN, prev, planes_dirty, swept_dirty, split)
        assert got == restated(window_run, WIN, prev, planes_dirty, swept_dirty, split), (name, planes_dirty, swept_dirty, split, window_run)
        if got == NONE:
            none.append((name, planes_dirty, swept_dirty, split, window_run))
    assert none == [("same", False, False, False, True)]


def test_an_empty_window_is_never_the_same(pvlib):
    """a run without tiles equals an empty previous rectangle member by member: still a rectangle clear (of nothing)"""
    assert pvlib.host_window_clear(True, (0, 0, 0, 0), (0, 0, 0, 0), False, False, False) == RECT
    assert pvlib.host_window_clear(True, (2, 0, 5, 3), (2, 0, 5, 3), False, False, False) == RECT
