"""The segment plan of the tall-column tridiagonal solve (qgcm_hip_thomas_segments: pure host code of the library, no
device) and the resource report of the two kernels that run it.  CPU only."""
import os
import re

import pytest

from qgcm_hip import QgcmHipError, lib

MAXIMA = (0, 7, 8, 9, 16, 63, 64, 65, 100, 600, 640, 1000, 1024, 2047, 2048, 2049, 4096)


def _cap(nrows, max_rows):
    """The longest segment allowed: the given maximum (at most 2048); without one 2048 rows for the columns the
    single-segment kernel holds, THOMAS_SEG_DEFAULT beyond."""
    if max_rows > 0:
        return min(max_rows, lib.THOMAS_MAX_ROWS)
    return lib.THOMAS_MAX_ROWS if nrows <= lib.THOMAS_MAX_ROWS else lib.THOMAS_SEG_DEFAULT


def _check_plan(nrows, max_rows, plan):
    cap = _cap(nrows, max_rows)
    first = [f for f, _ in plan]
    count = [n for _, n in plan]
    # every row once, in order
    assert first[0] == 0 and sum(count) == nrows
    assert all(first[s + 1] == first[s] + count[s] for s in range(len(plan) - 1))
    assert max(count) - min(count) <= 1
    assert max(count) <= cap
    if len(plan) > 1:
        assert min(count) >= lib.THOMAS_SEG_MIN
        assert len(plan) == -(-nrows // cap)  # the fewest segments that respect the maximum
    if nrows <= cap:
        assert len(plan) == 1


@pytest.mark.parametrize("max_rows", MAXIMA)
def test_plan_covers_every_row_once(max_rows):
    for nrows in range(4, 5001):
        if -(-nrows // _cap(nrows, max_rows)) > lib.THOMAS_MAX_SEG:
            with pytest.raises(QgcmHipError):
                lib.thomas_segments(nrows, max_rows)
            continue
        _check_plan(nrows, max_rows, lib.thomas_segments(nrows, max_rows))


def test_plan_of_the_shipped_columns():
    assert lib.thomas_segments(2048) == [(0, 2048)]                      # up to 2048 rows: today's single launch
    assert lib.thomas_segments(2049) == [(0, 683), (683, 683), (1366, 683)]  # the first column past the limit
    assert [n for _, n in lib.thomas_segments(2399)] == [800, 800, 799]  # NAtl 2 km
    assert [n for _, n in lib.thomas_segments(4799)] == [960, 960, 960, 960, 959]  # NAtl 1 km
    assert [n for _, n in lib.thomas_segments(4799, 2048)] == [1600, 1600, 1599]
    assert [n for _, n in lib.thomas_segments(79, 30)] == [27, 26, 26]   # a maximum forces segments on a short column
    assert [n for _, n in lib.thomas_segments(4799, 640)] == [600] * 7 + [599]


def test_plan_refuses_what_it_cannot_keep():
    for bad in (1, 3, 6):  # two halves of a column of max + 1 rows would fall below the minimum
        with pytest.raises(QgcmHipError, match="segments of at least 4 rows"):
            lib.thomas_segments(100, bad)
    with pytest.raises(QgcmHipError):
        lib.thomas_segments(0)
    with pytest.raises(QgcmHipError, match="more than 64 segments"):
        lib.thomas_segments(5000, 7)


def test_segment_kernels_do_not_spill(repo_root):
    """The compiler's resource report (q-gcm_amd/csrc/Makefile): every instantiation of k_thomas_seg - 1 .. 32 rows per
    thread, the same set as k_thomas - and k_thomas_corr_seg use no scratch."""
    path = os.path.join(repo_root, "q-gcm_amd", "lib", "kernel_resources.txt")
    if not os.path.exists(path):
        pytest.fail("kernel_resources.txt missing - rebuild with `make -C q-gcm_amd/csrc`")
    res, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            res[cur] = int(m.group(1))
    want = ["_Z12k_thomas_segILi%dELi1ELi8EE" % r for r in (1, 2, 4, 8, 10, 12, 16, 20, 24, 32)] + ["_Z17k_thomas_corr_seg"]
    for h in want:
        hits = [k for k in res if k.startswith(h)]
        assert hits, "kernel %s not in the report" % h
        for k in hits:
            assert res[k] == 0, "%s spills %d B per lane" % (k, res[k])
