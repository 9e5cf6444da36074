"""list_hourly_index_directories against a temporary tree: the restatement of
HourlyDirectoryWithSuccessFileListing.listHourlyIndexDirectories (one hour back per step, every step costs an attempt, a
directory counts if its _SUCCESS can be read, newest first).  Host only."""
import datetime as dt
import os

import pytest

UTC = dt.timezone.utc


def _hour(root, t, success=True):
    d = os.path.join(root, t.strftime("%Y/%m/%d/%H"))
    os.makedirs(d)
    if success:
        open(os.path.join(d, "_SUCCESS"), "wb").close()
    return d


def test_missing_hours_are_skipped_but_cost_attempts(pkg, tmp_path):
    ls = pkg.faiss_files.list_hourly_index_directories
    root = str(tmp_path)
    now = dt.datetime(2023, 3, 14, 15, 26, 53, tzinfo=UTC)
    h = lambda k: now - dt.timedelta(hours=k)
    d0, d2, d5 = _hour(root, h(0)), _hour(root, h(2)), _hour(root, h(5))
    assert d0.endswith("2023/03/14/15")
    assert ls(root, now, 3, 24) == [d0, d2, d5]  # newest first, hours 1, 3, 4 skipped
    assert ls(root, now, 2, 24) == [d0, d2]      # count caps the result
    assert ls(root, now, 3, 5) == [d0, d2]       # 5 attempts reach hour 4: the lookback is exhausted before hour 5
    assert ls(root, now, 3, 6) == [d0, d2, d5]
    assert ls(root, now, 3, 1) == [d0]
    assert ls(root, now, 3, 0) == [] and ls(root, now, 0, 24) == []
    assert ls(root, h(1), 3, 24) == [d2, d5]     # starting one hour earlier
    # seconds since the epoch and a naive datetime (taken as UTC) name the same hour
    assert ls(root, now.timestamp(), 1, 1) == [d0]
    assert ls(root, now.replace(tzinfo=None), 1, 1) == [d0]
    # another time zone is converted: 17:26 at +02:00 is 15:26 UTC
    assert ls(root, now.astimezone(dt.timezone(dt.timedelta(hours=2))), 1, 1) == [d0]


def test_a_directory_without_success_file_is_skipped(pkg, tmp_path):
    ls = pkg.faiss_files.list_hourly_index_directories
    root = str(tmp_path)
    now = dt.datetime(2023, 3, 14, 15, 0, 0, tzinfo=UTC)
    h = lambda k: now - dt.timedelta(hours=k)
    d0 = _hour(root, h(0), success=False)
    open(os.path.join(d0, "faiss.index"), "wb").close()  # the index file alone does not make the hour count
    d1 = _hour(root, h(1))
    d2 = _hour(root, h(2))
    os.mkdir(os.path.join(_hour(root, h(3), success=False), "_SUCCESS"))  # a directory named _SUCCESS is no success file
    d4 = _hour(root, h(4))
    assert ls(root, now, 3, 24) == [d1, d2, d4]
    assert ls(root, now, 3, 3) == [d1, d2]


def test_crossing_day_month_and_year(pkg, tmp_path):
    ls = pkg.faiss_files.list_hourly_index_directories
    root = str(tmp_path)
    now = dt.datetime(2024, 1, 1, 0, 10, 0, tzinfo=UTC)
    d0 = _hour(root, now)
    d1 = _hour(root, dt.datetime(2023, 12, 31, 23, 0, tzinfo=UTC))
    d2 = _hour(root, dt.datetime(2023, 12, 31, 22, 0, tzinfo=UTC))
    assert (d0[-13:], d1[-13:], d2[-13:]) == ("2024/01/01/00", "2023/12/31/23", "2023/12/31/22")
    assert ls(root, now, 3, 3) == [d0, d1, d2]
    # the first of March of a leap year: the hour before is on the 29th of February
    leap = dt.datetime(2024, 3, 1, 0, 59, 59, tzinfo=UTC)
    e0, e1 = _hour(root, leap), _hour(root, dt.datetime(2024, 2, 29, 23, 0, tzinfo=UTC))
    assert e1.endswith("2024/02/29/23")
    assert ls(root, leap, 2, 2) == [e0, e1]


def test_sharded_index_without_any_hour_raises_the_reference_message(pkg, tmp_path):
    """No device is needed to find nothing: reload lists first, loads second."""
    ff = pkg.faiss_files
    ix = ff.HourlyShardedIndex(pkg.dense_ann.DistanceMetric.L2, 32, str(tmp_path), 3, 24)
    with pytest.raises(RuntimeError, match="Failed to find any shards during startup"):
        ix.reload(dt.datetime(2023, 3, 14, 15, tzinfo=UTC))
    assert ix.loads == 0 and ix.directories == []
