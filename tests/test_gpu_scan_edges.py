"""The edges of the segmented offset scan (tf_scan.hip) as the CSV ingest uses it: every text column's cell lengths become its
Arrow offsets in one two-launch scan, a segment per column.  A workgroup covers W = 4096 elements, 16 consecutive ones a thread: the
second kernel loads them, adds up the totals of the workgroups in front of it, and writes the offsets; a column's last offset (the
total) is written by whichever thread holds the last row.  Row counts sit around one workgroup, around two, and around and past
16384 (a width that was measured and not kept); the limit up to which the workgroups add up the raw block totals themselves is
unchanged (4 Mi elements a segment), so no larger case is needed for it.  Cell lengths include 0; offsets are checked against
numpy.cumsum."""
import numpy as np
import pytest

from transferia_amd import abi

pytestmark = pytest.mark.gpu

W = 4096
ROWS = [1, W - 1, W, W + 1, 2 * W + 1, 4 * W - 1, 4 * W, 4 * W + 1, 8 * W + 1]


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


def cell_len(r, c):
    return (r * 7 + c * 3 + (r >> 9)) % 9   # 0..8 bytes, another pattern in every column


@pytest.fixture(scope="module")
def cases():
    """(text columns, rows) → (schema, csv bytes, expected lengths [column][row]), built once"""
    out = {}
    for ntext in (2, 5):
        schema = abi.Schema.of([["id", "int32", False, "0"]] + [["t%d" % c, "utf8", False, str(c + 1)] for c in range(ntext)])
        n = max(ROWS)
        lens = np.array([[cell_len(r, c) for r in range(n)] for c in range(ntext)], dtype=np.int64)
        lines = [b"%d,%s\n" % (r, b",".join(bytes([97 + c]) * int(lens[c, r]) for c in range(ntext))) for r in range(n)]
        out[ntext] = (schema, lines, lens)
    return out


@pytest.mark.parametrize("ntext", [2, 5])
@pytest.mark.parametrize("nrows", ROWS)
def test_text_offsets(tf, cases, ntext, nrows):
    schema, lines, lens = cases[ntext]
    data = b"".join(lines[:nrows])
    db, consumed, errs = tf.csv_parse(abi.csv_options(), schema, data)
    assert consumed == len(data) and not errs and db.nrows == nrows
    out = db.download()
    for c in range(ntext):
        col = out.col("t%d" % c)
        want = np.concatenate([[0], np.cumsum(lens[c, :nrows])])
        got = np.asarray(col.offsets, dtype=np.int64)
        assert got.shape == want.shape and np.array_equal(got, want), (ntext, nrows, c, np.flatnonzero(got != want)[:4])
        assert bytes(col.data[: int(want[-1])]) == bytes([97 + c]) * int(want[-1])
