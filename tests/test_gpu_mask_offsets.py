"""mask_field's digests are 64 hex bytes each, and the kernel that computes them writes the column's Arrow offsets itself — 64·r for
every row and offsets[n] by the last row's thread.  Row counts around one 256-thread workgroup, on a dense batch and on one whose
rows are still a filter_rows selection; offsets against 64·r, digests against the oracle's."""
import numpy as np
import pytest

from transferia_amd import abi
from test_gpu_transformers import assert_batches_equal

pytestmark = pytest.mark.gpu

ROWS = [1, 255, 256, 257]
SKIPPED = 100   # rows the filter drops in front of the kept ones
S = abi.Schema.of([["id", "int32", False, "0"], ["ip", "int64", False, "1"], ["name", "utf8", False, "2"]])
MASK = ("mask_field", {"maskFunctionHash": {"userDefinedSalt": "offsets-salt"}, "columns": ["ip"]})
FILTER = ("filter_rows", {"filter": "id >= %d" % SKIPPED})


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


def run(tf, oracle, chain, n):
    data = b"".join(b"%d,%d,n%d\n" % (r, r * 2654435761 % (1 << 40) - 77, r) for r in range(n))
    opts = abi.csv_options()
    db, consumed, errs = tf.csv_parse(opts, S, data)
    assert consumed == len(data) and not errs and db.nrows == n
    out = tf.apply_chain([tf.Transformer(t, c) for t, c in chain], db).transformed.download()
    ref = oracle.csv_parse(opts, S, data, "", "")
    want = oracle.apply_chain([oracle.Transformer(t, c) for t, c in chain], ref.batch, ref.schema).batch
    return out, want


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("behind_filter", [False, True], ids=["dense", "selection"])
def test_digest_offsets(tf, oracle, n, behind_filter):
    chain = [FILTER, MASK] if behind_filter else [MASK]
    out, want = run(tf, oracle, chain, n + SKIPPED if behind_filter else n)
    assert out.nrows == n
    col = out.col("ip")
    assert np.array_equal(np.asarray(col.offsets, dtype=np.int64), 64 * np.arange(n + 1, dtype=np.int64))
    assert_batches_equal(out, want, "mask %d rows%s" % (n, " behind a filter" if behind_filter else ""))
    if behind_filter:
        src = out.src_row if out.src_row is not None else np.arange(out.nrows)
        assert np.array_equal(src, want.src_row)
