"""filter_rows on the device (match_value and filter_eval_kernel, tf_transform.hip) against the plain-Python restatement of the Go (tests/filter_ref.py),
row for row: which source rows stay, which rows fail with which error class at which term.  The batches and filters are tests/filter_cases.py's — one
family of columns per test, 257 rows, edge values at rows 0, 255 and 256, nil cells, and a variant whose rows list their own columns.

HOST_FALLBACK: a row the device hands back is taken out of both sides only where the model marked that cell and term MAY_FALL_BACK (or has no answer
of its own); a row the model marks IMPL_DEFINED (Go's int64(float) outside the int64 range) must come back as HOST_FALLBACK; and in every family not
built for a fallback class no row at all may — tests/test_filter_ref.py asserts that the model marks none there.  Where the model has no answer (a text
under a time constant that is none of the fixed shapes) and the device answers, the answer must be the oracle's."""
import numpy as np
import pytest

import byids_ref
import filter_cases as cases
import filter_ref as ref
from transferia_amd import abi

pytestmark = pytest.mark.gpu
CASES = cases.all_cases()


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


def oracle_rows(oracle, fam, cfg):
    res = oracle.Transformer("filter_rows", cfg).apply(fam.batch, fam.schema())
    src = res.batch.src_row if res.batch.src_row is not None else np.arange(res.batch.nrows)
    out = {int(r): "keep" for r in src[: res.batch.nrows]}
    out.update({int(row): abi.ROWERR[code] for row, code, _msg in res.errors})
    return out


def assert_carries_the_rows(got, batch, idx, ctx):
    """the downloaded batch's columns are the input's at the kept rows"""
    want = byids_ref.take_rows(batch, idx)
    assert got.nrows == want.nrows and [c.name for c in got.cols] == [c.name for c in want.cols], ctx
    for a, b in zip(got.cols, want.cols):
        assert (a.dtype, a.repr) == (b.dtype, b.repr), (ctx, a.name)
        va = a.validity if a.validity is not None else np.ones(got.nrows, bool)
        vb = b.validity if b.validity is not None else np.ones(want.nrows, bool)
        ab = a.absent if a.absent is not None else np.zeros(got.nrows, bool)
        bb = b.absent if b.absent is not None else np.zeros(want.nrows, bool)
        assert np.array_equal(ab, bb) and np.array_equal(va & ~ab, vb & ~bb), (ctx, a.name, "nil / ABSENT")
        ok = va & ~ab
        if a.repr in abi.VAR_REPRS:
            assert [a.get_bytes(i) for i in np.flatnonzero(ok)] == [b.get_bytes(i) for i in np.flatnonzero(ok)], (ctx, a.name)
        else:
            assert np.array_equal(a.values[ok].view(np.uint8), b.values[ok].view(np.uint8)), (ctx, a.name)
            if a.repr == abi.R_TIME:
                na = a.nanos if a.nanos is not None else np.zeros(got.nrows, np.int32)
                nb = b.nanos if b.nanos is not None else np.zeros(want.nrows, np.int32)
                assert np.array_equal(na[ok], nb[ok]), (ctx, a.name, "nanos")
    wk = want.kind if want.kind is not None else np.zeros(want.nrows, np.uint8)
    gk = got.kind if got.kind is not None else np.zeros(got.nrows, np.uint8)
    assert np.array_equal(gk, wk), (ctx, "kind")


@pytest.mark.parametrize("fam", CASES, ids=[f.name for f in CASES])
def test_device_against_the_model(tf, oracle, fam):
    db = tf.DeviceBatch.upload(fam.batch)
    handed_back = carried = 0
    for cfg in fam.filters:
        rows = ref.apply(fam.batch, cfg)
        res = tf.Transformer("filter_rows", cfg).apply(db)
        out = res.transformed.download()
        kept = (out.src_row if out.src_row is not None else np.arange(out.nrows)).tolist()
        back = {row: term for row, code, _step, term in res.errors if code == "HOST_FALLBACK"}
        errs = sorted((row, code, term) for row, code, _step, term in res.errors if code != "HOST_FALLBACK")
        ctx = (fam.name, cfg)
        if not fam.fallback:
            assert not back, (ctx, "rows handed back to the host path", sorted(back.items())[:5])
        for row, term in back.items():
            r = rows[row]
            assert term in r.fall_back or (r.outcome in (ref.IMPL_DEFINED, ref.UNDECIDED) and r.term == term), (ctx, row, term, r, "handed back where the reference decides")
        handed_back += len(back)
        undecided = [i for i, r in enumerate(rows) if r.outcome == ref.UNDECIDED and i not in back]
        theirs = oracle_rows(oracle, fam, cfg) if undecided else {}
        want_kept, want_errs = [], []
        for i, r in enumerate(rows):
            if i in back:
                continue
            assert r.outcome != ref.IMPL_DEFINED, (ctx, i, [c.pyvalue(i) for c in fam.batch.cols], "int64(float) outside the int64 range: answered, not handed back")
            outcome = theirs.get(i, "drop") if r.outcome == ref.UNDECIDED else r.outcome
            if outcome == "keep":
                want_kept.append(i)
            elif outcome != "drop":
                want_errs.append((i, outcome, r.term))
        assert kept == want_kept, (ctx, "kept rows", [(i, [c.pyvalue(i) for c in fam.batch.cols], rows[i]) for i in sorted(set(kept) ^ set(want_kept))[:6]])
        assert errs == want_errs, (ctx, "row errors", sorted(set(errs) ^ set(want_errs))[:6])
        if not carried and 0 < len(kept) < fam.batch.nrows:
            assert_carries_the_rows(out, fam.batch, kept, ctx)
            carried = 1
    assert carried or fam.name.startswith(("interval", "json.Number", "any/containers", "system", "kinds/system")), fam.name
    if fam.fallback:
        assert handed_back > 0, fam.name      # the family reaches its fallback class on the device
