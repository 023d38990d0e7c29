"""A numpy model of what a device batch holds and of its plumbing (tf_shard.hip: slice, concat), independent of the library.

  rows(batch)                        the batch as comparable rows: per column "ABSENT" or the cell's value (nil included), the row's kind,
                                     part id, OldKeys presence and OldKeys values.  What is NOT there reads as its default, so two batches
                                     that differ only in whether they carry an all-default array give the same rows.
  concat_batches(parts, row_base)    tfgpu_dbatch_concat's result as an abi.Batch
  slice_batch(b, row0, n)            tfgpu_dbatch_slice's result as an abi.Batch
  part(n, start, attrs)              n rows of the mixed schema below built from explicit abi.Columns (every column's repr comes from the
                                     schema: a zero-row or all-nil column has no value to take one from), carrying the optional arrays `attrs` names

src_row is not part of rows(): the tests compare it on its own (merged_src_row states concat's rule)."""
import copy

import numpy as np

from transferia_amd import abi

SCHEMA = abi.Schema.of([["id", "int64", True], ["text", "utf8"], ["ts", "timestamp"], ["opt", "int32"], ["flag", "boolean"], ["js", "any"]])
NAMES = [c.name for c in SCHEMA.cols]
# the optional arrays a part may or may not carry
ATTRS = ("validity.text", "validity.ts", "validity.opt", "validity.js", "nanos", "absent", "kind", "part_id", "src_row", "old_present", "old_validity")
TEXTS = [b"", b"a", b"seven77", b"eight888", b"nine99999", "наж".encode(), b'q"\\', b"x" * 37]
DOCS = [b'{"a":1}', b"[]", b"null", b'"s<>"', b"12.5", b'{"k":[1,{"z":null}]}']


def _var(cells):
    off = np.zeros(len(cells) + 1, np.uint32)
    if cells:
        off[1:] = np.cumsum([len(c) for c in cells])
    return off, np.frombuffer(b"".join(cells), np.uint8).copy()


def part(n, start=0, attrs=(), ns="db", table="t", old=True):
    """rows start .. start + n - 1 of one endless deterministic table; `attrs`: which of ATTRS this part carries.  Without "validity.X" column X
    holds no nil (and no validity array); without "absent" every row lists every column; and so on: the arrays' absence is part of the case."""
    attrs = set(attrs)
    assert attrs <= set(ATTRS), attrs - set(ATTRS)
    k = np.arange(start, start + n, dtype=np.int64)
    h = (k * 2654435761 + 12345) % 1000003      # a scramble of the row number: cells differ from row to row and from part to part

    def valid(name, mod, r):   # (by the row number: any `mod` consecutive rows hold a nil, so a part of five rows has one in every column)
        return (k % mod != r) if "validity." + name in attrs else None
    vt = valid("text", 3, 0)
    off, data = _var([TEXTS[int(x) % len(TEXTS)] + b"%d" % int(r) if vt is None or vt[i] else b"" for i, (x, r) in enumerate(zip(h, k))])
    text = abi.Column("text", "utf8", abi.R_STRING, offsets=off, data=data, validity=vt)
    ts = abi.Column("ts", "timestamp", abi.R_TIME, values=1_600_000_000 + h, validity=valid("ts", 4, 1),
                    nanos=((h * 997) % 10**9).astype(np.int32) if "nanos" in attrs else None)
    opt = abi.Column("opt", "int32", abi.R_INT32, values=(h % 100000 - 50000).astype(np.int32), validity=valid("opt", 5, 2))
    if "absent" in attrs:
        opt.absent = k % 5 == 3
    vd = valid("js", 3, 1)
    off, data = _var([DOCS[int(x) % len(DOCS)] if vd is None or vd[i] else b"" for i, x in enumerate(h)])
    doc = abi.Column("js", "any", abi.R_JSON, offsets=off, data=data, validity=vd)
    cols = [abi.Column("id", "int64", abi.R_INT64, values=k * 10 + 1), text, ts, opt, abi.Column("flag", "boolean", abi.R_BOOL, values=(h & 1).astype(np.uint8)), doc]
    b = abi.Batch(cols, n, ns, table)
    b.schema = SCHEMA
    if old:
        b.old_keys = [abi.Column("id", "int64", abi.R_INT64, values=k * 10 + 7, validity=(k % 3 != 2) if "old_validity" in attrs else None)]
        b.old_present = (k % 4 != 2) if "old_present" in attrs else None
    if "kind" in attrs:
        b.kind = (h % 3).astype(np.uint8)           # insert / update / delete
    if "part_id" in attrs:
        b.part_id = (h % 11).astype(np.uint32)
    if "src_row" in attrs:
        b.src_row = (3 * np.arange(n) + 2).astype(np.int32)   # as a filter in front would leave it: increasing, with gaps
    return b


def _absent(c, n):
    a = getattr(c, "absent", None)
    return np.zeros(n, bool) if a is None else np.asarray(a, bool)


def _cell(c, i):
    v = c.pyvalue(i)
    return tuple(v) if v[0] != "nil" else ("nil", None)


def rows(b):
    n = b.nrows
    old = getattr(b, "old_keys", None) or []
    pres = getattr(b, "old_present", None)
    ab = [_absent(c, n) for c in b.cols]
    out = []
    for i in range(n):
        has = bool(old) and (pres is None or bool(pres[i]))
        out.append({"cells": tuple("ABSENT" if ab[j][i] else _cell(c, i) for j, c in enumerate(b.cols)),
                    "kind": 0 if b.kind is None else int(b.kind[i]),
                    "part_id": 0 if b.part_id is None else int(b.part_id[i]),
                    "old_present": has,
                    "old": tuple(_cell(c, i) for c in old) if has else None})
    return out


def shape(b):
    """what must agree between a batch and its model besides the rows: the table, the columns' names, types and reprs"""
    return (b.table_ns, b.table_name, [(c.name, c.dtype, c.repr) for c in b.cols], [(c.name, c.dtype, c.repr) for c in (getattr(b, "old_keys", None) or [])])


def _cat(parts, pick, default, dtype):
    """the parts' arrays end to end; a part without one contributes `default(n)`; nobody has one: None"""
    got = [pick(p) for p in parts]
    if all(g is None for g in got):
        return None
    return np.concatenate([np.asarray(g, dtype) if g is not None else default(p.nrows).astype(dtype) for g, p in zip(got, parts)]) if parts else None


def _cat_column(cols, parts):
    c0 = cols[0]
    d = abi.Column(c0.name, c0.dtype, c0.repr)
    ns = [p.nrows for p in parts]
    if c0.repr in abi.VAR_REPRS:
        lens, data = [], []
        for c, n in zip(cols, ns):
            o = np.asarray(c.offsets[: n + 1], np.int64)
            lens.append(o[1:] - o[:-1])
            data.append(np.asarray(c.data, np.uint8)[int(o[0]): int(o[-1])])   # the part's text is what ITS offsets name
        d.offsets = np.zeros(sum(ns) + 1, np.uint32)
        d.offsets[1:] = np.cumsum(np.concatenate(lens)) if lens else 0
        d.data = np.concatenate(data) if data else np.zeros(0, np.uint8)
    else:
        d.values = np.concatenate([np.asarray(c.values[:n], abi.REPR_NP[c0.repr]) for c, n in zip(cols, ns)])
        have = [c.nanos is not None for c in cols]
        if any(have):
            d.nanos = np.concatenate([np.asarray(c.nanos[:n], np.int32) if c.nanos is not None else np.zeros(n, np.int32) for c, n in zip(cols, ns)])
    if any(c.validity is not None for c in cols):
        d.validity = np.concatenate([np.asarray(c.validity[:n], bool) if c.validity is not None else np.ones(n, bool) for c, n in zip(cols, ns)])
    if any(getattr(c, "absent", None) is not None for c in cols):
        d.absent = np.concatenate([_absent(c, n)[:n] for c, n in zip(cols, ns)])
        d.validity = (d.validity if d.validity is not None else np.ones(sum(ns), bool)) & ~d.absent   # an ABSENT cell reads nil
    return d


def merged_src_row(parts, row_base=None):
    """tf_shard.hip's rule: present if a part (with rows) has one or row_base is given; a part without one contributes arange(k); row_base[g] is
    added to part g's"""
    live = [(g, p) for g, p in enumerate(parts) if p.nrows]
    if row_base is None and all(p.src_row is None for _, p in live):
        return None
    out = [(np.asarray(p.src_row, np.int64) if p.src_row is not None else np.arange(p.nrows, dtype=np.int64)) + (int(row_base[g]) if row_base is not None else 0) for g, p in live]
    return (np.concatenate(out) if out else np.zeros(0, np.int64)).astype(np.int32)


def concat_batches(parts, row_base=None):
    p0 = parts[0]
    for p in parts:
        assert shape(p) == shape(p0), "the model merges parts of one shape only"
    n = sum(p.nrows for p in parts)
    out = abi.Batch([_cat_column([p.cols[i] for p in parts], parts) for i in range(len(p0.cols))], n, p0.table_ns, p0.table_name)
    out.schema = getattr(p0, "schema", None)
    old0 = getattr(p0, "old_keys", None) or []
    if old0:
        out.old_keys = [_cat_column([p.old_keys[i] for p in parts], parts) for i in range(len(old0))]
        out.old_present = _cat(parts, lambda p: getattr(p, "old_present", None), lambda k: np.ones(k, bool), bool)
    out.kind = _cat(parts, lambda p: p.kind, lambda k: np.zeros(k, np.uint8), np.uint8)
    out.part_id = _cat(parts, lambda p: p.part_id, lambda k: np.zeros(k, np.uint32), np.uint32)
    out.src_row = merged_src_row(parts, row_base)
    return out


def _slice_column(c, r0, n):
    d = abi.Column(c.name, c.dtype, c.repr)
    if c.repr in abi.VAR_REPRS:
        o = np.asarray(c.offsets[r0: r0 + n + 1], np.int64)
        d.offsets = (o - o[0]).astype(np.uint32)
        d.data = np.asarray(c.data, np.uint8)[int(o[0]): int(o[-1])].copy()
    else:
        d.values = c.values[r0: r0 + n].copy()
        d.nanos = None if c.nanos is None else c.nanos[r0: r0 + n].copy()
    d.validity = None if c.validity is None else np.asarray(c.validity, bool)[r0: r0 + n].copy()
    if getattr(c, "absent", None) is not None:
        d.absent = np.asarray(c.absent, bool)[r0: r0 + n].copy()
    return d


def slice_batch(b, row0, n):
    assert 0 <= row0 and 0 <= n and row0 + n <= b.nrows
    out = abi.Batch([_slice_column(c, row0, n) for c in b.cols], n, b.table_ns, b.table_name)
    out.schema = getattr(b, "schema", None)
    old = getattr(b, "old_keys", None) or []
    if old:
        out.old_keys = [_slice_column(c, row0, n) for c in old]
        pres = getattr(b, "old_present", None)
        out.old_present = None if pres is None else np.asarray(pres, bool)[row0: row0 + n].copy()
    for f in ("kind", "src_row", "part_id"):
        x = getattr(b, f)
        setattr(out, f, None if x is None else x[row0: row0 + n].copy())
    return out


def shift_text(b, prefix=5, fill=b"X"):
    """the same rows with every text column's offsets moved `prefix` bytes up over an unreferenced prefix: an Arrow-style slice of a larger buffer"""
    out = copy.copy(b)
    out.cols = list(b.cols)
    for i, c in enumerate(b.cols):
        if c.repr in abi.VAR_REPRS:
            d = copy.copy(c)
            d.offsets = (np.asarray(c.offsets, np.int64) + prefix).astype(np.uint32)
            d.data = np.concatenate([np.frombuffer(fill * prefix, np.uint8), np.asarray(c.data, np.uint8)[: int(c.offsets[-1])]])
            out.cols[i] = d
    return out
