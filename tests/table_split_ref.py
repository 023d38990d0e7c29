"""table_splitter_transformer restated in plain Python (pkg/transformer/registry/table_splitter/table_splitter.go:37-59, 80-94): GenerateTableName of
every row, then the rows grouped by name in order of first appearance — what a sink's SplitByTableID makes of the transformer's output.

A component string is SerializeToString(item.AsMap()[col], schemaColumn.DataType); those come from the oracle's convert_to_string, which is pinned to
tests/golden/to_string.json.  A value the row does not have — a schema column the batch lacks, an ABSENT cell — is handed to it as the nil AsMap reads."""
import numpy as np

from transferia_amd import abi


def resolved_columns(config, batch):
    """[(name, DataType, batch column or None)] for every configured name the TableSchema has (the batch's columns when it carries none), in config order:
    a name outside the schema contributes nothing, a repeated name repeats; values by name, the last duplicate wins (AsMap)."""
    schema = getattr(batch, "schema", None)
    out = []
    for name in config.get("columns") or []:
        found = None
        for c in batch.cols:
            if c.name == name:
                found = c
        if schema is not None:
            dtype = next((c.dtype for c in schema.cols if c.name == name), None)
        else:
            dtype = found.dtype if found is not None else None
        if dtype is not None:
            out.append((name, dtype, found))
    return out


def component_strings(oracle, dtype, col, n):
    """SerializeToString of column `col` (None: nil in every row) under DataType `dtype`, one bytes object per row."""
    if n == 0:
        return []
    if col is None:
        c = abi.Column("c", dtype, abi.R_STRING, offsets=np.zeros(n + 1, np.uint32), data=np.zeros(0, np.uint8), validity=np.zeros(n, bool))
    else:
        valid = np.ones(n, bool) if col.validity is None else np.asarray(col.validity, bool).copy()
        if col.absent is not None:
            valid &= ~np.asarray(col.absent, bool)
        c = abi.Column("c", dtype, col.repr, values=col.values, offsets=col.offsets, data=col.data, nanos=col.nanos, validity=None if valid.all() else valid)
    out = oracle.apply_chain([oracle.Transformer("convert_to_string", {})], abi.Batch([c], n, "db", "t"), abi.Schema.of([["c", dtype, False]])).batch
    assert out.cols[0].validity is None or out.cols[0].validity.all()
    return [out.cols[0].get_bytes(i) for i in range(n)]


def table_names(oracle, config, batch):
    """GenerateTableName(item.Table, columns, splitter, &item) of every row, as bytes"""
    n = batch.nrows
    splitter = (config.get("splitter") or "/").encode("utf-8")
    parts = [[batch.table_name.encode("utf-8")] if batch.table_name else [] for _ in range(n)]
    for _name, dtype, col in resolved_columns(config, batch):
        for i, s in enumerate(component_strings(oracle, dtype, col, n)):
            parts[i].append(s)
    return [splitter.join(p) for p in parts]


def split(oracle, config, batch):
    """-> (names in order of first appearance, table of every row, rows of every table in input order)"""
    names, ids, index = [], np.zeros(batch.nrows, np.int32), {}
    for i, nm in enumerate(table_names(oracle, config, batch)):
        if nm not in index:
            index[nm] = len(names)
            names.append(nm)
        ids[i] = index[nm]
    return names, ids, [np.flatnonzero(ids == t).astype(np.int32) for t in range(len(names))]


def take_rows(batch, rows):
    """rows `rows` of a host batch, cell for cell: columns, OldKeys with presence, kinds, part_id, ABSENT bits; src_row composed with the batch's own"""
    rows = np.asarray(rows, np.int64)

    def col(c):
        o = abi.Column(c.name, c.dtype, c.repr)
        if c.repr in abi.VAR_REPRS:
            cells = [c.get_bytes(int(r)) for r in rows]
            o.offsets = np.zeros(len(rows) + 1, np.uint32)
            if len(rows):
                o.offsets[1:] = np.cumsum([len(x) for x in cells])
            o.data = np.frombuffer(b"".join(cells), np.uint8).copy()
        else:
            o.values = c.values[rows]
            o.nanos = c.nanos[rows] if c.nanos is not None else None
        o.validity = np.asarray(c.validity, bool)[rows] if c.validity is not None else None
        o.absent = np.asarray(c.absent, bool)[rows] if c.absent is not None else None
        return o

    out = abi.Batch([col(c) for c in batch.cols], len(rows), batch.table_ns, batch.table_name)
    if getattr(batch, "old_keys", None):
        out.old_keys = [col(c) for c in batch.old_keys]
        pres = getattr(batch, "old_present", None)
        out.old_present = np.asarray(pres, bool)[rows] if pres is not None else np.ones(len(rows), bool)
    out.kind = batch.kind[rows] if batch.kind is not None else None
    out.part_id = batch.part_id[rows] if batch.part_id is not None else None
    out.src_row = (batch.src_row[rows] if batch.src_row is not None else rows).astype(np.int32)
    return out
