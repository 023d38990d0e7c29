"""Pins the plain-Python restatement of the native parser (tests/nativeparse_ref.py) to the reference's own vectors — the assertions of TestRestore,
TestRestoreFloatInt64 and TestRestoreJSONB (pkg/abstract/restore_test.go, values in tests/golden/native_parser.json) and the ChangeItem fixtures under
tests/golden/debezium_emitter/ — and the host-side behaviour of the entry that needs no device: the size refusals and the guard on a NULL or
inconsistent batch.  No GPU."""
import glob
import json
import os

import numpy as np
import pytest

import nativeparse_ref as R
from oracle import dbz_emitter as E
from rawtable_ref import go_string_html
from transferia_amd import abi, lib
from util import golden

G = golden("native_parser.json")
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "debezium_emitter")


# ---- Restore's own test values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G["restore"], ids=lambda c: "line%d" % c["line"])
def test_restore_vectors(case):
    col = R.Column("test_col", {"name": "test_col", "type": case["type"], "original_type": case["original_type"]})
    try:
        got = R.restore_cell(col, case["value"].encode("utf-8"))
    except R.Fallback as f:
        assert case["device"] == f.reason   # the stock parser computes case["restore"]
        return
    assert case["device"] == "parsed"
    g, v = got
    wg, wv = case["restore"]
    assert (g, v.decode("utf-8") if isinstance(v, bytes) else v) == (wg, wv)


def test_restore_vectors_cover_both_sides():
    kinds = {c["device"] for c in G["restore"]}
    assert "parsed" in kinds and {"NUM_STRING", "INT_FORM", "ANY_STRING", "SCHEMA_COLUMN"} <= kinds


# ---- the ChangeItem fixtures --------------------------------------------------------------------------------------------------------------------------------
def fixtures():
    out = []
    for f in sorted(glob.glob(os.path.join(FIX, "*.txt"))):
        raw = open(f, "rb").read().strip()
        try:
            d = json.loads(raw)
        except ValueError:
            continue
        if isinstance(d, dict) and "columnnames" in d:
            out.append((os.path.basename(f), raw))
    return out


def as_cell(v):
    g, x = v
    return (g, tuple(x[:2]) if g == "time" else x)


def comparable(theirs, mine, dtype):
    """oracle/dbz_emitter.restore keeps an `any` value as the Go value (a string, a json.Number, a bool, json text without HTML escaping); the ABI carries
    its json.Marshal text"""
    g, x = theirs
    if dtype != "any" or g == "nil":
        return as_cell(theirs) == mine
    text = {"string": lambda: go_string_html(x.decode("utf-8")), "jsonnum": lambda: x, "bool": lambda: b"true" if x else b"false",
            "json": lambda: x.replace(b"<", b"\\u003c").replace(b">", b"\\u003e").replace(b"&", b"\\u0026")}[g]()
    return mine == ("json", text)


@pytest.mark.parametrize("name,raw", fixtures(), ids=lambda x: x if isinstance(x, str) else "")
def test_fixture(name, raw):
    res = R.parse([b"[" + raw + b"]"])
    want = G["fixtures"][name]
    if want != "parsed":
        assert res.fallback == [(0, want["reason"], want["item"], want["column"])] and not res.groups and res.items == [(0, -1, -1)]
        d = json.loads(raw)
        assert (d["columnnames"] + d.get("oldkeys", {}).get("keynames", []))[want["column"]] == want["column_name"]
        return
    assert not res.fallback and len(res.groups) == 1 and res.items == [(0, 0, 0)]
    item = E.unmarshal_change_item(raw)   # abstract.UnmarshalChangeItem as the emitter's oracle restates it
    grp = res.groups[0]
    kind, values, old, meta = grp.rows[0]
    assert (kind, grp.ns, grp.table, grp.names, grp.key_names) == (item.kind, item.schema, item.table, item.names, item.old_names)
    dts = {c.name: c.dtype for c in item.cols}
    exact = name.startswith("emitter_replica_identity")
    for n, theirs, mine in zip(item.names, item.values, values):
        assert (as_cell(theirs) == mine) if exact else comparable(theirs, mine, dts[n]), (name, n, theirs, mine)
    if item.kind != "insert" and item.old_values:
        for n, theirs, mine in zip(item.old_names, item.old_values, old):
            assert (as_cell(theirs) == mine) if exact else comparable(theirs, mine, dts[n]), (name, n, theirs, mine)
    assert (meta["id"], meta["lsn"], meta["commit_time"]) == (item.id, item.lsn, item.commit_time)
    b, schema, m = R.group_batch(grp)   # and the group as an abi.Batch
    assert b.nrows == 1 and [c.name for c in b.cols] == grp.names and [c.name for c in schema.cols] == [c.name for c in item.cols]


def test_fixture_expectations():
    names = [n for n, _ in fixtures()]
    assert sorted(names) == sorted(G["fixtures"])
    for n in ("emitter_replica_identity__canon_change_item_update.txt", "emitter_replica_identity__canon_change_item_delete.txt"):
        assert G["fixtures"][n] == "parsed"
    pg = [n for n in names if n.startswith("emitter_crud_test")]
    assert pg and all(G["fixtures"][n]["reason"] == "TIME_ZONE" for n in pg)   # the +04:00 timestamps


# ---- the restatement's own corners -------------------------------------------------------------------------------------------------------------------------------
def test_cut_and_all_or_nothing():
    a = b'{"kind":"insert","columnnames":null,"table":"t"}'
    assert R.cut(b" [ " + a + b" , " + a + b" ] ") == [(3, 3 + len(a)), (6 + len(a), 6 + 2 * len(a))]
    for bad in (b"", b"[", b"[1]", b"[{}{}]", b"[{},]", b"[{}]x", b'[{"a":"]}', b"{}"):
        assert R.cut(bad) is None, bad
    res = R.parse([b"[" + a + b"," + a.replace(b"insert", b"truncate") + b"]", None, b"[" + a + b"]"])
    assert res.fallback == [(0, "KIND", 1, -1)] and res.items == [(0, -1, -1), (0, -1, -1), (2, 0, 0)] and len(res.groups) == 1
    assert res.groups[0].names_form == 1 and res.groups[0].rows[0][0] == "insert"


# ---- the entry's host side ---------------------------------------------------------------------------------------------------------------------------------------------
def test_size_refusals_and_guard():
    with pytest.raises(lib.TfgpuError) as ex:
        lib.native_check_sizes(None)
    assert ex.value.code == lib.ERR_INVALID and "null batch" in str(ex.value)
    ok = abi.message_batch("t", 0, [(0, 0, None, b"[]", None)])
    lib.native_check_sizes(ok)
    for field, value, code, text in (("nmsg", -1, lib.ERR_INVALID, "negative message count"), ("mem", 7, lib.ERR_INVALID, "bad mem"),
                                     ("value_start", None, lib.ERR_INVALID, "value_start is null"), ("values", None, lib.ERR_INVALID, "values buffer is null"),
                                     ("values_len", 0xFFFFFFF0, lib.ERR_UNSUPPORTED, "the values reach 4 GiB"), ("nmsg", 1 << 31, lib.ERR_UNSUPPORTED, "2^31-1 messages")):
        b = abi.message_batch("t", 0, [(0, 0, None, b"[]", None)])
        setattr(b, field, value)
        with pytest.raises(lib.TfgpuError) as ex:
            lib.native_check_sizes(b)
        assert ex.value.code == code and text in str(ex.value), field
    # starts that claim more than the buffer holds, or 4 GiB
    b = abi.message_batch("t", 0, [(0, 0, None, b"[]", None)])
    starts = np.array([0, 3], np.uint64)
    b.value_start = starts.ctypes.data
    with pytest.raises(lib.TfgpuError) as ex:
        lib.native_check_sizes(b)
    assert ex.value.code == lib.ERR_INVALID and "inside the buffer" in str(ex.value)
    starts[1] = 0xFFFFFFF0
    with pytest.raises(lib.TfgpuError) as ex:
        lib.native_check_sizes(b)
    assert ex.value.code == lib.ERR_UNSUPPORTED
    # the parse entry runs the same checks before it asks for a device
    out = __import__("ctypes").c_void_p()
    assert lib.load().tfgpu_native_parse(None, __import__("ctypes").byref(out)) == lib.ERR_INVALID
    assert lib.load().tfgpu_native_parse(__import__("ctypes").byref(ok), None) == lib.ERR_INVALID
