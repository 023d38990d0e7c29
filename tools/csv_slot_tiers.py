#!/usr/bin/env python3
"""Replays, on the CPU, how csv_parse_regular deals the cells of the bench's hits CSV into slots of 64, and which tier of the
cell code each slot takes — for text under the tier rule the kernel had before the straight tier was widened ("before") and
under the present one ("now").

    python tools/csv_slot_tiers.py [ROWS]        (default 16384; no GPU, no oracle: transferia_amd.workload alone)

The input is cut into CT_T-byte tiles (a tile owns the lines whose '\\n' falls into it), the columns are grouped into runs as
tfgpu_csv_parse sorts them (kind, width, field), and a run's items (column, line) are numbered with lines fastest: 64 items are
one slot, and a slot takes a straight-line tier only if EVERY active lane qualifies (for_slots / reg_*_body in tf_csv.hip).
Printed per run: slots a tile, the share of slots on each tier, and for text slots off the straight tier the columns and
causes."""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from transferia_amd import workload  # noqa: E402

CT_T = 28672   # tf_csv.hip: NL_TILE, the bytes whose '\n' one workgroup owns
QUOTE = 0x22
WIDTH = {"int8": 1, "uint8": 1, "int16": 2, "uint16": 2, "int32": 4, "uint32": 4, "int64": 8, "uint64": 8}
TEXT = {"utf8", "string", "any"}


def split_fields(line: bytes):
    """fields of one line (without its '\\n'): a delimiter counts where the quote parity in front of it is even"""
    out, cur, odd = [], None, False
    for piece in line.split(b","):
        cur = piece if cur is None else cur + b"," + piece
        odd ^= piece.count(b'"') & 1 == 1
        if not odd:
            out.append(cur)
            cur = None
    if cur is not None:
        out.append(cur)
    return out


def run_of(typ):
    if typ in WIDTH:
        return "int%d" % (8 * WIDTH[typ])
    if typ in TEXT:
        return "text"
    return typ  # date, timestamp, …


# --- tier of one lane's cell; a slot's tier is the worst of its lanes -------------------------------------------------------
def int_tier(cell: bytes, width: int):
    n = len(cell)
    if 1 <= n <= 4:
        return 0
    fastd = 5 if width < 4 else 8
    if n and (cell[0] >= 0x31 or n == 1) and n <= fastd:
        return 1
    return 2


INT_TIERS = ("A (1-4 digits)", "first (5 / 8 digits)", "19-digit / rare shapes")


def ascii_ok(c):
    return 0x21 <= c <= 0x7E


def text_before(cell: bytes, prev2: bytes):
    n, qn = len(cell), cell.count(b'"')
    if n == 0 or (qn == 0 and ascii_ok(cell[0]) and ascii_ok(cell[-1])) or (qn == 2 and cell[0] == QUOTE and cell[-1] == QUOTE):
        return 0, None
    return 2, cause(cell)


def text_now(cell: bytes, prev2: bytes):
    """prev2: the two bytes in front of the cell (the kernel looks two bytes back from the last byte wherever that lands)"""
    n, qn = len(cell), cell.count(b'"')
    if n == 0:
        return 0, None
    if n >= 2 and cell[0] == QUOTE and cell[-1] == QUOTE:
        return (1 if qn > 2 else 0), None
    first, last = cell[0], cell[-1]
    back = (prev2 + cell)[-3:]
    first_ok = ascii_ok(first) or (first >= 0x80 and first not in (0xC2, 0xE1, 0xE2, 0xE3))
    last_ok = ascii_ok(last) or last >= 0xC0 or (last >= 0x80 and back[-2] != 0xC2 and back[-3] not in (0xE1, 0xE2, 0xE3))
    if qn == 0 and first_ok and last_ok:
        return 0, None
    return 2, cause(cell)


def cause(cell: bytes):
    qn = cell.count(b'"')
    if cell[0] == QUOTE and cell[-1] == QUOTE and len(cell) >= 2:
        return "enclosed, quotes inside"
    if qn:
        return "quote not enclosing"
    if cell[0] <= 0x20 or cell[-1] <= 0x20 or cell[-1] == 0x7F or cell[0] == 0x7F:
        return "ASCII space / control at an end"
    if cell[-1] >= 0x80 and cell[0] < 0x80:
        return "non-ASCII last byte"
    if cell[0] >= 0x80 and cell[-1] < 0x80:
        return "non-ASCII first byte"
    return "non-ASCII at both ends"


TEXT_TIERS = ("straight", "straight + pair count", "general code")


def time_shape(cell: bytes):
    """date and timestamp cells have no tier of their own (one was measured and dropped, profiles/EXPERIMENTS.md §3.28): what is
    reported is whether a slot's cells share the one shape such a tier would take"""
    return 0 if len(cell) in (10, 19) and cell[4:5] == b"-" else 1


TIME_TIERS = ("per-lane code, every cell 2006-01-02[ 15:04:05]", "per-lane code, other shapes among them")


def main():
    nrows = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    cols = workload.hits_columns()
    data = workload.hits_csv(nrows)
    # runs: columns of one kind and width, by field
    runs = collections.OrderedDict()
    for f, (name, typ, _k) in sorted(enumerate(cols), key=lambda x: (run_of(x[1][1]), x[0])):
        runs.setdefault(run_of(typ), []).append((f, name, WIDTH.get(typ, 0)))
    # tiles: lists of (line number, fields, line bytes)
    tiles, pos, lineno = collections.defaultdict(list), 0, 0
    while pos < len(data):
        e = data.find(b"\n", pos)
        if e < 0:
            break
        tiles[e // CT_T].append((lineno, split_fields(data[pos:e]), data[pos:e]))
        pos, lineno = e + 1, lineno + 1
    ntiles = len(tiles)
    lines_per_tile = [len(v) for v in tiles.values()]
    print("%d rows, %d bytes, %d tiles of %d bytes, %d-%d lines a tile" % (nrows, len(data), ntiles, CT_T, min(lines_per_tile), max(lines_per_tile)))

    for rname, rcols in runs.items():
        if rname.startswith("int"):
            names, rules = INT_TIERS, {"before": None, "now": None}
        elif rname == "text":
            names, rules = TEXT_TIERS, {"before": text_before, "now": text_now}
        elif rname in ("date", "timestamp"):
            names, rules = TIME_TIERS, {"now": time_shape}
        else:
            print("\n%s: %d columns — cells of this kind take the per-row path" % (rname, len(rcols)))
            continue
        share = {k: collections.Counter() for k in rules}
        causes = {k: collections.Counter() for k in rules}
        culprit_cols = {k: collections.Counter() for k in rules}
        nslots = 0
        for lines in tiles.values():
            nr = len(lines)
            items = len(rcols) * nr
            for s0 in range(0, items, 64):
                nslots += 1
                worst = {k: 0 for k in rules}
                why = {k: set() for k in rules}
                for it in range(s0, min(s0 + 64, items)):
                    ci, jj = divmod(it, nr)
                    ln, fields, _raw = lines[jj]
                    if ln == 0:   # the header line: an idle lane
                        continue
                    f, cname, width = rcols[ci]
                    cell = fields[f]
                    for k, rule in rules.items():
                        if rname.startswith("int"):
                            tier, c = int_tier(cell, width), None
                        elif rname == "text":
                            prev2 = (b",".join(fields[:f]) + b",")[-2:] if f else b"\n\n"
                            tier, c = rule(cell, prev2)
                        else:
                            tier, c = rule(cell), None
                        if tier > worst[k]:
                            worst[k] = tier
                        if c:
                            why[k].add((cname, c))
                for k in rules:
                    share[k][worst[k]] += 1
                    if rname == "text" and worst[k] == 2:
                        for c in {c for _n, c in why[k]}:
                            causes[k][c] += 1
                        for cname in {n for n, _c in why[k]}:
                            culprit_cols[k][cname] += 1
        print("\n%s: %d columns, %.1f slots a tile" % (rname, len(rcols), nslots / ntiles))
        for k in rules:
            if rname.startswith("int") and k == "before":
                continue  # the integer tiers did not change
            print("  %-6s %s" % (k if rname == "text" else "", "   ".join("%s %.1f %%" % (names[t], 100.0 * share[k][t] / nslots) for t in range(len(names)))))
            if causes[k]:
                off = share[k][2]
                print("         slots off the straight tier that hold a cell of each cause: " + ", ".join("%s %.1f %%" % (c, 100.0 * n / off) for c, n in causes[k].most_common()))
                print("         … and a cell of each column: " + ", ".join("%s %.1f %%" % (c, 100.0 * n / off) for c, n in culprit_cols[k].most_common(8)))


if __name__ == "__main__":
    main()
