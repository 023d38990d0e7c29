"""The edges of the newline count in front of the tile parser.  csv_count_newlines reads 28 KiB per tile: tiles wholly inside the
chunk take a path without the tail's byte masking, the last one keeps it, and the counts are kept per 1 KiB granule.  So the
chunk lengths sit 17, 16, 1, 0 bytes short of and 1, 15, 16, 17 bytes past a multiple of the tile and of the granule, each once
cut in the middle of a line and once ending in its '\\n'.  Every chunk is parsed twice on the same lane (the second time the lane
sizes the buffers ahead of the count) and both answers are compared with the oracle cell for cell; a child process repeats
everything with TFGPU_CSV_AHEAD=0."""
import os
import subprocess
import sys

import pytest

from transferia_amd import abi
from test_gpu_csv import compare

pytestmark = pytest.mark.gpu

NL_TILE = 28 * 1024
GRAN = 1024
DELTAS = [-17, -16, -1, 0, 1, 15, 16, 17]
LENGTHS = [NL_TILE * k + d for k in (1, 2, 3) for d in DELTAS] + [GRAN * k + d for k in (1, 2) for d in DELTAS]
S3 = abi.Schema.of([["a", "int32", False, "0"], ["b", "utf8", False, "1"], ["c", "int64", False, "2"]])
KW = dict(include_missing_columns=1)


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


def line(i):
    return b"%d,%s,%d\n" % (i, b"t" * (i % 23), i * 7)   # text cells of 0..22 bytes


def chunk(length, fit):
    """`length` bytes of three-column lines: cut where the length falls (an unfinished last line), or — fit — with a last line whose
    text cell is padded so that the chunk's last byte is its '\\n'"""
    out, n, i = [], 0, 0
    room = length - (64 if fit else 0)
    while n < room:
        ln = line(i)
        out.append(ln)
        n += len(ln)
        i += 1
    data = b"".join(out)
    if not fit:
        return data[:length]
    while len(data) > length - 5:  # make room for the shortest closing line: 1,,2\n
        data = data[: data.rstrip(b"\n").rfind(b"\n") + 1]
    return data + b"1," + b"p" * (length - len(data) - 5) + b",2\n"


def twice(tf, oracle, data, ctx, kw=KW):
    """the same chunk twice on the same lane: what a parse leaves behind (a control word not zeroed, the lane's size hint) must
    not change the next one"""
    a, ea = compare(tf, oracle, kw, S3, data, ctx + " (first)")
    b, eb = compare(tf, oracle, kw, S3, data, ctx + " (second)")
    assert a.nrows == b.nrows and sorted((e[0], e[1]) for e in ea) == sorted((e[0], e[1]) for e in eb), ctx
    return a


@pytest.mark.parametrize("fit", [False, True], ids=["cut", "fit"])
def test_lengths_around_tiles_and_granules(tf, oracle, fit):
    for length in LENGTHS:
        data = chunk(length, fit)
        assert len(data) == length and (data.endswith(b"\n") or not fit)
        twice(tf, oracle, data, "%d bytes %s" % (length, "fit" if fit else "cut"))


def test_shapes(tf, oracle):
    twice(tf, oracle, b"1," + b"x" * (2 * NL_TILE - 5) + b",2\n", "the only newline is the last byte")
    twice(tf, oracle, b"1,ab,2\n3,c", "fewer than 16 bytes")
    twice(tf, oracle, b"7\n", "two bytes")
    body = b"".join(line(i) for i in range(2000))
    twice(tf, oracle, body + b"5,\"" + b"y" * (NL_TILE + 3000) + b"\",6\n" + body, "a line longer than a tile (general path)")


def test_what_a_chunk_leaves_behind(tf, oracle):
    """a failing row, a doubled quote in a text cell and more lines than the lane expected (parsed again, the count read back first),
    each followed by a clean chunk on the same lane"""
    clean = chunk(2 * NL_TILE + 1, True)
    twice(tf, oracle, clean, "clean")
    bad = chunk(NL_TILE + 17, True).replace(b"\n40,", b"\nforty,", 1)
    _out, errs = compare(tf, oracle, KW, S3, bad, "a failing row")
    assert errs
    twice(tf, oracle, clean, "clean after a failing row")
    quoted = chunk(NL_TILE + 16, True).replace(line(41), b'41,"say ""hi""",287\n', 1)
    assert b'""hi""' in quoted
    twice(tf, oracle, quoted, "a doubled quote")
    twice(tf, oracle, clean, "clean after a doubled quote")
    dense = b"".join(b"%d,,%d\n" % (i % 10, i % 7) for i in range(3 * NL_TILE // 5))   # five-byte lines: several times the lines the hint allows
    twice(tf, oracle, dense, "more lines than the buffers were sized for")
    twice(tf, oracle, clean, "clean after the retry")


def test_again_without_sizing_ahead():
    if os.environ.get("TFGPU_CSV_AHEAD") == "0":
        return  # (this is the child)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TFGPU_CSV_AHEAD="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "lengths_around or shapes or leaves_behind"], capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "4 passed" in r.stdout, r.stdout[-500:]
