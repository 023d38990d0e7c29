"""tests/parquet_hand.py pinned to pyarrow, on the CPU: the hand-written objects read back as intended (every page kind the device
tests use), and each plain reference decoder equals pyarrow's codec / reader on every stream tests/test_gpu_parquet_pages.py
generates — the same generators, the same seeds — so those tests cannot be wrong on both sides."""
import io

import numpy as np
import pytest

import parquet_hand as ph

pa = pytest.importorskip("pyarrow")
pq = pytest.importorskip("pyarrow.parquet")

CODECS = {ph.C_SNAPPY: "snappy", ph.C_LZ4_RAW: "lz4_raw"}


def read(obj):
    return pq.read_table(io.BytesIO(obj)).column("c").to_pylist()


def compress(codec, raw):
    return raw if codec == ph.C_NONE else pa.Codec(CODECS[codec]).compress(raw).to_pybytes()


def decode(codec, s):
    return ph.snappy_decode(s) if codec == ph.C_SNAPPY else ph.lz4_decode(s)


@pytest.mark.parametrize("long", [False, True])
@pytest.mark.parametrize("codec", [ph.C_NONE, ph.C_SNAPPY, ph.C_LZ4_RAW])
def test_pyarrow_reads_every_page_kind(codec, long):
    """v1 and v2, required and optional, INT64 and BYTE_ARRAY, a dictionary page with RLE_DICTIONARY indices, DELTA_BINARY_PACKED, pad 0..3,
    field headers in delta and in long form"""
    rng = np.random.default_rng(3)
    n = 300
    ints = ph.repetitive_int64(n, rng)
    valid = ph.valid_mask("random", n, rng)
    texts = [b"text-%d" % (i % 17) * (i % 5) for i in range(n)]
    want_i = [int(v) for v in ints]
    for pad in range(4):
        # required
        raw = ints.tobytes()
        assert read(ph.hand_object([ph.Page(ph.V1, n, ph.E_PLAIN, compress(codec, raw), len(raw))], ph.T_INT64, codec, False, pad, long)) == want_i
        assert read(ph.hand_object([ph.Page(ph.V2, n, ph.E_PLAIN, compress(codec, raw), len(raw))], ph.T_INT64, codec, False, pad, long)) == want_i
        assert read(ph.values_object(compress(codec, raw), len(raw), codec, ph.V2, pad, long)) == want_i
        raw = ph.plain_byte_arrays(texts)
        assert read(ph.hand_object([ph.Page(ph.V1, n, ph.E_PLAIN, compress(codec, raw), len(raw))], ph.T_BYTE_ARRAY, codec, False, pad, long)) == texts
        # optional: v1 keeps the levels inside the compressed body, v2 in front of it
        opt_i = [int(v) if ok else None for v, ok in zip(ints, valid)]
        present = ints[valid].tobytes()
        raw = ph.levels_v1(valid) + present
        assert read(ph.hand_object([ph.Page(ph.V1, n, ph.E_PLAIN, compress(codec, raw), len(raw))], ph.T_INT64, codec, True, pad, long)) == opt_i
        lead = ph.levels_v1(valid)[4:]
        nulls = int(n - valid.sum())
        assert read(ph.hand_object([ph.Page(ph.V2, n, ph.E_PLAIN, compress(codec, present), len(present), nulls, lead)], ph.T_INT64, codec, True, pad, long)) == opt_i
        raw = ph.plain_byte_arrays([t for t, ok in zip(texts, valid) if ok])
        assert read(ph.hand_object([ph.Page(ph.V2, n, ph.E_PLAIN, compress(codec, raw), len(raw), nulls, lead)], ph.T_BYTE_ARRAY, codec, True, pad, long)) == [t if ok else None for t, ok in zip(texts, valid)]
        # a dictionary page and its indices; several pages in one chunk
        entries = rng.integers(-(1 << 62), 1 << 62, 5).astype("<i8")
        idx = [int(x) for x in rng.integers(0, 5, n)]
        draw = entries.tobytes()
        iraw = bytes([3]) + ph.hybrid([("bp", idx[:96]), ("rle", 50, idx[96]), ("bp", idx[146:])], 3)
        idx[96:146] = [idx[96]] * 50
        pages = [ph.Page(ph.DICT, 5, ph.E_PLAIN, compress(codec, draw), len(draw)), ph.Page(ph.V1, n, ph.E_RLE_DICTIONARY, compress(codec, iraw), len(iraw)),
                 ph.Page(ph.V2, n, ph.E_RLE_DICTIONARY, compress(codec, iraw), len(iraw))]
        assert read(ph.hand_object(pages, ph.T_INT64, codec, False, pad, long)) == [int(entries[i]) for i in idx] * 2
        # DELTA_BINARY_PACKED and DELTA_LENGTH_BYTE_ARRAY
        raw = ph.delta_binary_packed(want_i)
        assert read(ph.hand_object([ph.Page(ph.V1, n, ph.E_DELTA_BINARY_PACKED, compress(codec, raw), len(raw))], ph.T_INT64, codec, False, pad, long)) == want_i
        raw = ph.delta_binary_packed([len(t) for t in texts]) + b"".join(texts)
        assert read(ph.hand_object([ph.Page(ph.V1, n, ph.E_DELTA_LENGTH_BYTE_ARRAY, compress(codec, raw), len(raw))], ph.T_BYTE_ARRAY, codec, False, pad, long)) == texts


@pytest.mark.parametrize("codec", [ph.C_SNAPPY, ph.C_LZ4_RAW])
def test_stream_decoders_equal_pyarrows_codecs(codec):
    """every stream the device tests generate: pyarrow's decompressor accepts it and the plain decoder gives the same bytes"""
    c = pa.Codec(CODECS[codec])

    def same(s, want, what):
        assert c.decompress(s, decompressed_size=len(want)).to_pybytes() == want, what

    for total, seed in ph.ELEMENT_CASES:
        s, want = ph.element_stream(codec, total, seed)
        assert len(want) == total
        same(s, want, (total, seed))
    for g in ph.PHASE_GROUPS:
        lead, s, values = ph.phase_page(codec, g, g)
        assert (len(lead) & 15) == (g + 2) & 15 and decode(codec, s) == values.tobytes()
        same(s, values.tobytes(), g)
        assert read(ph.hand_object([ph.Page(ph.V2, 8 * g, ph.E_PLAIN, s, values.nbytes, 0, lead)], ph.T_INT64, codec, True, g & 3)) == [int(v) for v in values]
    for mis in range(4):
        for label, s in ph.seam_streams(codec, mis):
            want = decode(codec, s)
            assert len(want) % 8 == 0, label
            same(s, want, label)
    for n in (9, 64, 200, 1000):
        for k, pattern in enumerate(ph.NULL_PATTERNS):
            valid, values, body = ph.optional_v1_body(n, pattern, n + k)
            s = ph.encode_payload(body, np.random.default_rng(n + k), codec)
            assert decode(codec, s) == body
            same(s, body, (n, pattern))
            it = iter(values)
            assert read(ph.hand_object([ph.Page(ph.V1, n, ph.E_PLAIN, s, len(body))], ph.T_INT64, codec, True)) == [int(next(it)) if ok else None for ok in valid]


def _prefix_wants(body, index):
    """what the host's walk asks its prefix decoder for on an optional v1 page (tf_parquet.hip, the device-inflate branch of the page walk):
    the 4-byte length, then the levels — and the width byte of dictionary indices"""
    return [4, 4 + int.from_bytes(body[:4], "little") + (1 if index else 0)]


def _ends_inside(codec, stream, want):
    """"copy" / "literal" when output byte `want` is strictly inside such an element (bytes of it on both sides of the prefix's end), else None"""
    tr = []
    ph.snappy_decode(stream, tr) if codec == ph.C_SNAPPY else ph.lz4_decode(stream, tr)
    for e in tr:
        spans = [("copy" if e[0] else "literal", e[3], e[1])] if codec == ph.C_SNAPPY else [("literal", e[3], e[0]), ("copy", e[3] + e[0], e[1])]
        for what, at, n in spans:
            if at < want < at + n:
                return what
    return None


@pytest.mark.parametrize("codec", [ph.C_SNAPPY, ph.C_LZ4_RAW])
def test_prefix_reads_end_inside_literals_and_inside_copies(codec):
    """every prefix read tests/test_gpu_parquet_pages.py::test_host_decoders_and_prefix_reads makes: pyarrow's codec and the plain decoder agree
    on the streams, pyarrow reads the pages, and the prefix ends fall strictly inside literals (the random elements) AND strictly inside copies
    (ph.straddle_page: every one of its pages, at the end of the levels / behind the width byte)"""
    c = pa.Codec(CODECS[codec])
    ends = {"copy": 0, "literal": 0, None: 0}
    for n in (9, 64, 200, 1000):
        for k, pattern in enumerate(ph.NULL_PATTERNS):
            valid, values, body = ph.optional_v1_body(n, pattern, n + k)
            for want in _prefix_wants(body, False):
                ends[_ends_inside(codec, ph.encode_payload(body, np.random.default_rng(n + k), codec), want)] += 1
            valid, idx, pages = ph.index_page_pages(codec, n, k)
            for p in pages:
                raw = decode(codec, p.body)
                assert len(raw) == p.usize and c.decompress(p.body, decompressed_size=p.usize).to_pybytes() == raw, (n, pattern)
            for want in _prefix_wants(decode(codec, pages[1].body), True):
                ends[_ends_inside(codec, pages[1].body, want)] += 1
            it = iter(idx)
            assert read(ph.hand_object(pages, ph.T_INT64, codec, True)) == [int(ph.INDEX_ENTRIES[next(it)]) if ok else None for ok in valid]
    assert ends["literal"] > 0
    for index in (False, True):
        for seed in ph.STRADDLE_SEEDS:
            valid, got, stream, body, want = ph.straddle_page(codec, index, seed)
            assert decode(codec, stream) == body and c.decompress(stream, decompressed_size=len(body)).to_pybytes() == body
            assert want == _prefix_wants(body, index)[1] and _ends_inside(codec, stream, want) == "copy", (index, seed)
            ends["copy"] += 1
            pages = [ph.Page(ph.V1, len(valid), ph.E_RLE_DICTIONARY if index else ph.E_PLAIN, stream, len(body))]
            if index:
                pages.insert(0, ph.Page(ph.DICT, 2, ph.E_PLAIN, compress(codec, ph.INDEX_ENTRIES[:2].tobytes()), 16))
            it = iter(got)
            assert read(ph.hand_object(pages, ph.T_INT64, codec, True, seed % 4)) == [int(ph.INDEX_ENTRIES[next(it)] if index else next(it)) if ok else None for ok in valid]
    assert ends["copy"] >= 2 * len(ph.STRADDLE_SEEDS) and ends["literal"] > 0, ends


def test_hybrid_pages_under_snappy_are_streams_pyarrow_inflates():
    """the compressed pages of test_hybrid_index_widths_and_run_shapes: the same builder, the same seeds"""
    c = pa.Codec("snappy")
    for bw in range(33):
        for ending in ("padded", "overshoot"):
            want, pages = ph.hybrid_pages(bw, ending, ph.C_SNAPPY)
            for p in pages:
                raw = ph.snappy_decode(p.body)
                assert len(raw) == p.usize and c.decompress(p.body, decompressed_size=p.usize).to_pybytes() == raw, (bw, ending)
            assert raw == ph.hybrid_pages(bw, ending, ph.C_NONE)[1][1].body
            assert read(ph.hand_object(pages, ph.T_INT64, ph.C_SNAPPY)) == [int(ph.HYBRID_ENTRIES[i]) for i in want], (bw, ending)


def test_the_random_streams_hold_the_forms_they_are_for():
    """what no compressor emits is in the seeded streams — counted here, so a change of generator or seed cannot quietly lose a form"""
    sn, lz = [], []
    for total, seed in ph.ELEMENT_CASES:
        ph.snappy_decode(ph.element_stream(ph.C_SNAPPY, total, seed)[0], sn)
        ph.lz4_decode(ph.element_stream(ph.C_LZ4_RAW, total, seed)[0], lz)
    lits = [e for e in sn if e[0] == 0]
    copies = [e for e in sn if e[0]]
    assert {e[2] for e in lits} == {0, 1, 2, 3, 4}                                     # every count of length bytes
    assert {e[2] for e in lits if e[1] < 60} == {0, 1, 2, 3, 4}                          # the non-minimal forms
    assert {1, 3, 59, 60, 61, 64, 255, 256, 257, 511, 600, 5000, 70000} <= {e[1] for e in lits}
    for kind in (1, 2, 3):
        assert {e[1] for e in copies if e[0] == kind} >= set(range(4, 12) if kind == 1 else range(1, 65)), kind
    assert any(e[0] == 3 and e[2] > 65535 for e in copies)
    assert any(e[2] < e[1] and e[2] < 64 for e in copies) and any(e[2] == e[3] for e in copies)   # periods; the page's first byte
    offs = {e[2] for e in copies}, {e[2] for e in lz if e[1]}
    for got in offs:
        assert {e for e in ph.OFFSET_EDGES if e < 65536 or got is offs[0]} <= got, sorted(set(ph.OFFSET_EDGES) - got)
        for r in ph.RINGS:                                                               # each ring's far-source path: r - 128 < offset
            assert any(r - 128 < o <= r for o in got) and (r == 65536 or any(o > r for o in got))
    assert {0, 1, 14, 15, 16, 269, 270, 271, 524, 525, 6000, 70000} <= {e[0] for e in lz}
    assert {4, 5, 18, 19, 20, 64, 65, 273, 274, 275, 529, 1000, 70000} <= {e[1] for e in lz}
    # the payload encoder: copies of kinds 2 and 3 from length 1, literals of 1..8 bytes with every count of length bytes
    tr = []
    for g in ph.PHASE_GROUPS:
        ph.snappy_decode(ph.phase_page(ph.C_SNAPPY, g, g)[1], tr)
    assert {e[0] for e in tr} == {0, 2, 3} and {1, 2, 3} <= {e[1] for e in tr if e[0]} and {e[2] for e in tr if e[0] == 0 and e[1] <= 8} == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("codec", [ph.C_SNAPPY, ph.C_LZ4_RAW])
def test_malformed_streams_are_refused_by_the_plain_decoder_and_by_pyarrow(codec):
    c = pa.Codec(CODECS[codec])
    for label, s, usize in ph.malformed_streams(codec):
        try:
            assert len(decode(codec, s)) != usize, label
        except ValueError:
            pass
        with pytest.raises(Exception):
            got = c.decompress(s, decompressed_size=usize)
            assert len(got) != usize


def test_hybrid_decoder_equals_pyarrows_reading():
    """index widths 0..32 over both endings: the plain decoder gives the intended indices; pyarrow reads the page through the dictionary — a
    width it refuses is listed in `refused` (the plain decoder alone is the expectation there)"""
    entries = np.array([11, -22, 33, -44, 1 << 61], "<i8")
    refused = []
    for bw in range(33):
        for ending in ("padded", "overshoot"):
            s, want = ph.hybrid_case(bw, ending, 1)
            assert ph.hybrid_decode(s, bw, len(want)) == want, (bw, ending)
            top = min(5, 1 << bw)
            pages = [ph.Page(ph.DICT, top, ph.E_PLAIN, entries[:top].tobytes()), ph.Page(ph.V1, len(want), ph.E_RLE_DICTIONARY, bytes([bw]) + s)]
            try:
                got = read(ph.hand_object(pages))
            except Exception as ex:
                refused.append((bw, ending, str(ex)[:60]))
                continue
            assert got == [int(entries[i]) for i in want], (bw, ending)
    assert not [r for r in refused if r[0] <= 15], refused
    print("pyarrow refused:", refused)


@pytest.mark.parametrize("bits,lengths", [(64, False), (32, False), (32, True)])
def test_delta_decoder_equals_pyarrows_reading(bits, lengths):
    """every block geometry, count, style and unused-width byte: the plain decoder gives the values back; pyarrow reads the pages — a
    geometry it refuses is listed (the plain decoder alone is the expectation there)"""
    refused = []
    for block, mpb in ph.DELTA_GEOMETRIES:
        cases = ph.delta_pages(block, mpb, bits, lengths)
        pages, want = [], []
        for v, s in cases:
            got, end = ph.delta_decode(s, bits)
            assert got == v and end == len(s), (block, mpb, len(v))
            if lengths:
                text = bytes(65 + (i * 7 + len(v)) % 26 for i in range(sum(v)))
                pages.append(ph.Page(ph.V1, len(v), ph.E_DELTA_LENGTH_BYTE_ARRAY, s + text))
                at = np.concatenate(([0], np.cumsum(v)))
                want += [text[at[i]:at[i + 1]] for i in range(len(v))]
            else:
                pages.append(ph.Page(ph.V1, len(v), ph.E_DELTA_BINARY_PACKED, s))
                want += v
        try:
            got = read(ph.hand_object(pages, ph.T_BYTE_ARRAY if lengths else ph.T_INT32 if bits == 32 else ph.T_INT64))
        except Exception as ex:
            refused.append((block, mpb, str(ex)[:60]))
            continue
        assert got == want, (block, mpb)
    assert (128, 4) not in [r[:2] for r in refused], refused
    print("pyarrow refused:", refused)
