"""The page kernels of tf_parquet.hip — pq_inflate (SNAPPY, LZ4_RAW), pq_hybrid, pq_delta — and the host decoders beside them, on HAND-BUILT
pages no writer emits: every element form of both codecs on every LDS ring size, every output phase and input misalignment, elements
across the register windows' seams, malformed streams, prefix reads that end inside an element, index widths 0..32 and every run shape,
DELTA_BINARY_PACKED blocks of every geometry.  Expected: the plain decoders of tests/parquet_hand.py, which tests/test_parquet_hand.py
pins to pyarrow on the same streams.  Equality is exact; every test asserts through the profile that the kernel it aims at ran."""
import numpy as np
import pytest

import parquet_hand as ph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tf():
    from transferia_amd import lib
    lib.init()
    return lib


def kernels_of(tf, fn):
    tf.prof_reset(); tf.prof_enable(True)
    try:
        out = fn()
    finally:
        names = {n for n, l, ms in tf.prof_get() if l}
        tf.prof_enable(False)
    return out, names


def read(tf, obj, kernel):
    """column `c` of the object, downloaded — and `kernel` ran"""
    out, names = kernels_of(tf, lambda: tf.parquet_read(obj).download())
    assert kernel in names, (kernel, names)
    return out.col("c")


def refused(tf, obj, what):
    with pytest.raises(tf.TfgpuError) as ei:
        tf.parquet_read(obj).free()
    assert ei.value.code == tf.ERR_INVALID, (what, str(ei.value))


@pytest.mark.parametrize("total", sorted({t for t, _ in ph.ELEMENT_CASES}))
@pytest.mark.parametrize("codec", [ph.C_SNAPPY, ph.C_LZ4_RAW], ids=["snappy", "lz4_raw"])
@pytest.mark.parametrize("ring", [16, 32, 64])
def test_every_element_form_on_every_ring(tf, ring, codec, total, monkeypatch):
    """seeded random element streams (ph.random_snappy / ph.random_lz4): literal and match lengths around every length-extension step, all
    three snappy copy kinds from length 1, offsets over short periods, the whole page, the largest legal ones, the edges of each ring's
    far-source threshold and — snappy's 4-byte form — beyond 65535; v1 required pages alternate with v2 optional ones, pad = seed mod 4"""
    monkeypatch.setenv("TFGPU_PQ_RING_KB", str(ring))
    monkeypatch.setenv("TFGPU_PQ_DEVICE_INFLATE", "1")
    for t, seed in ph.ELEMENT_CASES:
        if t != total:
            continue
        stream, want = ph.element_stream(codec, total, seed)
        obj = ph.values_object(stream, total, codec, ph.V2 if seed & 1 else ph.V1, seed % 4)
        c = read(tf, obj, "pq_inflate")
        assert c.values.tobytes() == want, (ring, codec, total, seed)
        assert c.validity is None or c.validity.all()


@pytest.mark.parametrize("codec", [ph.C_SNAPPY, ph.C_LZ4_RAW], ids=["snappy", "lz4_raw"])
@pytest.mark.parametrize("groups", list(ph.PHASE_GROUPS))
def test_every_output_phase_and_input_misalignment(tf, groups, codec, monkeypatch):
    """v2 optional pages whose level bytes make (lead & 15) each of 0..15 — the ring position of output byte 0 — crossed with pad 0..3 (the
    compressed bytes' misalignment); short elements, then one stored literal of 20 000 bytes: the long literal's head, chunks and tail
    and several flushes of the 16 KiB ring at that phase"""
    monkeypatch.setenv("TFGPU_PQ_RING_KB", "16")
    monkeypatch.setenv("TFGPU_PQ_DEVICE_INFLATE", "1")
    lead, stream, values = ph.phase_page(codec, groups, groups)
    assert (len(lead) & 15) == (groups + 2) & 15
    seen = set()
    for pad in range(4):
        at = []
        obj = ph.hand_object([ph.Page(ph.V2, 8 * groups, ph.E_PLAIN, stream, values.nbytes, 0, lead)], ph.T_INT64, codec, True, pad, body_at=at)
        seen.add((at[0] + len(lead)) & 3)
        c = read(tf, obj, "pq_inflate")
        assert c.values.tobytes() == values.tobytes(), (groups, codec, pad)
        assert c.validity is None or c.validity.all()
    assert seen == {0, 1, 2, 3}
    assert {(g + 2) & 15 for g in ph.PHASE_GROUPS} == set(range(16))


@pytest.mark.parametrize("codec", [ph.C_SNAPPY, ph.C_LZ4_RAW], ids=["snappy", "lz4_raw"])
@pytest.mark.parametrize("mis", range(4))
def test_elements_across_the_window_seams(tf, mis, codec, monkeypatch):
    """every element form (snappy literals with 0..4 length bytes, copies of all kinds; LZ4 tokens with 0, 1 and 3 extension bytes a side)
    with its tag at window positions 250..258 and 505..516, and literals whose last byte lands at 510..513 — `pad` is chosen so that the
    page's compressed bytes really start at misalignment `mis`"""
    monkeypatch.setenv("TFGPU_PQ_DEVICE_INFLATE", "1")
    cases = ph.seam_streams(codec, mis)
    assert len(cases) > 150
    for label, stream in cases:
        want = ph.snappy_decode(stream) if codec == ph.C_SNAPPY else ph.lz4_decode(stream)
        at = []
        ph.values_object(stream, len(want), codec, ph.V1, 0, body_at=at)
        pad = (mis - at[0]) & 3
        at = []
        obj = ph.values_object(stream, len(want), codec, ph.V1, pad, body_at=at)
        assert at[0] & 3 == mis
        c = read(tf, obj, "pq_inflate")
        assert c.values.tobytes() == want, (label, mis)


@pytest.mark.parametrize("codec", [ph.C_SNAPPY, ph.C_LZ4_RAW], ids=["snappy", "lz4_raw"])
@pytest.mark.parametrize("mode,ring", [("1", 16), ("1", 64), ("0", 64)])
def test_malformed_hand_built_pages_are_refused(tf, mode, ring, codec, monkeypatch):
    """one broken place a page (ph.malformed_streams): TFGPU_ERR_INVALID from the device's inflate (rings 16 and 64) and from the host's"""
    # Who refuses: the pages are v1 PLAIN pages of a REQUIRED column, of which the host's walk reads nothing (no levels, no width byte: no prefix
    # read) — in mode "1" the refusal is pq_inflate's own (PQE_INFLATE), in mode "0" snappy_inflate's / lz4_raw_inflate's.  The routing is shown
    # on a good page first; a routing change that sends such pages elsewhere has to revisit this test.
    monkeypatch.setenv("TFGPU_PQ_RING_KB", str(ring))
    monkeypatch.setenv("TFGPU_PQ_DEVICE_INFLATE", mode)
    good, want = ph.element_stream(codec, 4096, 0)
    _, names = kernels_of(tf, lambda: tf.parquet_read(ph.values_object(good, 4096, codec)).download())
    assert ("pq_inflate" in names) == (mode == "1")          # this mode does route such a page where the test aims
    for label, stream, usize in ph.malformed_streams(codec):
        for pad in (0, 1):
            refused(tf, ph.values_object(stream, usize, codec, ph.V1, pad), label)


def check_optional(c, valid, values, what):
    got_valid = c.validity if c.validity is not None else np.ones(len(valid), bool)
    assert np.array_equal(np.asarray(got_valid, bool), valid), what
    assert np.array_equal(np.asarray(c.values)[valid], values), what


@pytest.mark.parametrize("codec", [ph.C_SNAPPY, ph.C_LZ4_RAW], ids=["snappy", "lz4_raw"])
@pytest.mark.parametrize("mode", ["1", "0"])
def test_host_decoders_and_prefix_reads(tf, mode, codec, monkeypatch):
    """optional v1 pages (a 4-byte length, RLE levels, the values) cut into short random elements, so the end of the levels falls inside
    copies and inside literals that go on: mode 1 reads the levels through snappy_inflate_prefix / lz4_raw_inflate_prefix and the values
    through pq_inflate, mode 0 all of it through snappy_inflate / lz4_raw_inflate; (mode 1) the same through dictionary indices,
    whose width byte is part of the prefix; and hand-placed copies that straddle the prefix's end (tests/test_parquet_hand.py counts, per
    codec, the prefix ends that fall strictly inside a literal and strictly inside a copy)"""
    monkeypatch.setenv("TFGPU_PQ_DEVICE_INFLATE", mode)
    entries = ph.INDEX_ENTRIES
    for n in (9, 64, 200, 1000):
        for k, pattern in enumerate(ph.NULL_PATTERNS):
            valid, values, body = ph.optional_v1_body(n, pattern, n + k)
            stream = ph.encode_payload(body, np.random.default_rng(n + k), codec)
            obj = ph.hand_object([ph.Page(ph.V1, n, ph.E_PLAIN, stream, len(body))], ph.T_INT64, codec, True, (n + k) % 4)
            out, names = kernels_of(tf, lambda: tf.parquet_read(obj).download())
            assert ("pq_inflate" in names) == (mode == "1"), names
            check_optional(out.col("c"), valid, values, (n, pattern))
            if mode == "1":
                valid, idx, pages = ph.index_page_pages(codec, n, k)
                out, names = kernels_of(tf, lambda: tf.parquet_read(ph.hand_object(pages, ph.T_INT64, codec, True, k % 4)).download())
                assert {"pq_inflate", "pq_hybrid"} <= names, names
                check_optional(out.col("c"), valid, entries[idx], (n, pattern, "indices"))
    # one copy that begins inside what the prefix read wants and ends behind it (ph.straddle_page: the random elements above never do that —
    # fresh values do not repeat the level bytes): behind the levels of a PLAIN page, behind the width byte of an index page
    for seed in ph.STRADDLE_SEEDS:
        valid, values, stream, body, want = ph.straddle_page(codec, False, seed)
        obj = ph.hand_object([ph.Page(ph.V1, len(valid), ph.E_PLAIN, stream, len(body))], ph.T_INT64, codec, True, seed % 4)
        out, names = kernels_of(tf, lambda: tf.parquet_read(obj).download())
        assert ("pq_inflate" in names) == (mode == "1"), names
        check_optional(out.col("c"), valid, values, ("straddle", seed))
        valid, idx, stream, body, want = ph.straddle_page(codec, True, seed)
        draw = entries[:2].tobytes()
        pages = [ph.Page(ph.DICT, 2, ph.E_PLAIN, ph.encode_payload(draw, np.random.default_rng(seed), codec), len(draw)), ph.Page(ph.V1, len(valid), ph.E_RLE_DICTIONARY, stream, len(body))]
        out, names = kernels_of(tf, lambda: tf.parquet_read(ph.hand_object(pages, ph.T_INT64, codec, True, seed % 4)).download())
        assert "pq_hybrid" in names and ("pq_inflate" in names) == (mode == "1"), names
        check_optional(out.col("c"), valid, entries[np.asarray(idx)], ("straddle indices", seed))


ENTRIES = ph.HYBRID_ENTRIES


@pytest.mark.parametrize("codec", [ph.C_NONE, ph.C_SNAPPY], ids=["stored", "snappy"])
@pytest.mark.parametrize("bw", range(33))
def test_hybrid_index_widths_and_run_shapes(tf, bw, codec, monkeypatch):
    """pq_hybrid at index widths 0..32: RLE runs whose counts take one, two and three varint bytes, bit-packed runs of 1..17 groups, a last
    bit-packed group that is partly padding, a last RLE run that states more values than the page has left — uncompressed, and under
    SNAPPY with the indices inflated on the device first"""
    monkeypatch.setenv("TFGPU_PQ_DEVICE_INFLATE", "1")
    for ending in ("padded", "overshoot"):
        want, pages = ph.hybrid_pages(bw, ending, codec)
        out, names = kernels_of(tf, lambda: tf.parquet_read(ph.hand_object(pages, ph.T_INT64, codec, False, bw % 4)).download())
        assert "pq_hybrid" in names and (codec == ph.C_NONE or "pq_inflate" in names), names
        assert np.array_equal(out.col("c").values, ENTRIES[np.asarray(want)]), (bw, ending)


def test_malformed_hybrid_streams_are_refused(tf):
    """a width byte of 33, a run of count 0 (RLE and bit-packed), a stream that ends inside a run (its header, its value, its groups)"""
    good = [ph.Page(ph.DICT, 5, ph.E_PLAIN, ENTRIES.tobytes()), ph.Page(ph.V1, 100, ph.E_RLE_DICTIONARY, bytes([3]) + ph.hybrid([("rle", 60, 2), ("bp", [1] * 40)], 3))]
    c = read(tf, ph.hand_object(good), "pq_hybrid")
    assert np.array_equal(c.values, ENTRIES[[2] * 60 + [1] * 40])
    rle, bp = ph.hybrid([("rle", 60, 2)], 3), ph.hybrid([("bp", [1] * 40)], 3)
    rle17 = ph.hybrid([("rle", 60, 70000)], 17)
    for label, body in [("width 33", bytes([33]) + rle + bp), ("RLE run of count 0", bytes([3]) + rle + b"\x00\x02" + bp), ("bit-packed run of no groups", bytes([3]) + rle + b"\x01" + bp),
                        ("ends before a run header", bytes([3]) + rle), ("ends inside a run header", bytes([3]) + rle + b"\x81"), ("ends inside an RLE value", bytes([17]) + rle17[:-1]),
                        ("ends inside the bit-packed groups", bytes([3]) + rle + bp[:-1])]:
        refused(tf, ph.hand_object([good[0], ph.Page(ph.V1, 100, ph.E_RLE_DICTIONARY, body)]), label)


@pytest.mark.parametrize("kind", ["int64", "int32", "lengths"])
@pytest.mark.parametrize("geometry", ph.DELTA_GEOMETRIES, ids=["%dx%d" % g for g in ph.DELTA_GEOMETRIES])
def test_delta_block_geometries(tf, geometry, kind):
    """pq_delta over blocks of 128..1024 values in 1..8 miniblocks (32, 64, 128 and 256 values a miniblock: the wave carries its running
    value through up to four rounds of one miniblock), counts that end in every part of a block, deltas of width 0, 1 and of nearly all
    bits with wrap-around, unused trailing miniblocks whose width bytes are 0 and 0xFF; INT64, INT32, and the same streams as the lengths
    of DELTA_LENGTH_BYTE_ARRAY pages.  80 pages a chunk: one wave each, twenty workgroups."""
    block, mpb = geometry
    bits, lengths = (64, False) if kind == "int64" else (32, kind == "lengths")
    pages, want, texts = [], [], []
    for v, s in ph.delta_pages(block, mpb, bits, lengths):
        assert ph.delta_decode(s, bits) == (v, len(s))
        want += v
        if lengths:
            texts.append(bytes(65 + (i * 7 + len(v)) % 26 for i in range(sum(v))))
            pages.append(ph.Page(ph.V1, len(v), ph.E_DELTA_LENGTH_BYTE_ARRAY, s + texts[-1]))
        else:
            pages.append(ph.Page(ph.V1, len(v), ph.E_DELTA_BINARY_PACKED, s))
    c = read(tf, ph.hand_object(pages, ph.T_BYTE_ARRAY if lengths else ph.T_INT32 if bits == 32 else ph.T_INT64), "pq_delta")
    if lengths:
        assert [int(x) for x in np.diff(np.asarray(c.offsets, np.int64))] == want
        assert bytes(c.data[:int(c.offsets[-1])]) == b"".join(texts)
    else:
        assert [int(x) for x in c.values] == want


def test_delta_geometries_the_reader_refuses(tf):
    """a block that is no multiple of 128, miniblocks that are no multiple of 32, no miniblocks at all: a clean error"""
    v = list(range(0, 600, 3))
    good = ph.delta_binary_packed(v, 256, 2)
    assert [int(x) for x in read(tf, ph.hand_object([ph.Page(ph.V1, len(v), ph.E_DELTA_BINARY_PACKED, good)]), "pq_delta").values] == v
    for block, mpb in ((100, 1), (64, 2), (192, 2), (128, 8), (256, 16)):
        s = ph.delta_binary_packed(v, block, mpb)
        with pytest.raises(ValueError):
            ph.delta_decode(s)
        refused(tf, ph.hand_object([ph.Page(ph.V1, len(v), ph.E_DELTA_BINARY_PACKED, s)]), (block, mpb))
    none = ph.uvarint(128) + ph.uvarint(0) + good[3:]
    refused(tf, ph.hand_object([ph.Page(ph.V1, len(v), ph.E_DELTA_BINARY_PACKED, none)]), "no miniblocks")
