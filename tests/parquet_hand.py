"""Hand-built Parquet objects: a minimal writer (Thrift compact metadata, page headers, one column chunk) and byte-level builders for
the streams inside the pages — snappy elements of every form, LZ4 sequences, RLE / bit-packed hybrid runs, DELTA_BINARY_PACKED blocks
of any geometry — with one plain reference decoder per format, each a direct loop over the public format description (snappy
format_description.txt, lz4_Block_format.md, parquet-format Encodings.md).  A compressor emits a narrow dialect of its format; the
page kernels of tf_parquet.hip implement all of it.  TEST INFRASTRUCTURE: tests/test_parquet_hand.py pins every builder and decoder
here to pyarrow, tests/test_gpu_parquet_pages.py reads the objects on the device.  Imports only struct and numpy."""
import struct

import numpy as np

# parquet.thrift
T_INT32, T_INT64, T_BYTE_ARRAY = 1, 2, 6
E_PLAIN, E_RLE, E_DELTA_BINARY_PACKED, E_DELTA_LENGTH_BYTE_ARRAY, E_RLE_DICTIONARY = 0, 3, 5, 6, 8
C_NONE, C_SNAPPY, C_LZ4_RAW = 0, 1, 7
DICT, V1, V2 = 2, 0, 3   # PageType: DICTIONARY_PAGE, DATA_PAGE, DATA_PAGE_V2


# ---- Thrift compact protocol ---------------------------------------------------------------------------------------------
def uvarint(v):
    assert v >= 0
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def zigzag(v):
    return uvarint((v << 1) ^ (v >> 63))


class TStruct:
    """one struct: fields in ascending id order; a header is (id delta << 4 | type), or — delta outside 1..15, or long=True — the type
    alone followed by the zigzag id"""
    def __init__(self, long=False):
        self.b, self.last, self.long = bytearray(), 0, long

    def _hdr(self, fid, ty):
        d = fid - self.last
        if 0 < d <= 15 and not self.long:
            self.b.append((d << 4) | ty)
        else:
            self.b.append(ty)
            self.b += zigzag(fid)
        self.last = fid

    def i32(self, fid, v):
        self._hdr(fid, 5)
        self.b += zigzag(v)

    def i64(self, fid, v):
        self._hdr(fid, 6)
        self.b += zigzag(v)

    def boolean(self, fid, v):
        self._hdr(fid, 1 if v else 2)

    def binary(self, fid, s):
        self._hdr(fid, 8)
        self.b += uvarint(len(s)) + s

    def struct(self, fid, st):
        self._hdr(fid, 12)
        self.b += st.done()

    def list(self, fid, ety, items):
        """items: encoded elements (ety 5 / 6: zigzag varints, 8: length-prefixed, 12: structs)"""
        self._hdr(fid, 9)
        n = len(items)
        self.b += bytes([(n << 4) | ety]) if n < 15 else bytes([0xF0 | ety]) + uvarint(n)
        for it in items:
            self.b += it

    def done(self):
        return bytes(self.b) + b"\x00"


# ---- the object ----------------------------------------------------------------------------------------------------------
class Page:
    """kind: DICT / V1 / V2.  body: the bytes as stored behind `lead` (a v2 page's definition levels, stored as they are); usize: the size
    the header states `body` inflates to (default: its own length, an uncompressed page)."""
    def __init__(self, kind, num_values, encoding, body, usize=None, num_nulls=0, lead=b""):
        assert kind == V2 or not lead
        self.kind, self.num_values, self.encoding, self.body, self.num_nulls, self.lead = kind, num_values, encoding, bytes(body), num_nulls, bytes(lead)
        self.usize = len(self.body) if usize is None else usize


def page_header(p, long=False):
    h = TStruct(long)
    h.i32(1, p.kind)
    h.i32(2, len(p.lead) + p.usize)
    h.i32(3, len(p.lead) + len(p.body))
    if p.kind == V1:
        d = TStruct(long)
        d.i32(1, p.num_values); d.i32(2, p.encoding); d.i32(3, E_RLE); d.i32(4, E_RLE)
        h.struct(5, d)
    elif p.kind == DICT:
        d = TStruct(long)
        d.i32(1, p.num_values); d.i32(2, p.encoding)
        h.struct(7, d)
    else:
        d = TStruct(long)
        d.i32(1, p.num_values); d.i32(2, p.num_nulls); d.i32(3, p.num_values); d.i32(4, p.encoding)
        d.i32(5, len(p.lead)); d.i32(6, 0); d.boolean(7, True)
        h.struct(8, d)
    return h.done()


def hand_object(pages, ptype=T_INT64, codec=C_NONE, optional=False, pad=0, long=False, body_at=None):
    """PAR1, `pad` filler bytes, the pages of one column chunk `c` each under its PageHeader, the FileMetaData, its length, PAR1.
    body_at (a list): receives the file offset of every page's stored bytes (its `lead` first)."""
    out = bytearray(b"PAR1" + b"\xA5" * pad)
    first = len(out)
    dict_at = data_at = None
    rows = tot_c = tot_u = 0
    encodings = []
    for p in pages:
        if p.kind == DICT and dict_at is None:
            dict_at = len(out)
        if p.kind != DICT and data_at is None:
            data_at = len(out)
        h = page_header(p, long)
        out += h
        if body_at is not None:
            body_at.append(len(out))
        out += p.lead + p.body
        tot_c += len(h) + len(p.lead) + len(p.body)
        tot_u += len(h) + len(p.lead) + p.usize
        if p.kind != DICT:
            rows += p.num_values
        if p.encoding not in encodings:
            encodings.append(p.encoding)
    if E_RLE not in encodings:
        encodings.append(E_RLE)
    assert data_at is not None and (dict_at is None or dict_at == first)
    root = TStruct(long)
    root.binary(4, b"schema"); root.i32(5, 1)
    leaf = TStruct(long)
    leaf.i32(1, ptype); leaf.i32(3, 1 if optional else 0); leaf.binary(4, b"c")
    cm = TStruct(long)
    cm.i32(1, ptype)
    cm.list(2, 5, [zigzag(e) for e in encodings])
    cm.list(3, 8, [uvarint(1) + b"c"])
    cm.i32(4, codec); cm.i64(5, rows); cm.i64(6, tot_u); cm.i64(7, tot_c); cm.i64(9, data_at)
    if dict_at is not None:
        cm.i64(11, dict_at)
    cc = TStruct(long)
    cc.i64(2, first); cc.struct(3, cm)
    rg = TStruct(long)
    rg.list(1, 12, [cc.done()]); rg.i64(2, tot_u); rg.i64(3, rows)
    fm = TStruct(long)
    fm.i32(1, 1); fm.list(2, 12, [root.done(), leaf.done()]); fm.i64(3, rows); fm.list(4, 12, [rg.done()])
    fm.binary(6, b"hand-built")
    footer = fm.done()
    out += footer + struct.pack("<I", len(footer)) + b"PAR1"
    return bytes(out)


# ---- snappy (format_description.txt) ---------------------------------------------------------------------------------------
def sn_preamble(n):
    return uvarint(n)


def sn_literal(data, nb=None):
    """a literal element; nb: the number of length bytes behind the tag (None: the fewest) — 0 only up to 60 bytes, otherwise any count
    that holds len - 1 (the format allows the non-minimal forms)"""
    n = len(data)
    assert 1 <= n <= 1 << 32
    least = 0 if n <= 60 else (n - 1).bit_length() + 7 >> 3
    nb = least if nb is None else nb
    assert 0 <= nb <= 4 and nb >= least and (nb or n <= 60), (n, nb)
    if nb == 0:
        return bytes([(n - 1) << 2]) + bytes(data)
    return bytes([(59 + nb) << 2]) + (n - 1).to_bytes(nb, "little") + bytes(data)


def sn_copy(length, off, kind):
    if kind == 1:
        assert 4 <= length <= 11 and 0 <= off < 2048
        return bytes([1 | (length - 4) << 2 | (off >> 8) << 5, off & 0xFF])
    assert 1 <= length <= 64
    if kind == 2:
        assert 0 <= off < 1 << 16
        return bytes([2 | (length - 1) << 2]) + struct.pack("<H", off)
    assert kind == 3 and 0 <= off < 1 << 32
    return bytes([3 | (length - 1) << 2]) + struct.pack("<I", off)


def snappy_decode(buf, trace=None):
    """the stream inflated, element by element; ValueError where the format is broken.  trace (a list): receives every element as
    (kind — 0 a literal, its length, its offset | a literal's count of length bytes, where its output starts)"""
    p = n = sh = 0
    while True:
        if p >= len(buf) or sh > 28:
            raise ValueError("preamble")
        b = buf[p]; p += 1
        n |= (b & 0x7F) << sh; sh += 7
        if not b & 0x80:
            break
    out = bytearray()
    while p < len(buf):
        tag = buf[p]; p += 1
        kind = tag & 3
        if kind == 0:
            length = (tag >> 2) + 1
            nb = 0
            if length > 60:
                nb = length - 60
                if p + nb > len(buf):
                    raise ValueError("literal length cut")
                length = 0
                for i in range(nb):
                    length |= buf[p + i] << (8 * i)
                length += 1
                p += nb
            if p + length > len(buf):
                raise ValueError("literal past the input")
            if trace is not None:
                trace.append((0, length, nb, len(out)))
            for i in range(length):
                out.append(buf[p + i])
            p += length
            continue
        if kind == 1:
            need, length = 1, ((tag >> 2) & 7) + 4
        else:
            need, length = (2 if kind == 2 else 4), (tag >> 2) + 1
        if p + need > len(buf):
            raise ValueError("copy cut")
        off = 0
        for i in range(need):
            off |= buf[p + i] << (8 * i)
        if kind == 1:
            off |= (tag >> 5) << 8
        p += need
        if off == 0 or off > len(out):
            raise ValueError("offset")
        if trace is not None:
            trace.append((kind, length, off, len(out)))
        for _ in range(length):
            out.append(out[-off])
    if len(out) != n:
        raise ValueError("stated %d, holds %d" % (n, len(out)))
    return bytes(out)


# ---- LZ4 block format (lz4_Block_format.md) --------------------------------------------------------------------------------
def _lz4_ext(v):
    """the bytes behind a token nibble of 15: 255s, then the rest (0 included)"""
    v -= 15
    return b"\xFF" * (v // 255) + bytes([v % 255])


def lz4_seq(literals, off=None, match_len=None):
    """one sequence: token, literal length extension, literals, and — unless it is the block's last — a 2-byte offset and the match
    length extension"""
    n = len(literals)
    assert (off is None) == (match_len is None)
    ml = 0 if match_len is None else match_len - 4
    assert ml >= 0
    out = bytes([min(n, 15) << 4 | min(ml, 15)])
    if n >= 15:
        out += _lz4_ext(n)
    out += bytes(literals)
    if off is not None:
        assert 0 <= off < 1 << 16
        out += struct.pack("<H", off)
        if ml >= 15:
            out += _lz4_ext(ml)
    return out


def lz4_match_fits(at, match_len, total):
    """liblz4's end-of-block rules: a match starts at least 12 bytes before the end of the output and the last 5 bytes are literals"""
    return at + 12 <= total and at + match_len + 5 <= total


def lz4_decode(buf, trace=None):
    """trace (a list): receives every sequence as (literal length, match length | 0, offset | 0, where its output starts)"""
    out = bytearray()
    p = 0
    while p < len(buf):
        tok = buf[p]; p += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                if p >= len(buf):
                    raise ValueError("literal length cut")
                b = buf[p]; p += 1
                lit += b
                if b != 255:
                    break
        if p + lit > len(buf):
            raise ValueError("literal past the input")
        for i in range(lit):
            out.append(buf[p + i])
        p += lit
        if p == len(buf):
            if trace is not None:
                trace.append((lit, 0, 0, len(out) - lit))
            break
        if p + 2 > len(buf):
            raise ValueError("offset cut")
        off = buf[p] | buf[p + 1] << 8
        p += 2
        ml = tok & 15
        if ml == 15:
            while True:
                if p >= len(buf):
                    raise ValueError("match length cut")
                b = buf[p]; p += 1
                ml += b
                if b != 255:
                    break
        if off == 0 or off > len(out):
            raise ValueError("offset")
        if trace is not None:
            trace.append((lit, ml + 4, off, len(out) - lit))
        for _ in range(ml + 4):
            out.append(out[-off])
    return bytes(out)


# ---- seeded random element streams (every element form; the same streams on every ring size) ---------------------------------
RINGS = (16384, 32768, 65536)
OFFSET_EDGES = sorted({63, 64, 65, 65408, 65409, 65535} | {r - 128 for r in RINGS} | {r - 127 for r in RINGS} | set(RINGS))
SN_LITERALS = ((1, 3, 59, 60, 61, 64), (255, 256, 257, 511, 600), (5000,))
LZ4_LITERALS = ((0, 1, 14, 15, 16), (269, 270, 271, 524, 525), (6000,))
LZ4_MATCHES = ((4, 5, 18, 19, 20, 64, 65), (273, 274, 275, 529), (1000,))
HUGE = 70000          # one literal (and one LZ4 match) of this length in every stream large enough to hold it


def _tiered(rng, tiers):
    t = rng.random()
    tier = tiers[0] if t < 0.70 else tiers[1] if t < 0.98 else tiers[2]
    return int(tier[int(rng.integers(0, len(tier)))])


def _offset(rng, o, limit, unused):
    """a legal offset (1 .. min(o, limit)) from one of four sets: short periods, anything, the largest, the listed edges — of those first
    the ones this stream has not used yet (`unused`: a list the pick is taken out of)"""
    top = min(o, limit)
    s = int(rng.integers(0, 4))
    if s == 1:
        return int(rng.integers(1, top + 1))
    if s == 2:
        return top - int(rng.integers(0, min(4, top)))
    if s == 3:
        ok = [e for e in unused if e <= top]
        if ok:
            unused.remove(ok[-1])
            return ok[-1]
        ok = [e for e in OFFSET_EDGES if e <= top]
        if ok:
            return int(ok[int(rng.integers(0, len(ok)))])
    return int(rng.integers(1, min(top, 70) + 1))


def random_snappy(total, seed):
    """a snappy stream of `total` output bytes: literals of the listed lengths with any legal count of length bytes, copies of all three
    kinds, lengths 1..64, offsets from the four sets — kind 3 also beyond 65535"""
    rng = np.random.default_rng(seed)
    out = bytearray(sn_preamble(total))
    huge_at = int(rng.integers(0, total - HUGE)) if total > HUGE + 4096 else -1
    unused = list(OFFSET_EDGES)
    o = 0
    while o < total:
        left = total - o
        if huge_at >= 0 and o >= huge_at:
            n, huge_at = HUGE, -1
            out += sn_literal(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), int(rng.integers(3, 5)))
        elif o == 0 or rng.random() < 0.35:
            n = min(_tiered(rng, SN_LITERALS), left)
            least = 0 if n <= 60 else (n - 1).bit_length() + 7 >> 3
            nb = int(rng.integers(least if n <= 60 else max(least, 1), 5))
            out += sn_literal(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), nb)
        else:
            kind = int(rng.integers(1, 4))
            if kind == 1 and left < 4:
                kind = 2
            n = min(int(rng.integers(4, 12)) if kind == 1 else int(rng.integers(1, 65)), left)
            if kind == 3 and o > 65536 and rng.random() < 0.5:
                off = int(rng.integers(65536, o + 1))
            else:
                off = _offset(rng, o, (2047, 65535, (1 << 32) - 1)[kind - 1], unused)
            out += sn_copy(n, off, kind)
        o += n
    return bytes(out)


def random_lz4(total, seed):
    """an LZ4 block of `total` output bytes (total >= 13) under liblz4's end-of-block rules: literal and match lengths around the 15 / 270 / 525
    extension steps, offsets from the four sets"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    huge_at = int(rng.integers(0, total - 2 * HUGE)) if total > 2 * HUGE + 4096 else -1
    unused = list(OFFSET_EDGES)
    o = 0
    while True:
        huge = huge_at >= 0 and o >= huge_at
        lit = HUGE if huge else _tiered(rng, LZ4_LITERALS)
        ml = HUGE if huge else _tiered(rng, LZ4_MATCHES)
        if huge:
            huge_at = -1
        if o + lit == 0:
            lit = 1
        if not lz4_match_fits(o + lit, ml, total):
            ml = total - 5 - (o + lit)                       # the longest match that still fits, if any does
        if ml < 4 or not lz4_match_fits(o + lit, ml, total):
            out += lz4_seq(rng.integers(0, 256, total - o, dtype=np.uint8).tobytes())
            return bytes(out)
        o += lit
        out += lz4_seq(rng.integers(0, 256, lit, dtype=np.uint8).tobytes(), _offset(rng, o, 65535, unused), ml)
        o += ml


def encode_payload(payload, rng, codec, stored_tail=0):
    """`payload` as a stream of many short random elements: literals of 1..8 bytes, copies from any earlier place that matches (the
    nearest or the farthest; snappy: kinds 2 and 3, lengths from 1; LZ4: from 4, under its end-of-block rules).  The last
    `stored_tail` bytes are one stored literal."""
    payload = bytes(payload)
    total = len(payload)
    body = total - stored_tail
    assert body >= 0

    def find(o, want, least):
        k = min(want, body - o)
        while k >= least:
            pat = payload[o:o + k]
            at = payload.rfind(pat, 0, o + k - 1) if rng.random() < 0.5 else payload.find(pat, 0, o + k - 1)
            if 0 <= at < o:
                return k, o - at
            k //= 2
        return 0, 0

    out = bytearray()
    o = 0
    if codec == C_SNAPPY:
        out += sn_preamble(total)
        while o < body:
            n, off = find(o, int(rng.integers(1, 65)), 1) if o and rng.random() < 0.6 else (0, 0)
            if n:
                out += sn_copy(n, off, 3 if off > 65535 or rng.random() < 0.4 else 2)
            else:
                n = min(int(rng.integers(1, 9)), body - o)
                out += sn_literal(payload[o:o + n], int(rng.integers(0, 5)))
            o += n
        if stored_tail:
            out += sn_literal(payload[body:])
        return bytes(out)
    assert codec == C_LZ4_RAW
    start = 0                                                 # where the pending literals begin
    while True:
        o += min(int(rng.integers(0, 9)), body - o)
        n, off = find(o, int(rng.integers(4, 41)), 4) if o else (0, 0)
        while n >= 4 and not (lz4_match_fits(o, n, total) and off < 65536):
            n -= 1
        if n >= 4:
            out += lz4_seq(payload[start:o], off, n)
            o += n
            start = o
        elif o >= body:
            out += lz4_seq(payload[start:])
            return bytes(out)
        else:
            o += 1                                            # no match here: the literals grow


# ---- RLE / bit-packed hybrid (Encodings.md) ----------------------------------------------------------------------------------
def hybrid(runs, bw):
    """runs: ("rle", count, value) or ("bp", values) — a bit-packed run of ceil(len / 8) groups, the last one padded with zeros"""
    out = bytearray()
    for r in runs:
        if r[0] == "rle":
            out += uvarint(r[1] << 1) + int(r[2]).to_bytes((bw + 7) // 8, "little")
        else:
            vals = list(r[1]) + [0] * (-len(r[1]) % 8)
            out += uvarint(len(vals) // 8 << 1 | 1)
            acc = nbits = 0
            for v in vals:
                assert 0 <= v < 1 << bw or (bw == 0 and v == 0)
                acc |= int(v) << nbits
                nbits += bw
            out += acc.to_bytes(nbits // 8, "little")
    return bytes(out)


def hybrid_decode(buf, bw, n):
    """the first n values of the stream (a last run may state more); ValueError: a run of no values, or the stream ends early"""
    out = []
    p = 0
    while len(out) < n:
        h = sh = 0
        while True:
            if p >= len(buf):
                raise ValueError("run header cut")
            b = buf[p]; p += 1
            h |= (b & 0x7F) << sh; sh += 7
            if not b & 0x80:
                break
        if h >> 1 == 0:
            raise ValueError("empty run")
        if h & 1:
            if p + (h >> 1) * bw > len(buf):
                raise ValueError("bit-packed run cut")
            for i in range((h >> 1) * 8):
                v = 0
                for b in range(bw):
                    q = i * bw + b
                    v |= (buf[p + (q >> 3)] >> (q & 7) & 1) << b
                out.append(v)
            p += (h >> 1) * bw
        else:
            nb = (bw + 7) // 8
            if p + nb > len(buf):
                raise ValueError("run value cut")
            v = 0
            for i in range(nb):
                v |= buf[p + i] << (8 * i)
            p += nb
            out.extend([v] * min(h >> 1, n - len(out)))
    return out[:n]


# ---- DELTA_BINARY_PACKED (Encodings.md) --------------------------------------------------------------------------------------
def delta_binary_packed(values, block=128, minis_per_block=4, unused_width_byte=0, bits=64):
    """<block size> <miniblocks per block> <count> <first value>, then blocks of <min delta> <a width byte per miniblock> <miniblocks>.
    Deltas wrap in `bits`-bit arithmetic; the last used miniblock is padded to full size; a miniblock with no value keeps only its
    width byte (`unused_width_byte`: readers must not look at it)."""
    m = (1 << bits) - 1
    half = 1 << (bits - 1)
    vpm = block // minis_per_block
    out = bytearray(uvarint(block) + uvarint(minis_per_block) + uvarint(len(values)) + zigzag(int(values[0]) if len(values) else 0))
    deltas = [((int(values[i + 1]) - int(values[i]) & m) ^ half) - half for i in range(len(values) - 1)]   # signed, wrapped
    for b0 in range(0, len(deltas), block):
        blk = deltas[b0:b0 + block]
        lo = min(blk)
        out += zigzag(lo)
        rel = [(d - lo) & m for d in blk]
        minis = [rel[i:i + vpm] for i in range(0, len(rel), vpm)]
        out += bytes([max(x.bit_length() for x in mb) for mb in minis] + [unused_width_byte] * (minis_per_block - len(minis)))
        for mb in minis:
            bw = max(x.bit_length() for x in mb)
            acc = 0
            for i, x in enumerate(mb):
                acc |= x << (i * bw)
            out += acc.to_bytes(vpm * bw // 8, "little")
    return bytes(out)


def delta_decode(buf, bits=64):
    """(values as signed `bits`-bit integers, the position behind the stream)"""
    pos = [0]

    def varint():
        v = sh = 0
        while True:
            if pos[0] >= len(buf):
                raise ValueError("varint cut")
            b = buf[pos[0]]; pos[0] += 1
            v |= (b & 0x7F) << sh; sh += 7
            if not b & 0x80:
                return v

    def zz():
        v = varint()
        return (v >> 1) ^ -(v & 1)

    m = (1 << bits) - 1
    half = 1 << (bits - 1)
    block, mpb, total = varint(), varint(), varint()
    if block == 0 or block % 128 or mpb == 0 or block % mpb or (block // mpb) % 32:
        raise ValueError("block geometry")
    vpm = block // mpb
    v = zz() & m
    out = [v] if total else []
    while len(out) < total:
        lo = zz()
        if pos[0] + mpb > len(buf):
            raise ValueError("widths cut")
        widths = buf[pos[0]:pos[0] + mpb]
        pos[0] += mpb
        for j in range(mpb):
            if len(out) >= total:
                break
            bw = widths[j]
            if bw > bits or pos[0] + vpm * bw // 8 > len(buf):
                raise ValueError("miniblock")
            for i in range(vpm):
                if len(out) >= total:
                    break
                d = 0
                for b in range(bw):
                    q = i * bw + b
                    d |= (buf[pos[0] + (q >> 3)] >> (q & 7) & 1) << b
                v = (v + d + lo) & m
                out.append(v)
            pos[0] += vpm * bw // 8
    return [(x ^ half) - half for x in out], pos[0]


# ---- page bodies -----------------------------------------------------------------------------------------------------------
def levels_v1(valid):
    """a v1 page's definition levels: a 4-byte length and the hybrid stream of width 1, runs of equal levels as RLE, the rest bit-packed"""
    runs, i, n = [], 0, len(valid)
    while i < n:
        j = i
        while j < n and valid[j] == valid[i]:
            j += 1
        if j - i >= 8 or j == n:
            runs.append(("rle", j - i, int(valid[i])))
            i = j
        else:
            k = min(n, i + 8 * ((j - i + 7) // 8))        # whole groups: the levels behind the run's end ride along
            runs.append(("bp", [int(x) for x in valid[i:k]]))
            i = k
    s = hybrid(runs, 1)
    return struct.pack("<I", len(s)) + s


def levels_v2_all_present(groups):
    """the definition levels of 8 * groups present values as one bit-packed run: a header varint and `groups` bytes of ones"""
    return uvarint(groups << 1 | 1) + b"\xFF" * groups


# ---- the cases of tests/test_gpu_parquet_pages.py (tests/test_parquet_hand.py checks the same streams against pyarrow) ------------
ELEMENT_CASES = [(total, seed) for total, seeds in ((4096, 6), (40000, 3), (150000, 2)) for seed in range(seeds)]
_streams = {}


def element_stream(codec, total, seed):
    """(the stream, what it inflates to by the plain decoder) — built once per process"""
    key = (codec, total, seed)
    if key not in _streams:
        s = random_snappy(total, 1000 + seed) if codec == C_SNAPPY else random_lz4(total, 2000 + seed)
        _streams[key] = (s, snappy_decode(s) if codec == C_SNAPPY else lz4_decode(s))
    return _streams[key]


def repetitive_int64(n, rng):
    """n values from a few dozen distinct ones, runs among them: a payload in which copies of every length and distance are found"""
    pool = rng.integers(-(1 << 62), 1 << 62, 24)
    v = pool[rng.integers(0, len(pool), n)]
    for _ in range(n // 16):
        at = int(rng.integers(0, n))
        v[at:at + int(rng.integers(2, 12))] = v[at]
    return v.astype("<i8")


PHASE_GROUPS = range(318, 334)   # bit-packed level groups of an all-present v2 page: 2 header bytes + groups = a lead of 320 .. 335, every value of lead & 15
STORED_TAIL = 20000


def phase_page(codec, groups, seed):
    """a v2 optional INT64 page of 8 * groups present values: (lead, stream, values) — the stream is short random elements, then one stored
    literal of 20 000 bytes"""
    rng = np.random.default_rng(seed)
    n = 8 * groups
    values = repetitive_int64(n, rng)
    values[-STORED_TAIL // 8:] = rng.integers(-(1 << 63), (1 << 63) - 1, STORED_TAIL // 8)
    return levels_v2_all_present(groups), encode_payload(values.tobytes(), rng, codec, stored_tail=STORED_TAIL), values


SEAM_POSITIONS = list(range(250, 259)) + list(range(505, 517))


def _sn_seam(P, mis, pre, element):
    """preamble, [a literal of `pre` bytes,] a filler literal whose data ends at window position P - 1 (the compressed page's first byte sits at
    window position `mis`), the elements made by element(output so far), a 9-byte literal and a copy"""
    rng = np.random.default_rng(P * 8 + mis)
    for pl in (1, 2, 3):
        for hdr in (1, 2, 3):
            lead = sn_literal(rng.integers(0, 256, pre, dtype=np.uint8).tobytes()) if pre else b""
            F = P - mis - pl - len(lead) - hdr
            if F < 1:
                continue
            fill = sn_literal(rng.integers(0, 256, F, dtype=np.uint8).tobytes())
            body = lead + fill + element(pre + F)
            out_len = _sn_out_len(body)
            t = 9 + -(out_len + 29) % 8                       # (the page is INT64 values: whole ones)
            tail = sn_literal(b"seam-tail-literal"[:t]) + sn_copy(20, out_len + t, 2)
            s = sn_preamble(out_len + t + 20) + body + tail
            if len(sn_preamble(out_len + t + 20)) == pl and len(fill) - F == hdr:
                return s
    raise AssertionError((P, mis, pre))


def _sn_out_len(elements):
    """output bytes of a string of well-formed snappy elements (no preamble)"""
    p = n = 0
    while p < len(elements):
        tag = elements[p]
        if tag & 3 == 0:
            length = (tag >> 2) + 1
            nb = max(length - 60, 0)
            if nb:
                length = int.from_bytes(elements[p + 1:p + 1 + nb], "little") + 1
            p += 1 + nb + length
        else:
            length = ((tag >> 2) & 7) + 4 if tag & 3 == 1 else (tag >> 2) + 1
            p += (2, 3, 5)[(tag & 3) - 1]
        n += length
    return n


def seam_streams(codec, mis):
    """[(label, stream)]: every element form with its tag at the window positions around the two 256-byte seams, and literals whose last
    byte lands at 510 .. 513, for a compressed page whose first byte sits at window position `mis`"""
    out = []
    if codec == C_SNAPPY:
        forms = [("literal nb=%d" % nb, lambda o, nb=nb: sn_literal(b"LITERAL"[:5 + nb % 3], nb)) for nb in range(5)]
        forms += [("copy kind 1", lambda o: sn_copy(7, 100, 1)), ("copy kind 2", lambda o: sn_copy(33, o, 2)), ("copy kind 3", lambda o: sn_copy(64, 17, 3))]
        for P in SEAM_POSITIONS:
            for name, el in forms:
                out.append(("%s at %d" % (name, P), _sn_seam(P, mis, 0, el)))
        for last in (510, 511, 512, 513):
            for pre in (0, 150):
                out.append(("literal ends at %d after %d" % (last, pre), _sn_seam(last + 1, mis, pre, lambda o: b"")))
        return out
    ext = {0: (5, 8), 1: (20, 24), 3: (530, 535)}              # extension bytes → (a literal length, a match length) that need that many
    for P in SEAM_POSITIONS:
        for kl in (0, 1, 3):
            for km in (0, 1, 3):
                rng = np.random.default_rng(P * 64 + kl * 8 + km * 2 + mis)
                for e in (1, 2, 3):                              # bytes of the filler sequence in front of its literals: the token and its extension
                    F = P - 2 - mis - e
                    first = lz4_seq(rng.integers(0, 256, F, dtype=np.uint8).tobytes(), 1 + (P % 60), 4)
                    if len(first) - F - 2 == e:
                        break
                else:
                    raise AssertionError((P, mis))
                s = first + lz4_seq(rng.integers(0, 256, ext[kl][0], dtype=np.uint8).tobytes(), F, ext[km][1])
                s += lz4_seq(b"twelve bytes and more"[:12 + -(F + 4 + ext[kl][0] + ext[km][1] + 12) % 8])
                out.append(("token ext %d/%d at %d" % (kl, km, P), s))
    for last in (510, 511, 512, 513):                            # a literal whose last byte lands there: token, two extension bytes, the bytes
        rng = np.random.default_rng(last + mis)
        F = last + 1 - mis - 3
        s = lz4_seq(rng.integers(0, 256, F, dtype=np.uint8).tobytes(), 77, 9) + lz4_seq(b"twelve bytes and more"[:12 + -(F + 9 + 12) % 8])
        out.append(("literal ends at %d" % last, s))
    return out


def malformed_streams(codec):
    """[(label, stream, stated size)]: pages of 128 .. 400 bytes that break the format in one place each — every one a clean refusal"""
    rng = np.random.default_rng(5)
    lit = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    N = 140                                                    # output bytes of the well-formed front
    if codec == C_SNAPPY:
        ok = sn_literal(lit[:N])
        cases = [
            ("offset 0", sn_preamble(N + 64) + ok + sn_copy(64, 0, 2), N + 64),
            ("2-byte offset one past the output", sn_preamble(N + 64) + ok + sn_copy(64, N + 1, 2), N + 64),
            ("4-byte offset one past the output", sn_preamble(N + 64) + ok + sn_copy(64, N + 1, 3), N + 64),
            ("1-byte offset one past the output", sn_preamble(N + 11) + ok + sn_copy(11, N + 1, 1), N + 11),
            ("4-byte offset of 2^31", sn_preamble(N + 64) + ok + sn_copy(64, 1 << 31, 3), N + 64),
            ("copy overruns the stated size", sn_preamble(N + 36) + ok + sn_copy(64, 50, 2), N + 36),
            ("literal overruns the stated size", sn_preamble(N + 36) + ok + sn_literal(lit[:100]), N + 36),
            ("stops short of the stated size", sn_preamble(N + 100) + ok + sn_copy(64, 50, 2), N + 100),
            ("wrong preamble", sn_preamble(N + 60) + ok + sn_copy(64, 50, 2), N + 64),
            ("preamble that never ends", b"\xFF" * 6 + ok + sn_copy(64, 50, 2), N + 64),
            ("2-byte copy cut inside its operand", sn_preamble(N + 64) + ok + sn_copy(64, 50, 2)[:2], N + 64),
            ("4-byte copy cut inside its operand", sn_preamble(N + 64) + ok + sn_copy(64, 50, 3)[:3], N + 64),
            ("literal runs past the input", sn_preamble(N + 100) + ok + sn_literal(lit[:100])[:60], N + 100),
            ("literal length bytes cut", sn_preamble(N + 300) + ok + sn_literal(lit, 2)[:2], N + 300),
            ("nb = 4 with FF FF FF FF", sn_preamble(N + 100) + ok + bytes([63 << 2]) + b"\xFF" * 4 + lit[:100], N + 100),
            ("nb = 4 with a length past the input", sn_preamble(N + 100) + ok + bytes([63 << 2]) + struct.pack("<I", 0x7FFFFFFF) + lit[:100], N + 100),
        ]
    else:
        ok = lz4_seq(lit[:N - 30], 50, 30)
        end = lz4_seq(lit[:20])
        cases = [
            ("offset 0", lz4_seq(lit[:N - 30], 0, 30) + end, N + 20),
            ("offset one past the output", lz4_seq(lit[:N - 30], N - 29, 30) + end, N + 20),
            ("match overruns the stated size", ok + lz4_seq(lit[:20], 10, 300) + end, N + 70),
            ("literal overruns the stated size", ok + lz4_seq(lit[:120]), N + 70),
            ("stops short of the stated size", ok + end, N + 70),
            ("literal extension cut off", ok + lz4_seq(lit[:20], 10, 30) + bytes([0xF0, 0xFF]), N + 600),
            ("match extension cut off", ok + lz4_seq(lit[:20], 10, 300)[:-1], N + 340),
            ("offset cut off", ok + lz4_seq(lit[:20], 10, 30)[:-1], N + 70),
            ("literal runs past the input", ok + lz4_seq(lit[:120])[:60], N + 120),
        ]
    for name, st, _ in cases:
        assert 128 <= len(st) <= 400, (name, len(st))
    return cases


NULL_PATTERNS = ("none", "every-third", "random", "runs", "all-but-last")


def valid_mask(pattern, n, rng):
    if pattern == "none":
        return np.ones(n, bool)
    if pattern == "every-third":
        return np.arange(n) % 3 != 0
    if pattern == "random":
        return rng.integers(0, 2, n).astype(bool)
    if pattern == "runs":
        return (np.arange(n) // 37) % 2 == 0
    v = np.zeros(n, bool)
    v[-1] = True
    return v


def optional_v1_body(n, pattern, seed):
    """(valid, values of the present rows, the page's uncompressed body: a 4-byte length, RLE levels, PLAIN values)"""
    rng = np.random.default_rng(seed)
    valid = valid_mask(pattern, n, rng)
    values = repetitive_int64(int(valid.sum()), rng)
    return valid, values, levels_v1(valid) + values.tobytes()


def index_page_pages(codec, n, k):
    """(valid, indices, [a dictionary page of 5 INT64 entries, an optional v1 RLE_DICTIONARY page]) — both bodies cut into short random
    elements: the page's level bytes AND its index-width byte are what the host reads of it"""
    valid = optional_v1_body(n, NULL_PATTERNS[k], n + k)[0]
    rng = np.random.default_rng(n * 8 + k)
    idx = rng.integers(0, 5, int(valid.sum()))
    draw = INDEX_ENTRIES.tobytes()
    ibody = levels_v1(valid) + bytes([3]) + hybrid([("bp", [int(x) for x in idx])], 3)
    return valid, idx, [Page(DICT, 5, E_PLAIN, encode_payload(draw, rng, codec), len(draw)), Page(V1, n, E_RLE_DICTIONARY, encode_payload(ibody, rng, codec), len(ibody))]


INDEX_ENTRIES = np.array([5, -6, 1 << 60, -(1 << 59), 0], "<i8")
STRADDLE_SEEDS = range(6)


def straddle_page(codec, index, seed):
    """An optional v1 page whose stream has ONE COPY that begins in the last byte the host's prefix read wants and runs on into what the
    device inflates: PLAIN values (index False: the prefix ends behind the levels) or dictionary indices of width 1 (index True: behind the
    width byte).  The levels begin with the runs 4 x present, 4 x nil, 4 x present — bytes 08 01 08 00 08 01 — and the byte in front of
    the boundary is 01 (the last run's level, or the index width), so the copy repeats `01 08 00 08 01` from there: legal bytes on both
    sides (as indices of width 1 they are the runs 4 x 0, 4 x 1).  Returns (valid, the present rows' values | indices, stream, body, want).
    A copy cannot straddle the two other prefix ends: the first four bytes are a length below 65536 whose two zero bytes would repeat
    into the first run header, and a stream's first byte is always a literal's."""
    rng = np.random.default_rng(300 + seed * 2 + int(index))
    runs = [("rle", 4, 1), ("rle", 4, 0), ("rle", 4, 1), ("bp", [int(x) for x in rng.integers(0, 2, 8 * int(rng.integers(1, 6)))]),
            ("rle", 8 + int(rng.integers(0, 300)), 0), ("rle", 16 + int(rng.integers(0, 200)), 1)]
    valid = []
    for r in runs:
        valid += [r[2]] * r[1] if r[0] == "rle" else r[1]
    valid = np.array(valid, bool)
    present = int(valid.sum())
    lev = hybrid(runs, 1)
    front = struct.pack("<I", len(lev)) + lev + (b"\x01" if index else b"")
    want = len(front)
    assert front[5:10] == b"\x01\x08\x00\x08\x01" and front[-1] == 1
    if index:
        got = [int(x) for x in rng.integers(0, 2, present - 8)]
        body = front + front[6:10] + hybrid([("bp", got)], 1)
        got = [0] * 4 + [1] * 4 + got
    else:
        raw = bytearray(repetitive_int64(present, rng).tobytes())
        raw[:4] = front[6:10]
        body = front + bytes(raw)
        got = np.frombuffer(bytes(raw), "<i8")
    at, off = want - 1, want - 1 - 5
    assert body[at:at + 5] == body[at - off:at - off + 5]
    if codec == C_SNAPPY:
        stream = sn_preamble(len(body)) + sn_literal(body[:7], seed % 5) + sn_literal(body[7:at]) + sn_copy(5, off, 1 + seed % 3) + sn_literal(body[at + 5:])
    else:
        assert lz4_match_fits(at, 5, len(body))
        stream = lz4_seq(body[:at], off, 5) + lz4_seq(body[at + 5:])
    return valid, got, stream, body, want


def hybrid_pages(bw, ending, codec):
    """(indices, [the dictionary page, the RLE_DICTIONARY page of hybrid_case(bw, ending, 1)]) — stored, or (SNAPPY) cut into short random elements"""
    s, want = hybrid_case(bw, ending, 1)
    top = min(5, 1 << bw)
    body, draw = bytes([bw]) + s, HYBRID_ENTRIES[:top].tobytes()
    if codec == C_NONE:
        return want, [Page(DICT, top, E_PLAIN, draw), Page(V1, len(want), E_RLE_DICTIONARY, body)]
    rng = np.random.default_rng(bw)
    return want, [Page(DICT, top, E_PLAIN, encode_payload(draw, rng, codec), len(draw)), Page(V1, len(want), E_RLE_DICTIONARY, encode_payload(body, rng, codec), len(body))]


HYBRID_ENTRIES = np.array([11, -22, 33, -44, 1 << 61], "<i8")
HYBRID_RLE = (1, 7, 8, 63, 64, 65, 127, 128, 129, 1000, 20000)
HYBRID_GROUPS = (1, 7, 8, 9, 16, 17)


def hybrid_case(bw, ending, seed):
    """(stream, indices): RLE runs and bit-packed runs mixed; ending "padded": a last bit-packed group of which 1..7 values are padding,
    "overshoot": a last RLE run that states more values than the page has left"""
    rng = np.random.default_rng(seed * 64 + bw)
    top = min(5, 1 << bw)                                       # dictionary entries the indices may name
    parts = [("rle", c, int(rng.integers(0, top))) for c in HYBRID_RLE] + [("bp", [int(x) for x in rng.integers(0, top, 8 * g)]) for g in HYBRID_GROUPS]
    runs = [parts[i] for i in rng.permutation(len(parts))]
    want = []
    for r in runs:
        want += [r[2]] * r[1] if r[0] == "rle" else r[1]
    if ending == "padded":
        last = [int(x) for x in rng.integers(0, top, 8 * 3 + 1 + int(rng.integers(0, 7)))]
        runs.append(("bp", last))
        want += last
    else:
        v, c = int(rng.integers(0, top)), 1 + int(rng.integers(0, 300))
        runs.append(("rle", c + 1 + int(rng.integers(0, 5000)), v))
        want += [v] * c
    return hybrid(runs, bw), want


DELTA_GEOMETRIES = ((128, 4), (128, 2), (128, 1), (256, 8), (256, 4), (256, 1), (384, 3), (512, 4), (1024, 4))
DELTA_COUNTS = (1, 2, 33, 65, 129, 130, 257, 700, 1025, 2500)
DELTA_STYLES = ("full", "steps", "const", "edges")


def delta_values(style, n, bits, lengths, rng):
    """full: the whole range (deltas wrap); steps: deltas 0 / 1 (width 1); const (width 0); edges: near the ends of a quarter of the range,
    alternating sign (deltas of nearly all bits).  lengths: small non-negative values — text lengths."""
    if lengths:
        if style == "full":
            return rng.integers(0, 41, n)
        if style == "steps":
            return np.cumsum(rng.integers(0, 64, n) == 0)
        if style == "const":
            return np.full(n, 7)
        v = rng.integers(0, 5, n)
        v[rng.integers(0, n, max(1, n // 50))] = 3000
        return v
    top = 1 << (bits - 1)
    if style == "full":
        return rng.integers(-top, top - 1, n, dtype=np.int64, endpoint=True)
    if style == "steps":
        return int(rng.integers(-1000, 1000)) + np.cumsum(rng.integers(0, 2, n))
    if style == "const":
        return np.full(n, int(rng.integers(-top, top)), dtype=np.int64)
    return (top // 2 + rng.integers(0, 1000, n)) * np.where(np.arange(n) % 2 == 0, 1, -1)


def delta_pages(block, mpb, bits, lengths):
    """[(values, stream)] for every count, style and unused-width byte of one block geometry"""
    rng = np.random.default_rng(block * 16 + mpb + bits + int(lengths))
    out = []
    for n in DELTA_COUNTS:
        for style in DELTA_STYLES:
            for unused in (0, 0xFF):
                v = [int(x) for x in delta_values(style, n, bits, lengths, rng)]
                out.append((v, delta_binary_packed(v, block, mpb, unused, bits)))
    return out


def values_object(stream, usize, codec, kind=V1, pad=0, long=False, body_at=None):
    """one page of usize // 8 INT64 values whose stored body is `stream`: a required column's v1 page, or (kind V2) an optional column's
    v2 page with every value present, its levels one RLE run in front of the compressed part"""
    n = usize // 8
    if kind == V1:
        return hand_object([Page(V1, n, E_PLAIN, stream, usize)], T_INT64, codec, False, pad, long, body_at)
    return hand_object([Page(V2, n, E_PLAIN, stream, usize, 0, hybrid([("rle", n, 1)], 1))], T_INT64, codec, True, pad, long, body_at)


def plain_byte_arrays(values):
    return b"".join(struct.pack("<I", len(v)) + v for v in values)
