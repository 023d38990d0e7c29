"""A plain-Python restatement of the reference's protobuf parser (pkg/parsers/registry/protobuf), for the tests of tfgpu_proto_parser_*.

No third-party imports: the GPU tests must not need google.protobuf.  It holds
  - a small FileDescriptorSet writer, so that tests state schemas as data (fds / file_ / msg / field / map_field),
  - a FileDescriptorSet reader and a wire decoder with protobuf-go's unmarshal rules (proto3 UTF-8, last value wins, oneofs, merges, packed runs),
  - the three scanners (protoseq_scan, repeated framing, single),
  - NewProtoParser's schema logic and makeValues, returning the Go values and the `any` texts json.Marshal makes of them.
Where protobuf-go's behaviour is not pinned by anything the project can read (groups, field numbers above 2^29 - 1, a known field with a foreign wire
type) the decoder raises HostOnly: the device answers TFGPU_ROW_HOST_FALLBACK there and the tests check that code, not a value."""
import base64
import struct

# FieldDescriptorProto.Type
T_DOUBLE, T_FLOAT, T_INT64, T_UINT64, T_INT32, T_FIXED64, T_FIXED32, T_BOOL, T_STRING, T_GROUP, T_MESSAGE, T_BYTES, T_UINT32, T_ENUM, T_SFIXED32, \
    T_SFIXED64, T_SINT32, T_SINT64 = range(1, 19)
TYPE_BY_NAME = {"double": T_DOUBLE, "float": T_FLOAT, "int64": T_INT64, "uint64": T_UINT64, "int32": T_INT32, "fixed64": T_FIXED64, "fixed32": T_FIXED32,
                "bool": T_BOOL, "string": T_STRING, "group": T_GROUP, "message": T_MESSAGE, "bytes": T_BYTES, "uint32": T_UINT32, "enum": T_ENUM,
                "sfixed32": T_SFIXED32, "sfixed64": T_SFIXED64, "sint32": T_SINT32, "sint64": T_SINT64}
LABEL_OPTIONAL, LABEL_REQUIRED, LABEL_REPEATED = 1, 2, 3
WT_OF = {T_DOUBLE: 1, T_FIXED64: 1, T_SFIXED64: 1, T_FLOAT: 5, T_FIXED32: 5, T_SFIXED32: 5, T_STRING: 2, T_BYTES: 2, T_MESSAGE: 2}

PROTOSEQ_MAGIC = bytes([31, 247, 247, 126, 190, 166, 94, 158, 55, 166, 246, 46, 254, 174, 71, 167, 183, 110, 191, 175, 22, 158, 159, 55, 246, 87,
                        247, 102, 167, 6, 175, 247])
PROTOSEQ_MAX_RECORD = 64 * 1024 * 1024


class HostOnly(Exception):
    """what protobuf-go does here is not pinned: the device answers TFGPU_ROW_HOST_FALLBACK"""


class UnmarshalError(Exception):
    pass


class ConfigError(Exception):
    pass


# ---- wire encoding ------------------------------------------------------------------------------------------------------------------------------------
def varint(v: int) -> bytes:
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def zigzag(v: int) -> int:
    return (v << 1) ^ (v >> 63)


def tag(num: int, wt: int) -> bytes:
    return varint(num << 3 | wt)


def enc_varint(num, v):
    return tag(num, 0) + varint(v)


def enc_fixed64(num, raw8: bytes):
    return tag(num, 1) + raw8


def enc_fixed32(num, raw4: bytes):
    return tag(num, 5) + raw4


def enc_bytes(num, b: bytes):
    return tag(num, 2) + varint(len(b)) + bytes(b)


def enc_scalar(num, ftype, v) -> bytes:
    """one occurrence of a scalar field from its Python value"""
    if ftype == T_DOUBLE:
        return enc_fixed64(num, struct.pack("<d", v))
    if ftype == T_FLOAT:
        return enc_fixed32(num, struct.pack("<f", v))
    if ftype in (T_FIXED64, T_SFIXED64):
        return enc_fixed64(num, struct.pack("<Q", v & (1 << 64) - 1))
    if ftype in (T_FIXED32, T_SFIXED32):
        return enc_fixed32(num, struct.pack("<I", v & (1 << 32) - 1))
    if ftype in (T_STRING, T_BYTES):
        return enc_bytes(num, v.encode() if isinstance(v, str) else v)
    if ftype in (T_SINT32, T_SINT64):
        return enc_varint(num, zigzag(v))
    return enc_varint(num, int(v))


def enc_packed(num, ftype, values) -> bytes:
    body = b"".join(enc_scalar(1, ftype, v)[1:] for v in values)  # (the one-byte tag of field 1 cut off)
    return enc_bytes(num, body)


# ---- FileDescriptorSet writer ----------------------------------------------------------------------------------------------------------------------------
def field(name, number, ftype, label=LABEL_OPTIONAL, type_name="", oneof_index=None, proto3_optional=False):
    t = TYPE_BY_NAME[ftype] if isinstance(ftype, str) else ftype
    return dict(name=name, number=number, type=t, label=label, type_name=type_name, oneof_index=oneof_index, proto3_optional=proto3_optional)


def msg(name, fields=(), nested=(), oneofs=(), map_entry=False):
    return dict(name=name, fields=list(fields), nested=list(nested), oneofs=list(oneofs), map_entry=map_entry)


def map_field(owner_full, name, number, key_type, value_type, value_type_name=""):
    """(the field, its synthesized entry message) of `map<key_type, value_type> name = number;` inside the message whose full name is owner_full"""
    entry = "".join(p.capitalize() if i else p[:1].upper() + p[1:] for i, p in enumerate(name.split("_"))) + "Entry"
    e = msg(entry, [field("key", 1, key_type), field("value", 2, value_type, type_name=value_type_name)], map_entry=True)
    return field(name, number, "message", LABEL_REPEATED, "." + owner_full + "." + entry), e


def file_(name, package="", syntax="proto3", messages=(), enums=()):
    return dict(name=name, package=package, syntax=syntax, messages=list(messages), enums=list(enums))


def _w_field(f):
    out = enc_bytes(1, f["name"].encode()) + enc_varint(3, f["number"]) + enc_varint(4, f["label"]) + enc_varint(5, f["type"])
    if f["type_name"]:
        out += enc_bytes(6, f["type_name"].encode())
    if f["oneof_index"] is not None:
        out += enc_varint(9, f["oneof_index"])
    if f["proto3_optional"]:
        out += enc_varint(17, 1)
    return out


def _w_msg(m):
    out = enc_bytes(1, m["name"].encode())
    for f in m["fields"]:
        out += enc_bytes(2, _w_field(f))
    for n in m["nested"]:
        out += enc_bytes(3, _w_msg(n))
    if m["map_entry"]:
        out += enc_bytes(7, enc_varint(7, 1))
    for o in m["oneofs"]:
        out += enc_bytes(8, enc_bytes(1, o.encode()))
    return out


def fds(files) -> bytes:
    out = b""
    for f in files:
        body = enc_bytes(1, f["name"].encode())
        if f["package"]:
            body += enc_bytes(2, f["package"].encode())
        for m in f["messages"]:
            body += enc_bytes(4, _w_msg(m))
        for e in f["enums"]:
            body += enc_bytes(5, enc_bytes(1, e.encode()) + enc_bytes(2, enc_bytes(1, (e + "_ZERO").encode()) + enc_varint(2, 0)))
        if f["syntax"] != "proto2":
            body += enc_bytes(12, f["syntax"].encode())
        out += enc_bytes(1, body)
    return out


# ---- wire decoding ---------------------------------------------------------------------------------------------------------------------------------------
def read_varint(b, i, end):
    x = 0
    for s in range(0, 70, 7):
        if i >= end:
            raise UnmarshalError("truncated varint")
        c = b[i]
        i += 1
        x |= (c & 0x7F) << s
        if not c & 0x80:
            return x & (1 << 64) - 1, i
    raise UnmarshalError("varint overflow")


def wire_fields(b, a=0, z=None, strict=True):
    """[(number, wire type, value | (start, len))] of b[a:z].  strict: HostOnly for what the device leaves to the host"""
    z = len(b) if z is None else z
    i = a
    out = []
    while i < z:
        t, i = read_varint(b, i, z)
        wt, num = t & 7, t >> 3
        if num == 0 or num > (1 << 29) - 1:
            if strict:
                raise HostOnly("field number %d" % num)
            raise UnmarshalError("invalid field number")
        if wt == 0:
            v, i = read_varint(b, i, z)
        elif wt == 1:
            if z - i < 8:
                raise UnmarshalError("truncated fixed64")
            v, i = int.from_bytes(b[i:i + 8], "little"), i + 8
        elif wt == 5:
            if z - i < 4:
                raise UnmarshalError("truncated fixed32")
            v, i = int.from_bytes(b[i:i + 4], "little"), i + 4
        elif wt == 2:
            n, i = read_varint(b, i, z)
            if n > z - i:
                raise UnmarshalError("truncated bytes")
            v, i = (i, n), i + n
        else:
            raise HostOnly("wire type %d" % wt)
        out.append((num, wt, v))
    return out


# ---- descriptors ---------------------------------------------------------------------------------------------------------------------------------------------
class FieldDesc:
    def __init__(self, name, number, ftype, label, type_name, oneof_index, proto3_optional, proto3):
        self.name, self.number, self.type, self.label, self.type_name = name, number, ftype, label, type_name
        self.proto3_optional, self.proto3 = proto3_optional, proto3
        self.oneof = None if oneof_index is None or proto3_optional else oneof_index
        self.message = None  # MessageDesc of a message-typed field

    @property
    def is_map(self):
        return self.label == LABEL_REPEATED and self.type == T_MESSAGE and self.message.map_entry

    @property
    def is_list(self):
        return self.label == LABEL_REPEATED and not self.is_map

    @property
    def has_presence(self):  # protoreflect.FieldDescriptor.HasPresence
        if self.label == LABEL_REPEATED:
            return False
        return self.type in (T_MESSAGE, T_GROUP) or self.proto3_optional or self.oneof is not None or not self.proto3


class MessageDesc:
    def __init__(self, name, full, proto3, file_name):
        self.name, self.full, self.proto3, self.file_name = name, full, proto3, file_name
        self.fields, self.map_entry = [], False

    def by_name(self, n):
        for f in self.fields:
            if f.name == n:
                return f
        return None

    def by_number(self, n):
        for f in self.fields:
            if f.number == n:
                return f
        return None


class Pool:
    def __init__(self):
        self.files, self.by_full = [], {}  # files: [(name, [top-level MessageDesc])]


def _s(b, v):
    return bytes(b[v[0]:v[0] + v[1]]).decode()


def _read_msg(b, a, z, scope, proto3, file_name, pool):
    fs = wire_fields(b, a, z, strict=False)
    name = next(_s(b, v) for n, w, v in fs if n == 1 and w == 2)
    m = MessageDesc(name, scope + "." + name if scope else name, proto3, file_name)
    pool.by_full["." + m.full] = m
    for n, w, v in fs:
        if n == 2 and w == 2:
            d = dict(name="", number=0, label=1, type=0, type_name="", oneof_index=None, p3o=False)
            for n2, w2, v2 in wire_fields(b, v[0], v[0] + v[1], strict=False):
                if n2 == 1:
                    d["name"] = _s(b, v2)
                elif n2 == 3:
                    d["number"] = v2
                elif n2 == 4:
                    d["label"] = v2
                elif n2 == 5:
                    d["type"] = v2
                elif n2 == 6:
                    d["type_name"] = _s(b, v2)
                elif n2 == 9:
                    d["oneof_index"] = v2
                elif n2 == 17:
                    d["p3o"] = bool(v2)
            m.fields.append(FieldDesc(d["name"], d["number"], d["type"], d["label"], d["type_name"], d["oneof_index"], d["p3o"], proto3))
        elif n == 3 and w == 2:
            _read_msg(b, v[0], v[0] + v[1], m.full, proto3, file_name, pool)
        elif n == 7 and w == 2:
            for n2, w2, v2 in wire_fields(b, v[0], v[0] + v[1], strict=False):
                if n2 == 7:
                    m.map_entry = bool(v2)
    return m


def parse_fds(data: bytes) -> Pool:
    pool = Pool()
    for n, w, v in wire_fields(data, strict=False):
        if n != 1 or w != 2:
            continue
        fs = wire_fields(data, v[0], v[0] + v[1], strict=False)
        name = next((_s(data, x) for k, w2, x in fs if k == 1 and w2 == 2), "")
        package = next((_s(data, x) for k, w2, x in fs if k == 2 and w2 == 2), "")
        syntax = next((_s(data, x) for k, w2, x in fs if k == 12 and w2 == 2), "proto2")
        tops = [_read_msg(data, x[0], x[0] + x[1], package, syntax == "proto3", name, pool) for k, w2, x in fs if k == 4 and w2 == 2]
        pool.files.append((name, tops))
    for m in pool.by_full.values():
        for f in m.fields:
            if f.type in (T_MESSAGE, T_GROUP):
                if f.type_name not in pool.by_full:
                    raise ConfigError("could not resolve type " + f.type_name)
                f.message = pool.by_full[f.type_name]
    return pool


def extract_message_desc(pool: Pool, name: str):
    """extractMessageDesc: a top-level message by its short name.  (the files that define it, the first one's descriptor)"""
    hits = [(fn, m) for fn, tops in pool.files for m in tops if m.name == name]
    if not hits:
        raise ConfigError("error extracting message descriptor from desc file: message with provided name '%s' not found" % name)
    return hits[0][1], [fn for fn, _ in hits]


def extract_embedded_repeated(m: MessageDesc):
    if len(m.fields) == 1 and m.fields[0].is_list and m.fields[0].type == T_MESSAGE:
        return m.fields[0].message
    return None


# ---- the dynamic message ------------------------------------------------------------------------------------------------------------------------------------
class NilBytes(bytes):
    """a nil []byte: what Get returns for an unset bytes field.  json.Marshal writes null for it; as a column cell it is an empty, non-nil value
    (the interface holds a typed nil)"""


NIL_BYTES = NilBytes()


class Msg:
    """dynamicpb.Message after proto.Unmarshal: values[number] for the populated fields (a scalar, bytes, list, dict or Msg)"""

    def __init__(self, desc):
        self.desc, self.values = desc, {}

    def has(self, f: FieldDesc) -> bool:
        if f.number not in self.values:
            return False
        v = self.values[f.number]
        if f.label == LABEL_REPEATED:
            return len(v) > 0
        if f.has_presence:
            return True
        if f.type in (T_STRING, T_BYTES):
            return len(v) > 0
        if f.type in (T_FLOAT, T_DOUBLE) and v == 0 and struct.pack("<d", v)[7] & 0x80:
            raise HostOnly("Has() of -0.0")
        return bool(v)

    def get(self, f: FieldDesc):
        if f.number in self.values:
            return self.values[f.number]
        if f.is_map:
            return {}
        if f.label == LABEL_REPEATED:
            return []
        if f.type == T_MESSAGE:
            return Msg(f.message)
        return {T_STRING: "", T_BYTES: NIL_BYTES, T_BOOL: False, T_FLOAT: 0.0, T_DOUBLE: 0.0}.get(f.type, 0)


def _scalar(f: FieldDesc, wt, v, b):
    t = f.type
    if wt != WT_OF.get(t, 0):
        raise HostOnly("field %s arrives with wire type %d" % (f.name, wt))
    if t == T_DOUBLE:
        return struct.unpack("<d", v.to_bytes(8, "little"))[0]
    if t == T_FLOAT:
        return struct.unpack("<f", v.to_bytes(4, "little"))[0]
    if t in (T_INT32, T_ENUM, T_SFIXED32):
        v &= 0xFFFFFFFF
        return v - (1 << 32) if v >> 31 else v
    if t in (T_INT64, T_SFIXED64):
        return v - (1 << 64) if v >> 63 else v
    if t in (T_UINT32, T_FIXED32):
        return v & 0xFFFFFFFF
    if t == T_SINT32:
        v &= 0xFFFFFFFF
        return (v >> 1) ^ -(v & 1)
    if t == T_SINT64:
        return (v >> 1) ^ -(v & 1)
    if t == T_BOOL:
        return v != 0
    if t == T_STRING:
        raw = bytes(b[v[0]:v[0] + v[1]])
        if f.proto3:
            try:
                return raw.decode("utf-8")
            except UnicodeDecodeError:
                raise UnmarshalError("string field contains invalid UTF-8")
        return raw.decode("utf-8", "surrogateescape")
    if t == T_BYTES:
        return bytes(b[v[0]:v[0] + v[1]])
    return v  # uint64, fixed64


def _packed(f: FieldDesc, b, a, n):
    out, i, z = [], a, a + n
    w = WT_OF.get(f.type, 0)
    while i < z:
        if w == 0:
            v, i = read_varint(b, i, z)
        else:
            k = 8 if w == 1 else 4
            if z - i < k:
                raise UnmarshalError("truncated packed run")
            v, i = int.from_bytes(b[i:i + k], "little"), i + k
        out.append(_scalar(f, w, v, b))
    return out


def unmarshal(desc: MessageDesc, b, a=0, z=None, into=None) -> Msg:
    m = into if into is not None else Msg(desc)
    for num, wt, v in wire_fields(b, a, len(b) if z is None else z):
        f = desc.by_number(num)
        if f is None:
            continue  # an unknown field
        if f.type == T_GROUP:
            raise HostOnly("group")
        if f.oneof is not None:
            for g in desc.fields:
                if g is not f and g.oneof == f.oneof:
                    m.values.pop(g.number, None)
        if f.is_map:
            if wt != 2:
                raise HostOnly("map field with wire type %d" % wt)
            kf, vf = f.message.by_number(1), f.message.by_number(2)
            key = {T_STRING: "", T_BOOL: False}.get(kf.type, 0)
            val, have = None, False
            for n2, w2, v2 in wire_fields(b, v[0], v[0] + v[1]):
                if n2 == 1:
                    key = _scalar(kf, w2, v2, b)
                elif n2 == 2:
                    if vf.type == T_MESSAGE:
                        if w2 != 2:
                            raise HostOnly("wire type")
                        val = unmarshal(vf.message, b, v2[0], v2[0] + v2[1], val if have else None)
                    else:
                        val = _scalar(vf, w2, v2, b)
                    have = True
            if not have:
                val = Msg(vf.message) if vf.type == T_MESSAGE else Msg(f.message).get(vf)
            d = m.values.setdefault(num, {})
            d.pop(key, None)
            d[key] = val
        elif f.label == LABEL_REPEATED:
            lst = m.values.setdefault(num, [])
            if f.type == T_MESSAGE:
                if wt != 2:
                    raise HostOnly("wire type")
                lst.append(unmarshal(f.message, b, v[0], v[0] + v[1]))
            elif wt == 2 and WT_OF.get(f.type, 0) != 2:
                lst.extend(_packed(f, b, v[0], v[1]))
            else:
                lst.append(_scalar(f, wt, v, b))
        elif f.type == T_MESSAGE:
            if wt != 2:
                raise HostOnly("wire type")
            m.values[num] = unmarshal(f.message, b, v[0], v[0] + v[1], m.values.get(num))  # occurrences merge
        else:
            m.values[num] = _scalar(f, wt, v, b)
    return m


# ---- scanners --------------------------------------------------------------------------------------------------------------------------------------------------
def protoseq_scan(data: bytes):
    """ProtoseqScanner: [(start, len, error text | None)] — the event's bytes are data[start:start + len] (the failing forms included: the
    incomplete frame's data is the size field plus the rest, which is contiguous in the message)"""
    out, pos, z = [], 0, len(data)
    while pos < z:
        if z - pos < 4:
            out.append((pos, z - pos, "last incomplete protoseq message: expected size len = 4, got size len = %d" % (z - pos)))
            break
        size = int.from_bytes(data[pos:pos + 4], "little")
        pos += 4
        if size <= PROTOSEQ_MAX_RECORD:
            if z - pos < size + 32:
                out.append((pos - 4, z - pos + 4, "last incomplete protoseq message"))
                break
            if data[pos + size:pos + size + 32] == PROTOSEQ_MAGIC:
                out.append((pos, size, None))
                pos += size + 32
                continue
        q = data.find(PROTOSEQ_MAGIC, pos)
        if q < 0:
            break  # "can't find any magic sequence entry": do never reads sc.Err(), the rest is dropped
        out.append((pos, q - pos, "frame corrupted"))
        pos = q + 32
    return out


def protoseq_frame(payload: bytes) -> bytes:
    return len(payload).to_bytes(4, "little") + payload + PROTOSEQ_MAGIC


# ---- json.Marshal of the Go values ------------------------------------------------------------------------------------------------------------------------------
class F32(float):
    """a Go float32 (json.Marshal formats it by the 32-bit rule)"""


def _shortest(x: float, bits: int):
    """(digits, decimal exponent of the first digit) of the shortest decimal that reads back as x"""
    for p in range(0, 17):
        s = "%.*e" % (p, x)
        back = struct.unpack("<f", struct.pack("<f", float(s)))[0] if bits == 32 else float(s)
        if back == x:
            mant, exp = s.split("e")
            return mant.replace(".", "").rstrip("0") or "0", int(exp)
    raise AssertionError(x)


def go_json_float(x: float, bits: int = 64) -> str:
    if x != x or x in (float("inf"), float("-inf")):
        raise HostOnly("json: unsupported value")
    if x == 0:
        return "-0" if struct.pack("<d", x)[7] & 0x80 else "0"
    neg, ax = x < 0, abs(x)
    digits, exp = _shortest(ax, bits)
    if ax < 1e-6 or ax >= 1e21:
        s = digits[0] + ("." + digits[1:] if len(digits) > 1 else "") + "e" + ("-" if exp < 0 else "+") + ("%02d" % abs(exp))
        if len(s) >= 4 and s[-4] == "e" and s[-3] == "-" and s[-2] == "0":
            s = s[:-2] + s[-1]
    elif exp < 0:
        s = "0." + "0" * (-exp - 1) + digits
    elif len(digits) <= exp + 1:
        s = digits + "0" * (exp + 1 - len(digits))
    else:
        s = digits[:exp + 1] + "." + digits[exp + 1:]
    return ("-" if neg else "") + s


def go_json_string(s: str, html=False) -> str:
    """encoding/json's string; html: with escapeHTML on (json.Marshal's default).  An `any` column's text is the form with SetEscapeHTML(false): the ABI's
    definition of TFGPU_R_JSON"""
    out = ['"']
    for ch in s:
        c = ord(ch)
        if ch == '"':
            out.append('\\"')
        elif ch == "\\":
            out.append("\\\\")
        elif ch == "\n":
            out.append("\\n")
        elif ch == "\r":
            out.append("\\r")
        elif ch == "\t":
            out.append("\\t")
        elif ch == "\b":
            out.append("\\b")
        elif ch == "\f":
            out.append("\\f")
        elif c < 0x20 or (html and ch in "<>&") or c in (0x2028, 0x2029):
            out.append("\\u%04x" % c)
        else:
            out.append(ch)
    out.append('"')
    return "".join(out)


def go_json(v, html=False) -> str:
    """json.Marshal(v); html: with escapeHTML on (ChangeItem.ToJSONString), off for the text of an `any` column"""
    if v is None or isinstance(v, NilBytes):
        return "null"
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, F32):
        return go_json_float(float(v), 32)
    if isinstance(v, float):
        return go_json_float(v, 64)
    if isinstance(v, int):
        return str(v)
    if isinstance(v, str):
        return go_json_string(v, html)
    if isinstance(v, (bytes, bytearray)):
        return '"' + base64.b64encode(bytes(v)).decode() + '"'
    if isinstance(v, list):
        return "[" + ",".join(go_json(x, html) for x in v) + "]"
    if isinstance(v, dict):
        return "{" + ",".join(go_json_string(k, html) + ":" + go_json(v[k], html) for k in sorted(v, key=lambda k: k.encode())) + "}"
    raise TypeError(type(v))


# ---- NewProtoParser / makeValues ----------------------------------------------------------------------------------------------------------------------------------
def yt_type(f: FieldDesc) -> str:
    if f.label == LABEL_REPEATED:
        return "any"
    return {T_BOOL: "boolean", T_INT32: "int32", T_SINT32: "int32", T_SFIXED32: "int32", T_ENUM: "int32", T_INT64: "int64", T_SINT64: "int64",
            T_SFIXED64: "int64", T_UINT32: "uint32", T_FIXED32: "uint32", T_UINT64: "uint64", T_FIXED64: "uint64", T_FLOAT: "float",
            T_DOUBLE: "double", T_STRING: "utf8", T_BYTES: "string"}.get(f.type, "any")


def _fmt_sprint(k):
    if isinstance(k, bool):
        return "true" if k else "false"
    return str(k)


def extract_value(f: FieldDesc, val, nfe: bool, as_list=True):
    """extractValueRecursive: the Go value as Python (F32 for float32, bytes / None for []byte, dict / list for `any`)"""
    if as_list and f.is_list:
        return [extract_value(f, x, nfe, False) for x in val]  # (a nil element stays nil in its slot either way)
    if f.type == T_MESSAGE and not f.is_map:
        items, empty = {}, 0
        for g in val.desc.fields:
            if nfe and not val.has(g):
                empty += 1
                continue
            items[g.name] = extract_value(g, val.get(g), nfe)
        return None if empty == len(val.desc.fields) else items
    if f.is_map:
        kf, vf = f.message.by_number(1), f.message.by_number(2)
        items = {}
        for k, v in val.items():
            vv = extract_value(vf, v, nfe)
            if vv is not None:  # (a nil []byte is a typed nil inside the interface: it stays, NIL_BYTES is not None)
                items[_fmt_sprint(extract_value(kf, k, nfe))] = vv
        return items
    if f.type == T_FLOAT:
        return F32(val)
    return val


def go_cell(f: FieldDesc, v):
    """[gotype, value] of one column value, the form Column.pyvalue gives after a download: `any` values as their json.Marshal text"""
    if v is None:
        return ["nil", None]
    if f.label == LABEL_REPEATED or f.type == T_MESSAGE:
        return ["json", go_json(v).encode()]
    if f.type == T_STRING:
        return ["string", v.encode("utf-8", "surrogateescape")]
    if f.type == T_BYTES:
        return ["bytes", bytes(v)]
    if f.type == T_BOOL:
        return ["bool", bool(v)]
    if f.type == T_FLOAT:
        return ["float32", float(v)]
    if f.type == T_DOUBLE:
        return ["float64", float(v)]
    return [yt_type(f), int(v)]


def encode(desc: MessageDesc, items, packed=True) -> bytes:
    """a message of `desc` from [(field name, value)] in the order given: a list for a repeated field (one packed run for the packable kinds unless
    packed is False), a dict for a map, [(name, value)] for a message; ("#raw", bytes) splices bytes in as they are"""
    out = b""
    for name, v in items:
        if name == "#raw":
            out += v
            continue
        f = desc.by_name(name)
        if f.is_map:
            kf, vf = f.message.by_number(1), f.message.by_number(2)
            for k, x in v.items():
                out += enc_bytes(f.number, enc_scalar(1, kf.type, k) + (enc_bytes(2, encode(vf.message, x)) if vf.type == T_MESSAGE else enc_scalar(2, vf.type, x)))
        elif f.label == LABEL_REPEATED:
            if f.type == T_MESSAGE:
                for x in v:
                    out += enc_bytes(f.number, encode(f.message, x, packed))
            elif packed and WT_OF.get(f.type, 0) != 2:
                out += enc_packed(f.number, f.type, v)
            else:
                for x in v:
                    out += enc_scalar(f.number, f.type, x)
        elif f.type == T_MESSAGE:
            out += enc_bytes(f.number, encode(f.message, v, packed))
        else:
            out += enc_scalar(f.number, f.type, v)
    return out


class Parser:
    """protoparser.ProtoParser built by ToProtoParserConfig + NewProtoParser.  schema: [(name, DataType, key, required)]"""

    def __init__(self, desc_file: bytes, message_name: str, package_type="PackageTypeSingleMsg", include_columns=(), primary_keys=(), null_keys_allowed=False,
                 add_system_columns=False, skip_dedup_keys=False, add_synthetic_keys=False, not_fill_empty_fields=False):
        if not desc_file:
            raise ConfigError("desc file and desc resource are both empty")
        self.pkg, self.nfe = package_type, not_fill_empty_fields
        pool = parse_fds(desc_file)
        try:
            root, self.defined_in = extract_message_desc(pool, message_name)
        except ConfigError as e:
            raise ConfigError("SetDescriptors error: " + str(e))
        self.wrapper = root
        self.desc = root
        if package_type == "PackageTypeRepeated":
            el = extract_embedded_repeated(root)
            if el is None:
                raise ConfigError("SetDescriptors error: can't extract embedded repeated message descriptor while provided package type is repeated")
            self.desc = el
        d = self.desc
        params = {}
        for name, req in include_columns:
            if name in params:
                raise ConfigError("duplicate column name '%s'" % name)
            params[name] = req
        schema, self.included, self.extra = [], [], []
        keys = set()
        for k in primary_keys:
            keys.add(k)
            f = d.by_name(k)
            if f is None:
                raise ConfigError("given key field '%s' not found in proto message desc" % k)
            req = not null_keys_allowed
            if k in params:
                if not null_keys_allowed and not params[k]:
                    raise ConfigError("key param '%s' must be set as required" % k)
                req = params[k]
            schema.append((k, yt_type(f), True, req))
            self.included.append((f, req))
        if not include_columns:
            for f in d.fields:
                if f.name not in keys:
                    schema.append((f.name, yt_type(f), False, False))
                    self.included.append((f, False))
        else:
            for name, req in include_columns:
                f = d.by_name(name)
                if f is None:
                    raise ConfigError("requested column %s not found in proto descriptor" % name)
                if name in keys:
                    continue
                schema.append((name, yt_type(f), False, bool(req)))
                self.included.append((f, bool(req)))
        if add_system_columns:
            have = {s[0] for s in schema}
            for f in d.fields:
                if f.name not in have:
                    schema.append(("_lb_extra_" + f.name, yt_type(f), False, False))
                    self.extra.append(f)
        self.aux = []
        if add_synthetic_keys:
            self.aux += [("_partition", "utf8", True), ("_offset", "uint64", True), ("_idx", "uint64", True)]
        if add_system_columns:
            self.aux += [("_lb_ctime", "datetime", not skip_dedup_keys), ("_lb_wtime", "datetime", not skip_dedup_keys)]
        for name, t, key in self.aux:
            schema.append((name, t, key, key and not null_keys_allowed))
        self.schema = schema

    # makeValues: the column values of one unmarshalled event, or the error text
    def make_values(self, m: Msg):
        res = []
        for f, req in self.included:
            if req and f.has_presence and not m.has(f):
                return None, "required field '%s' was not populated" % f.name, f.name
            if self.nfe and not m.has(f):
                res.append(None)
                continue
            res.append(extract_value(f, m.get(f), self.nfe))
        for f in self.extra:
            res.append(extract_value(f, m.get(f), self.nfe))
        return res, None, None

    def events(self, value: bytes):
        """the scanner over one queue message: [(start, len, counter, error | None)], or ("wrapper", text) when the repeated wrapper fails"""
        if self.pkg == "PackageTypeSingleMsg":
            return [(0, len(value), 1, None)] if value else []
        if self.pkg == "PackageTypeProtoseq":
            return [(s, n, i + 1, err) for i, (s, n, err) in enumerate(protoseq_scan(value))]
        fnum = self.wrapper.fields[0].number
        out = []
        for num, wt, v in wire_fields(value):
            if num != fnum:
                continue
            if wt != 2:
                raise HostOnly("the wrapper's field with wire type %d" % wt)
            out.append((v[0], v[1], len(out) + 1, None))
        return out

    def do_batch(self, values):
        """ProtoParser.DoBatch over the messages' values → (rows, unparsed, event_base).
        rows: [(event, msg, counter, [go_cell per field column])]; unparsed: [(event, msg, idx, kind, column name | None, start, len)] with kind one of
        'unmarshal', 'required', 'corrupted', 'incomplete', 'short', 'wrapper', 'host' and start relative to the message's own value"""
        rows, unparsed, base, ev = [], [], [0], 0
        rep = self.pkg == "PackageTypeRepeated"
        for mi, value in enumerate(values):
            whole = None  # repeated: the message as ONE event — "wrapper": it (an element of it) does not unmarshal, counter 1; "host": not pinned
            evs, msgs = [], []
            try:
                evs = self.events(value)
            except UnmarshalError:
                whole = "wrapper"
            except HostOnly:
                whole = "host"
            for s, n, idx, err in evs:
                if err is not None:
                    msgs.append(None)
                    continue
                try:
                    msgs.append(unmarshal(self.desc, value, s, s + n))
                except (UnmarshalError, HostOnly) as e:
                    msgs.append(e)
            if rep and any(isinstance(m, UnmarshalError) for m in msgs):
                whole = "wrapper"
            elif rep and whole is None and any(isinstance(m, HostOnly) for m in msgs):
                whole = "host"
            if whole is not None:
                unparsed.append((ev, mi, 1 if whole == "wrapper" else 0, whole, None, 0, len(value)))
                ev += 1
                base.append(ev)
                continue
            for (s, n, idx, err), m in zip(evs, msgs):
                e = ev + idx - 1
                if err is not None:
                    kind = "corrupted" if err == "frame corrupted" else "incomplete" if err == "last incomplete protoseq message" else "short"
                    unparsed.append((e, mi, idx, kind, None, s, n))
                elif isinstance(m, UnmarshalError):
                    unparsed.append((e, mi, idx, "unmarshal", None, s, n))
                elif isinstance(m, HostOnly):
                    unparsed.append((e, mi, idx, "host", None, s, n))
                else:
                    try:
                        vals, text, col = self.make_values(m)
                        if vals is not None:
                            vals = [go_cell(f, v) for f, v in zip([x for x, _ in self.included] + self.extra, vals)]
                    except HostOnly:
                        unparsed.append((e, mi, idx, "host", None, s, n))
                        continue
                    if text is not None:
                        unparsed.append((e, mi, idx, "required", col, s, n))
                    else:
                        rows.append((e, mi, idx, vals))
            ev += len(evs)
            base.append(ev)
        return rows, unparsed, base


# ---- schemas the tests share, stated as data -----------------------------------------------------------------------------------------------------------------------
def struct_file():
    """google/protobuf/struct.proto"""
    fields_f, fields_e = map_field("google.protobuf.Struct", "fields", 1, "string", "message", ".google.protobuf.Value")
    value = msg("Value", [field("null_value", 1, "enum", type_name=".google.protobuf.NullValue", oneof_index=0), field("number_value", 2, "double", oneof_index=0),
                          field("string_value", 3, "string", oneof_index=0), field("bool_value", 4, "bool", oneof_index=0),
                          field("struct_value", 5, "message", type_name=".google.protobuf.Struct", oneof_index=0),
                          field("list_value", 6, "message", type_name=".google.protobuf.ListValue", oneof_index=0)], oneofs=["kind"])
    lst = msg("ListValue", [field("values", 1, "message", LABEL_REPEATED, ".google.protobuf.Value")])
    return file_("google/protobuf/struct.proto", "google.protobuf", messages=[msg("Struct", [fields_f], nested=[fields_e]), value, lst], enums=["NullValue"])


SCALARS = ["double", "float", "int32", "int64", "uint32", "uint64", "sint32", "sint64", "fixed32", "fixed64", "sfixed32", "sfixed64", "bool", "string", "bytes"]


def std_data_types_fds() -> bytes:
    """the reference's gotest/prototest/std_data_types.proto (StdDataTypesMsg, EmbeddedMsg, OneOfs) with its import"""
    mf, me = map_field("StdDataTypesMsg", "mapField", 16, "string", "int32")
    std = msg("StdDataTypesMsg", [field(t + "Field", i + 1, t) for i, t in enumerate(SCALARS)] + [
        mf, field("repeatedField", 17, "string", LABEL_REPEATED), field("msgField", 18, "message", type_name=".EmbeddedMsg"),
        field("structField", 19, "message", type_name=".google.protobuf.Struct", oneof_index=0, proto3_optional=True),
        field("one", 20, "message", type_name=".OneOfs")], nested=[me], oneofs=["_structField"])
    emb = msg("EmbeddedMsg", [field("stringField", 1, "string"), field("int32Field", 2, "int32"), field("enumField", 3, "enum", type_name=".EmbeddedEnum")])
    one = msg("OneOfs", [field(t + "Field", i + 1, t, oneof_index=0) for i, t in enumerate(SCALARS)] + [
        field("msgField", 16, "message", type_name=".EmbeddedMsg", oneof_index=0),
        field("structField", 17, "message", type_name=".google.protobuf.Struct", oneof_index=0)], oneofs=["one"])
    lst = msg("StdDataTypesMsgList", [field("items", 1, "message", LABEL_REPEATED, ".StdDataTypesMsg")])
    return fds([struct_file(), file_("std_data_types.proto", messages=[lst, std, emb, one], enums=["EmbeddedEnum"])])


def device_cases_fds(foreign=True) -> bytes:
    """the message the device tests decode: every scalar kind, optional and oneof members, lists, one-level messages, maps — and two fields outside
    the device subset's ordinary shapes: `deep` (nesting of two levels; left out with foreign=False) and `big` (a field number above the lookup table)"""
    inner = msg("Inner", [field("s", 1, "string"), field("i", 2, "int32"), field("e", 3, "enum", type_name=".t.E"), field("f", 4, "float"), field("b", 5, "bytes"),
                          field("oi", 6, "int32", oneof_index=0, proto3_optional=True)], oneofs=["_oi"])
    maps = [map_field("t.Ev", n, k, "string", v) for n, k, v in (("mi", 30, "int32"), ("ms", 31, "string"), ("mf", 34, "float"), ("mb", 35, "bytes"))]
    ev = msg("Ev", [field(n, i + 1, t) for i, (n, t) in enumerate(zip(
        ["d", "f", "i32", "i64", "u32", "u64", "s32", "s64", "fx32", "fx64", "sf32", "sf64", "b", "s", "by"], SCALARS))] + [
        field("en", 16, "enum", type_name=".t.E"),
        field("oi", 17, "int32", oneof_index=1, proto3_optional=True), field("os", 18, "string", oneof_index=2, proto3_optional=True),
        field("ua", 19, "int32", oneof_index=0), field("ub", 20, "string", oneof_index=0),
        field("ri", 21, "int32", LABEL_REPEATED), field("rs", 22, "string", LABEL_REPEATED), field("rb", 23, "bytes", LABEL_REPEATED),
        field("rf", 24, "float", LABEL_REPEATED), field("re", 25, "enum", LABEL_REPEATED, ".t.E"), field("rz", 26, "sint64", LABEL_REPEATED),
        field("rx", 27, "fixed64", LABEL_REPEATED), field("m", 28, "message", type_name=".t.Inner"),
        field("rm", 29, "message", LABEL_REPEATED, ".t.Inner"), maps[0][0], maps[1][0], field("em", 32, "message", type_name=".t.Empty"),
        field("rem", 33, "message", LABEL_REPEATED, ".t.Empty"), maps[2][0], maps[3][0],
        field("big", 2000, "int32"), field("rd", 41, "double", LABEL_REPEATED)] + ([field("deep", 40, "message", type_name=".t.Deep")] if foreign else []),
        nested=[m[1] for m in maps], oneofs=["u", "_oi", "_os"])
    deep = msg("Deep", [field("in", 1, "message", type_name=".t.Inner")])
    lst = msg("EvList", [field("items", 1, "message", LABEL_REPEATED, ".t.Ev")])
    return fds([file_("t.proto", "t", messages=[inner, msg("Empty"), ev, deep, lst], enums=["E"])])


DEVICE_COLUMNS = ["d", "f", "i32", "i64", "u32", "u64", "s32", "s64", "fx32", "fx64", "sf32", "sf64", "b", "s", "by", "en", "oi", "os", "ua", "ub", "ri", "rs", "rb",
                  "rf", "re", "rz", "rx", "m", "rm", "mi", "ms", "em", "rem", "mf", "mb", "big", "rd"]  # every field of t.Ev but `deep`
