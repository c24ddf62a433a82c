"""Builders for datanode packet streams (test infrastructure).

Wire formats (src/datanode.c:2345-2418, big-endian integers per
src/heapbuf.c:174-215):
  v1: [plen s32][offsetInBlock s64][seqno s64][lastPacketInBlock s8][dataLen s32]
  v2: [plen s32][hlen u16][PacketHeaderProto]
followed by plen - dataLen - 4 bytes of BE chunk CRCs and the data.

header_v2() emits the canonical encoding of PacketHeaderProto
(src/proto/datatransfer.proto:228-235): fields in number order, sfixed64 /
sfixed32 as little-endian fixed-width, bools as one-byte varints, syncBlock
only when set.  oracle/gen_golden_packets.py pins it byte-for-byte to the
google.protobuf encoder.

header_v2_variant() / header_v2_padded() emit VALID encodings off that
canonical layout (protobuf-c unpacks them to the same fields), and
random_header() draws valid and invalid ones with the decode they must get,
known from how each was put together (tests/test_header_decode.py).
"""
import struct
import zlib

import numpy as np

from oracle import splitmix64_np

CSUM_NULL, CSUM_CRC32, CSUM_CRC32C = 0, 1, 2


def header_v2(offset, seqno, last, dlen, sync=None):
    b = b"\x09" + struct.pack("<q", offset) + b"\x11" + struct.pack("<q", seqno)
    b += b"\x18" + bytes([1 if last else 0]) + b"\x25" + struct.pack("<i", dlen)
    if sync is not None:
        b += b"\x28" + bytes([1 if sync else 0])
    return b


def header_class():
    """PacketHeaderProto as a google.protobuf message class, declared from
    src/proto/datatransfer.proto:228-235 (the cross-check of the builders
    here; needs google.protobuf)."""
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    fdp = descriptor_pb2.FileDescriptorProto(name="packet_header.proto", package="hadoop.hdfs", syntax="proto2")
    m = fdp.message_type.add(name="PacketHeaderProto")
    F = descriptor_pb2.FieldDescriptorProto
    for name, num, typ, lab in [("offsetInBlock", 1, F.TYPE_SFIXED64, F.LABEL_REQUIRED),
                                ("seqno", 2, F.TYPE_SFIXED64, F.LABEL_REQUIRED),
                                ("lastPacketInBlock", 3, F.TYPE_BOOL, F.LABEL_REQUIRED),
                                ("dataLen", 4, F.TYPE_SFIXED32, F.LABEL_REQUIRED),
                                ("syncBlock", 5, F.TYPE_BOOL, F.LABEL_OPTIONAL)]:
        m.field.add(name=name, number=num, type=typ, label=lab)
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName("hadoop.hdfs.PacketHeaderProto"))


# --- non-canonical PacketHeaderProto encodings --------------------------------
WT_VARINT, WT_FIXED64, WT_LEN, WT_SGROUP, WT_EGROUP, WT_FIXED32 = 0, 1, 2, 3, 4, 5
FIELD_WT = {1: WT_FIXED64, 2: WT_FIXED64, 3: WT_VARINT, 4: WT_FIXED32, 5: WT_VARINT}
MAX_FIELD = (1 << 29) - 1

REJECT_REASONS = ("missing", "wire_type", "group", "wt6", "wt7", "field0", "trunc_tag", "trunc_varint",
                  "trunc_fixed", "trunc_len", "unterminated")


def pb_varint(v, nbytes=None):
    """Varint of v >= 0, padded with continuation bytes to nbytes when given
    (0x81 0x80 0x00 is 1 in three bytes)."""
    out = bytearray()
    while True:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
        if not v:
            break
    if nbytes is not None:
        assert nbytes >= len(out), (nbytes, len(out))
        out += b"\x80" * (nbytes - len(out))
    out[-1] &= 0x7F
    return bytes(out)


def pb_tag(field, wt, pad=0):
    """Tag of (field, wire type) with `pad` extra continuation bytes; a tag
    is at most 5 bytes (protobuf-c's parse_tag_and_wiretype)."""
    t = pb_varint((field << 3) | wt)
    assert len(t) + pad <= 5, (field, pad)
    return pb_varint((field << 3) | wt, len(t) + pad)


def pb_bool(v, nbytes=1, bit=0):
    """A bool as a varint of nbytes bytes; a true one has payload bit `bit`
    set (any bit makes protobuf-c's bool true; bit < 7 * nbytes, and < 64 so
    that every decoder agrees)."""
    assert 1 <= nbytes <= 10 and bit < min(7 * nbytes, 64)
    return pb_varint((1 << bit) if v else 0, nbytes)


def pb_known(field, value, tag_pad=0, bool_bytes=1, bool_bit=0):
    """One known field of PacketHeaderProto."""
    t = pb_tag(field, FIELD_WT[field], tag_pad)
    if field in (1, 2):
        return t + struct.pack("<q", value)
    if field == 4:
        return t + struct.pack("<i", value)
    return t + pb_bool(value, bool_bytes, bool_bit)


def pb_unknown(field, wt, payload=0, tag_pad=0, len_bytes=None):
    """A field of the given number and wire type: payload is the value
    (varint, fixed64, fixed32) or, length-delimited, the payload bytes or
    their count (len_bytes: width of the length varint, at most 5)."""
    t = pb_tag(field, wt, tag_pad)
    if wt == WT_VARINT:
        return t + pb_varint(payload)
    if wt == WT_FIXED64:
        return t + struct.pack("<Q", payload & (2**64 - 1))
    if wt == WT_FIXED32:
        return t + struct.pack("<I", payload & (2**32 - 1))
    assert wt == WT_LEN, wt
    body = bytes((7 * i + 3) & 0xFF for i in range(payload)) if isinstance(payload, int) else bytes(payload)
    assert len_bytes is None or len_bytes <= 5
    return t + pb_varint(len(body), len_bytes) + body


def header_v2_variant(offset, seqno, last, dlen, sync=None, *, order=(1, 2, 3, 4, 5), repeat=None, unknown=(),
                      tag_pad=0, bool_bytes=1):
    """One valid non-canonical PacketHeaderProto of the given field values.
    order: the known fields' order (5 is emitted only when sync is not
    None); repeat: a known field emitted twice -- at its place in `order`
    with a WRONG value and again, right, after the other known fields (last
    occurrence wins); unknown: (slot, field number, wire type, payload)
    entries, emitted before the slot-th emitted known field (slot >= their
    count: at the end), payload as in pb_unknown; tag_pad: continuation
    bytes added to every tag; bool_bytes: width of the bool varints (1-10; a
    true one is 0x80 .. 0x80 0x01, its only set bit in the last byte)."""
    vals = {1: offset, 2: seqno, 3: bool(last), 4: dlen, 5: bool(sync)}
    wrong = {1: offset ^ 0x5A5A5A5A5A, 2: seqno + 12345, 3: not last, 4: dlen ^ 0x1234, 5: not sync}
    assert sorted(order) == [1, 2, 3, 4, 5], order
    fields = [f for f in order if f != 5 or sync is not None]
    assert repeat is None or repeat in fields
    bit = 7 * (bool_bytes - 1)  # a true bool's only set bit lies in its last byte
    elems = [pb_known(f, wrong[f] if f == repeat else vals[f], tag_pad, bool_bytes, bit) for f in fields]
    if repeat is not None:
        elems.append(pb_known(repeat, vals[repeat], tag_pad, bool_bytes, bit))
    out = []
    for i in range(len(elems) + 1):
        for slot, field, wt, pl in unknown:
            if min(slot, len(elems)) == i:
                assert field > 5
                out.append(pb_unknown(field, wt, pl, tag_pad))
        if i < len(elems):
            out.append(elems[i])
    return b"".join(out)


def header_v2_padded(total, offset, seqno, last, dlen, sync=None, front=True):
    """The canonical fields plus one unknown length-delimited field 6 sized
    so that the wire header [plen][hlen][PacketHeaderProto] is exactly
    `total` = 6 + hlen bytes; front: the padding comes first, so the known
    fields lie behind it."""
    core = header_v2(offset, seqno, last, dlen, sync)
    room = total - 6 - len(core) - 1  # the padding field's length varint + payload
    for nb in range(1, 6):
        n = room - nb
        if n >= 0 and len(pb_varint(n)) <= nb:
            pad = pb_unknown(6, WT_LEN, n, len_bytes=nb)
            out = pad + core if front else core + pad
            assert 6 + len(out) == total and len(out) <= 0xFFFF
            return out
    raise ValueError(total)


def _rand_field(rng, known_ok=False):
    """A field number: mostly unknown ones with 1-, 2- and 5-byte tags."""
    r = rng.random()
    if known_ok and r < 0.3:
        return int(rng.integers(1, 6))
    if r < 0.6:
        return int(rng.integers(6, 16))
    if r < 0.8:
        return int(rng.integers(16, 2048))
    return int(rng.integers(2048, MAX_FIELD + 1))


def _rand_pad(rng, field, wt):
    room = 5 - len(pb_varint((field << 3) | wt))
    return int(rng.integers(0, room + 1)) if rng.random() < 0.3 else 0


def _rand_value(rng, wt):
    """A well-formed value of wire type 0, 1, 2 or 5 (what follows the tag)."""
    if wt == WT_VARINT:
        nb = int(rng.integers(1, 11))
        v = int(rng.integers(0, 1 << 62)) & ((1 << min(7 * nb, 63)) - 1)
        return pb_varint(v, nb)
    if wt == WT_LEN:
        n = int(rng.choice([0, 1, 3, 40, 127, 128, 300]))
        nb = int(rng.integers(len(pb_varint(n)), 6)) if rng.random() < 0.3 else None
        return pb_varint(n, nb) + rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return rng.integers(0, 256, 8 if wt == WT_FIXED64 else 4, dtype=np.uint8).tobytes()


def _rand_elem(rng, field, wt):
    """A well-formed field of any number with wire type 0, 1, 2 or 5."""
    return pb_tag(field, wt, _rand_pad(rng, field, wt)) + _rand_value(rng, wt)


def random_header(rng, info=None):
    """One random PacketHeaderProto encoding -> (bytes, expected): expected
    is the (offset, seqno, last, dlen, sync) protobuf-c's unpack gives it, or
    None when it must be rejected -- known from how the bytes were put
    together, never from a decoder.  info (a dict) receives "reason": None or
    one of REJECT_REASONS.  A rejected header is a valid one with exactly one
    defect added.  dataLen is 0 in most draws (the header of an empty packet)
    and any int32 in the others."""
    off = int(rng.integers(-(1 << 63), 1 << 63))
    seq = int(rng.integers(-(1 << 63), 1 << 63))
    last = bool(rng.random() < 0.8)
    dlen = 0 if rng.random() < 0.7 else int(rng.integers(-(1 << 31), 1 << 31))
    sync = None if rng.random() < 0.5 else bool(rng.integers(0, 2))
    vals = {1: off, 2: seq, 3: last, 4: dlen, 5: bool(sync)}
    reason = None if rng.random() < 0.45 else REJECT_REASONS[int(rng.integers(0, len(REJECT_REASONS)))]
    missing = int(rng.integers(1, 5)) if reason == "missing" else 0

    def known(f, v):
        nb = int(rng.integers(1, 11)) if rng.random() < 0.5 else 1
        return pb_known(f, v, _rand_pad(rng, f, FIELD_WT[f]), nb, int(rng.integers(0, min(7 * nb, 64))))

    elems = []
    for f in rng.permutation([1, 2, 3, 4, 5]):
        f = int(f)
        if (f == 5 and sync is None) or f == missing:
            continue
        elems.append((f, known(f, vals[f])))
    # repeated fields: an earlier copy with another value (last one wins)
    for f, _ in list(elems):
        if rng.random() < 0.2:
            other = (not vals[f]) if f in (3, 5) else int(rng.integers(-(1 << 31), 1 << 31))
            at = next(i for i, e in enumerate(elems) if e[0] == f)
            elems.insert(int(rng.integers(0, at + 1)), (0, known(f, other)))
    elems = [e for _, e in elems]
    for _ in range(int(rng.integers(0, 4))):  # unknown fields, skipped
        wt = int(rng.choice([WT_VARINT, WT_FIXED64, WT_LEN, WT_FIXED32]))
        elems.insert(int(rng.integers(0, len(elems) + 1)), _rand_elem(rng, _rand_field(rng), wt))

    def anywhere(e):
        elems.insert(int(rng.integers(0, len(elems) + 1)), e)

    if reason == "wire_type":  # a known field, well formed, in another field's wire type
        f = int(rng.integers(1, 6))
        anywhere(_rand_elem(rng, f, int(rng.choice([w for w in (0, 1, 2, 5) if w != FIELD_WT[f]]))))
    elif reason == "group":  # a lone start-group or end-group tag
        f = _rand_field(rng, known_ok=True)
        wt = int(rng.choice([WT_SGROUP, WT_EGROUP]))
        anywhere(pb_tag(f, wt, _rand_pad(rng, f, wt)))
    elif reason in ("wt6", "wt7"):
        f = _rand_field(rng, known_ok=True)
        wt = 6 if reason == "wt6" else 7
        anywhere(pb_tag(f, wt, _rand_pad(rng, f, wt)) + rng.integers(0, 256, int(rng.integers(0, 9)),
                                                                       dtype=np.uint8).tobytes())
    elif reason == "field0":  # one-byte tag of field number 0
        wt = int(rng.choice([WT_VARINT, WT_FIXED64, WT_LEN, WT_FIXED32]))
        anywhere(bytes([wt]) + _rand_value(rng, wt))
    elif reason == "unterminated":
        if rng.random() < 0.25:  # a tag whose fifth byte still continues
            anywhere(b"\xc8\x80\x80\x80\x80\x01" + b"\x00")
        else:  # a varint whose tenth byte still continues
            f = int(rng.choice([3, 5])) if rng.random() < 0.5 else _rand_field(rng)
            anywhere(pb_tag(f, WT_VARINT) + b"\x81" + b"\x80" * 9 + b"\x00" * int(rng.integers(1, 3)))
    elif reason == "trunc_tag":  # the message ends inside a tag
        f = int(rng.integers(16, MAX_FIELD + 1))
        wt = int(rng.choice([0, 1, 2, 5]))
        t = pb_tag(f, wt, _rand_pad(rng, f, wt))
        elems.append(t[:int(rng.integers(1, len(t)))])
    elif reason == "trunc_varint":  # ... inside a varint value
        f = int(rng.choice([3, 5])) if rng.random() < 0.5 else _rand_field(rng)
        nb = int(rng.integers(2, 11))
        elems.append(pb_tag(f, WT_VARINT) + pb_varint(1, nb)[:int(rng.integers(0, nb))])
    elif reason == "trunc_fixed":  # ... inside a fixed64 / fixed32 value
        f = int(rng.choice([1, 2, 4])) if rng.random() < 0.5 else _rand_field(rng)
        wt = FIELD_WT.get(f, int(rng.choice([WT_FIXED64, WT_FIXED32])))
        e = pb_unknown(f, wt, int(rng.integers(0, 1 << 63)))
        elems.append(e[:len(e) - int(rng.integers(1, 9 if wt == WT_FIXED64 else 5))])
    elif reason == "trunc_len":  # ... inside a length-delimited field or its length
        f = _rand_field(rng)
        n = int(rng.choice([1, 5, 127, 128, 300, 70000, (1 << 31) - 1, (1 << 32) - 1]))
        e = pb_tag(f, WT_LEN, _rand_pad(rng, f, WT_LEN)) + pb_varint(n, 5 if rng.random() < 0.2 else None)
        if rng.random() < 0.2 and len(pb_varint(n)) > 1:
            elems.append(e[:-1])  # the length varint itself is cut
        else:
            elems.append(e + bytes(int(rng.integers(0, min(n, 64)))))
    if info is not None:
        info["reason"] = reason
    return b"".join(elems), (None if reason else (off, seq, last, dlen, bool(sync)))


def frame_v2(hdr, crcs, data, plen=None):
    if plen is None:
        plen = 4 + len(crcs) + len(data)
    return struct.pack(">iH", plen, len(hdr)) + hdr + crcs + data


def frame_v1(offset, seqno, last, crcs, data, plen=None, dlen=None, last_byte=None):
    if plen is None:
        plen = 4 + len(crcs) + len(data)
    if dlen is None:
        dlen = len(data)
    lb = (1 if last else 0) if last_byte is None else last_byte
    return struct.pack(">iqqBi", plen, offset, seqno, lb, dlen) + crcs + data


def chunk_crcs_be(data, cs, ctype, crc32c):
    """BE CRC bytes of data's chunks; crc32c(crc, bytes) is the CRC32C function
    to use (the oracle, in tests and in the fixture generator)."""
    out = []
    for i in range(0, len(data), cs):
        piece = bytes(data[i:i + cs])
        c = zlib.crc32(piece) if ctype == CSUM_CRC32 else crc32c(0, piece)
        out.append(int(c).to_bytes(4, "big"))
    return b"".join(out)


def payload(seed, g0, n):
    return splitmix64_np((n + 7) // 8, seed=seed, g0=g0).view(np.uint8)[:n].copy()


def assemble(parts):
    """Fixture parts -> stream bytes: {"hex": ...} literal wire bytes or
    {"data": {"seed", "g0", "len"}, "flips": [[byte, mask], ...]}."""
    out = []
    for p in parts:
        if "hex" in p:
            out.append(bytes.fromhex(p["hex"]))
        else:
            d = payload(p["data"]["seed"], p["data"]["g0"], p["data"]["len"])
            for off, mask in p.get("flips", []):
                d[off] ^= np.uint8(mask)
            out.append(d.tobytes())
    return b"".join(out)


def build_stream(crc32c, proto, cs, ctype, dlens, seed=0, corrupt=(), last_empty=True, sync_every=0,
                 seqnos=None, offset_skew=None, offset0=0, last_flag=None, sync_at=(), header=None):
    """A clean stream of packets with the given data lengths (the last one
    flagged lastPacketInBlock unless last_empty adds the v2-style trailing
    empty packet).  corrupt: iterable of (packet, chunk) -> flip one bit of
    that chunk after its CRC is computed.  seqnos: header seqno per packet
    (default k); offset_skew: {packet: bytes added to its offsetInBlock} --
    header fields off the regular progression, same wire sizes.  offset0:
    offsetInBlock of the first packet (a read from inside a block);
    last_flag: packet index flagged lastPacketInBlock instead; sync_at:
    packets whose v2 header carries syncBlock (27-B headers).  header: a
    callable (k, offset, seqno, last, dlen) -> PacketHeaderProto bytes of v2
    packet k (the trailing empty one included) instead of header_v2.  Returns
    (stream bytes, expected per-packet bad chunk lists)."""
    out = []
    bad = {}
    for pk, ch in corrupt:
        bad.setdefault(pk, []).append(ch)
    off = 0
    for k, dl in enumerate(dlens):
        d = payload(seed, off // 8 + 1000 * k, dl)
        crcs = chunk_crcs_be(d, cs, ctype, crc32c) if ctype != CSUM_NULL else b""
        for ch in bad.get(k, []):
            clen = min(cs, dl - ch * cs)
            d[ch * cs + (k * 7919 + ch) % clen] ^= np.uint8(1 << (ch % 8))
        last = (k == len(dlens) - 1) and not last_empty if last_flag is None else k == last_flag
        seq = k if seqnos is None else seqnos[k]
        ho = offset0 + off + (offset_skew or {}).get(k, 0)
        if proto == 1:
            out.append(frame_v1(ho, seq, last, crcs, d.tobytes()))
        else:
            sync = (k % sync_every == 0) if sync_every else (True if k in sync_at else None)
            hdr = header(k, ho, seq, last, dl) if header else header_v2(ho, seq, last, dl, sync)
            out.append(frame_v2(hdr, crcs, d.tobytes()))
        off += dl
    if last_empty:
        k = len(dlens)
        if proto == 1:
            out.append(frame_v1(offset0 + off, k, True, b"", b""))
        else:
            hdr = header(k, offset0 + off, k, True, 0) if header else header_v2(offset0 + off, k, True, 0)
            out.append(frame_v2(hdr, b"", b""))
    return b"".join(out), {k: sorted(set(v)) for k, v in bad.items()}
