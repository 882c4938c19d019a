"""Host-side protobuf wire helpers for simpledb's WAL records (simpledb/proto/wal_mutation.proto).

    message WalMutation { oneof mutation { UpsertMutation addition = 1; DeleteTombstoneMutation deleteTombStone = 2; } }
    message UpsertMutation { string key = 1; string value = 2; bytes keyBytes = 3; bytes valueBytes = 4; }
    message DeleteTombstoneMutation { string key = 1; bytes keyBytes = 2; }

The marshal helpers write what db.PutBytes / DeleteBytes / Put / Delete append to the WAL (db.go:256-320):
proto.Marshal with deterministic field order and proto3 defaults omitted. unmarshal_wal_mutation is
proto.Unmarshal into a reset WalMutation, the host mirror of the device parser (pb_wal_mutation_t,
csrc/rio_pb.h) and the one-record path: recovery runs it on the one record the device refused, for the error
text. Bulk parsing runs on the device (rio_wal_ops_plan).

CompactionMetadata (simpledb/proto/compaction_metadata.proto) is the one record of a compaction's
compaction_successful file: marshal_compaction_metadata / unmarshal_compaction_metadata, with the same rules.
"""
from __future__ import annotations

from dataclasses import dataclass

from sstables.proto import _skip_group, _varint, put_varint

ADDITION, DELETE_TOMBSTONE = 1, 2  # WalMutation's oneof members = their field numbers

# field number -> (name, is a proto3 string) of the two member messages
_FIELDS = {
    ADDITION: {1: ("key", True), 2: ("value", True), 3: ("keyBytes", False), 4: ("valueBytes", False)},
    DELETE_TOMBSTONE: {1: ("key", True), 2: ("keyBytes", False)},
}
_MESSAGE = {ADDITION: "UpsertMutation", DELETE_TOMBSTONE: "DeleteTombstoneMutation"}


class WireError(ValueError):
    """proto.Unmarshal's "cannot parse invalid wire-format data" (malformed tag, length or group)."""


class InvalidUTF8Error(ValueError):
    """A proto3 string field whose bytes are not valid UTF-8; `field` is its full name."""

    def __init__(self, field: str):
        super().__init__(f"field {field} contains invalid UTF-8")
        self.field = field


@dataclass
class WalMutation:
    """member: None, ADDITION or DELETE_TOMBSTONE; the member's fields as bytes (an absent field is b"")."""

    member: "int | None" = None
    key: bytes = b""
    value: bytes = b""
    keyBytes: bytes = b""
    valueBytes: bytes = b""


def _field(num: int, payload: bytes) -> bytes:
    return put_varint(num << 3 | 2) + put_varint(len(payload)) + payload


def _member(num: int, fields) -> bytes:
    body = b"".join(_field(n, bytes(v)) for n, v in fields if v)  # proto3: an empty field is omitted
    return _field(num, body)  # the oneof member is written even when its message is empty


def marshal_upsert(key_bytes: bytes, value_bytes: bytes) -> bytes:
    """db.PutBytes's record (db.go:258-265): addition {keyBytes, valueBytes}."""
    return _member(ADDITION, ((3, key_bytes), (4, value_bytes)))


def marshal_delete(key_bytes: bytes) -> bytes:
    """db.DeleteBytes's record (db.go:312-318): deleteTombStone {keyBytes}."""
    return _member(DELETE_TOMBSTONE, ((2, key_bytes),))


def marshal_upsert_str(key: str, value: str) -> bytes:
    """The string-field form: addition {key, value}."""
    return _member(ADDITION, ((1, key.encode()), (2, value.encode())))


def marshal_delete_str(key: str) -> bytes:
    """The string-field form: deleteTombStone {key}."""
    return _member(DELETE_TOMBSTONE, ((1, key.encode()),))


def utf8_valid(b: bytes) -> bool:
    """Go's utf8.Valid: shortest forms, no surrogates, nothing above U+10FFFF (CPython's strict decoder)."""
    try:
        bytes(b).decode("utf-8", "strict")
        return True
    except UnicodeDecodeError:
        return False


def _skip(b: bytes, pos: int, end: int, num: int, wt: int) -> int:
    """protowire.ConsumeFieldValue inside b[:end]."""
    if wt == 0:
        _, pos = _varint(b[:end], pos)
        return pos
    if wt in (1, 5):
        w = 8 if wt == 1 else 4
        if w > end - pos:
            raise ValueError("truncated fixed")
        return pos + w
    if wt == 2:
        ln, pos = _varint(b[:end], pos)
        if ln > end - pos:
            raise ValueError("truncated bytes")
        return pos + ln
    if wt == 3:
        return _skip_group(b[:end], pos, num)
    raise ValueError(f"wire type {wt}")


def _tag(b: bytes, pos: int):
    tag, pos = _varint(b, pos)
    num, wt = tag >> 3, tag & 7
    if num < 1 or num > 0x1FFFFFFF:
        raise ValueError("invalid field number")
    return num, wt, pos


def unmarshal_wal_mutation(b) -> WalMutation:
    """proto.Unmarshal(b, &WalMutation{}). Fields in wire order; the member seen last is the oneof's; a
    member seen again while it is the current one merges (each field keeps its last occurrence), a switch to
    the other member starts it empty; a known field with another wire type and unknown fields are skipped at
    both levels; every occurrence of a string field must be valid UTF-8. None (a nil record) is the empty
    message. Raises WireError / InvalidUTF8Error (both ValueError)."""
    m = WalMutation()
    b = b"" if b is None else bytes(b)
    pos = 0
    try:
        while pos < len(b):
            num, wt, pos = _tag(b, pos)
            if num not in _FIELDS or wt != 2:
                pos = _skip(b, pos, len(b), num, wt)
                continue
            ln, pos = _varint(b, pos)
            if ln > len(b) - pos:
                raise ValueError("truncated message")
            if m.member != num:
                m = WalMutation(member=num)
            end = pos + ln
            sub = b[:end]
            while pos < end:
                f, w, pos = _tag(sub, pos)
                known = _FIELDS[num].get(f)
                if known is None or w != 2:
                    pos = _skip(sub, pos, end, f, w)
                    continue
                fl, pos = _varint(sub, pos)
                if fl > end - pos:
                    raise ValueError("truncated field")
                name, is_string = known
                payload = sub[pos:pos + fl]
                if is_string and not utf8_valid(payload):
                    raise InvalidUTF8Error(f"proto.{_MESSAGE[num]}.{name}")
                setattr(m, name, payload)
                pos += fl
    except InvalidUTF8Error:
        raise
    except ValueError as e:
        raise WireError(f"cannot parse invalid wire-format data ({e})") from None
    return m


@dataclass
class CompactionMetadata:
    """simpledb/proto/compaction_metadata.proto: message CompactionMetadata { string writePath = 1;
    string replacementPath = 2; repeated string sstablePaths = 3; }. Paths are str; bytes that are not UTF-8
    cannot be a field's value (surrogate escapes marshal back to them and fail the check)."""

    writePath: str = ""
    replacementPath: str = ""
    sstablePaths: "list[str]" = None

    def __post_init__(self):
        self.sstablePaths = list(self.sstablePaths or [])


_COMPACTION_FIELDS = {1: "writePath", 2: "replacementPath", 3: "sstablePaths"}


def marshal_compaction_metadata(m: CompactionMetadata) -> bytes:
    """proto.Marshal(CompactionMetadata): fields in number order, the empty singular strings left out, every
    element of the repeated field written (an empty one too). A string that is not valid UTF-8 raises
    InvalidUTF8Error, as proto.Marshal refuses it."""
    out = []
    for num, vals in ((1, [m.writePath]), (2, [m.replacementPath]), (3, m.sstablePaths)):
        for v in vals:
            b = v.encode("utf-8", "surrogateescape") if isinstance(v, str) else bytes(v)
            if not utf8_valid(b):
                raise InvalidUTF8Error(f"proto.CompactionMetadata.{_COMPACTION_FIELDS[num]}")
            if b or num == 3:
                out.append(_field(num, b))
    return b"".join(out)


def unmarshal_compaction_metadata(b) -> CompactionMetadata:
    """proto.Unmarshal(b, &CompactionMetadata{}): fields in wire order, a singular field keeps its last
    occurrence, the repeated one appends; a known field with another wire type and unknown fields are skipped;
    every string must be valid UTF-8. Raises WireError / InvalidUTF8Error (both ValueError)."""
    m = CompactionMetadata()
    b = b"" if b is None else bytes(b)
    pos = 0
    try:
        while pos < len(b):
            num, wt, pos = _tag(b, pos)
            name = _COMPACTION_FIELDS.get(num)
            if name is None or wt != 2:
                pos = _skip(b, pos, len(b), num, wt)
                continue
            ln, pos = _varint(b, pos)
            if ln > len(b) - pos:
                raise ValueError("truncated field")
            payload = b[pos:pos + ln]
            pos += ln
            if not utf8_valid(payload):
                raise InvalidUTF8Error(f"proto.CompactionMetadata.{name}")
            if num == 3:
                m.sstablePaths.append(payload.decode())
            else:
                setattr(m, name, payload.decode())
    except InvalidUTF8Error:
        raise
    except ValueError as e:
        raise WireError(f"cannot parse invalid wire-format data ({e})") from None
    return m


def mutation_op(m: WalMutation):
    """The switch of recovery.go:224-237 on an unmarshalled record: None (no member: nothing is applied),
    or (key, value) with value None for a tombstone. An addition whose keyBytes is set and whose valueBytes is
    absent or empty is Upsert(key, nil): ("value was nil", memstore.go:124) is raised as ValueNilError."""
    if m.member == ADDITION:
        if m.keyBytes:
            if not m.valueBytes:
                raise ValueNilError()
            return m.keyBytes, m.valueBytes
        return m.key, m.value
    if m.member == DELETE_TOMBSTONE:
        return (m.keyBytes if m.keyBytes else m.key), None
    return None


class ValueNilError(ValueError):
    """memstore.Upsert(key, nil)."""

    def __init__(self):
        super().__init__("value was nil")
