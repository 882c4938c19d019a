"""A plain Python model of simpledb's WAL recovery loop (simpledb/recovery.go:215-240) for the WAL-ops tests:
every record through simpledb.proto.unmarshal_wal_mutation (the host mirror of the device parser) and the
switch, giving the op list, the arrays rio_wal_ops_gather writes and the plan's result block. The expectation
table is flush_model's (the ops applied to a dict, sorted, written by the host writer).

A record is bytes, or None for a nil record. An op is (key, value): value None is a tombstone."""
import random

from simpledb import proto as P

PROTO, UTF8, VALUE_NIL, RANGE = 1, 2, 3, 4  # RIO_WAL_BAD_*
NONE = 0xFFFFFFFFFFFFFFFF
FLAG_NIL = 1


def field(num, payload, wt=2):
    """One field on the wire; wt 2 carries a length, 0 a varint (payload an int), 1 / 5 fixed bytes."""
    tag = P.put_varint(num << 3 | wt)
    if wt == 0:
        return tag + P.put_varint(payload)
    if wt == 2:
        return tag + P.put_varint(len(payload)) + bytes(payload)
    return tag + bytes(payload)


def group(num, body=b""):
    return P.put_varint(num << 3 | 3) + body + P.put_varint(num << 3 | 4)


def nested_groups(depth, num=7):
    """`depth` start-group tags, then their end tags."""
    return P.put_varint(num << 3 | 3) * depth + P.put_varint(num << 3 | 4) * depth


_memo = {}


def classify(rec):
    """-> (bad class or 0, op or None) of one record (remembered: the large cases repeat a few records)."""
    if rec is not None and len(rec) > 16:
        return _classify(rec)
    if rec not in _memo:
        _memo[rec] = _classify(rec)
    return _memo[rec]


def _classify(rec):
    try:
        m = P.unmarshal_wal_mutation(rec)
    except P.InvalidUTF8Error:
        return UTF8, None
    except P.WireError:
        return PROTO, None
    try:
        return 0, P.mutation_op(m)
    except P.ValueNilError:
        return VALUE_NIL, None


def accepted(records):
    """The records recovery does not stop at."""
    return [r for r in records if classify(r)[0] == 0]


def replay(records):
    """-> (ops, op_rec, first_bad, bad_class) of the records in order; stops at the first refused record."""
    ops, op_rec = [], []
    for g, rec in enumerate(records):
        bad, op = classify(rec)
        if bad:
            return ops, op_rec, g, bad
        if op is not None:
            ops.append(op)
            op_rec.append(g)
    return ops, op_rec, NONE, 0


def expected(records):
    """What the plan and the gather leave behind for these records (all segments concatenated): the result
    block and the six arrays. With a refused record only FIRST_BAD and BAD_CLASS of the block are meaningful
    (and returned: the other words are None)."""
    ops, op_rec, first_bad, cls = replay(records)
    if first_bad != NONE:
        return dict(result=[None] * 5 + [first_bad, cls, None])
    keys = b"".join(k for k, _ in ops)
    values = b"".join(v or b"" for _, v in ops)
    key_off, val_off = [0], [0]
    for k, v in ops:
        key_off.append(key_off[-1] + len(k))
        val_off.append(val_off[-1] + len(v or b""))
    result = [len(records), len(ops), len(keys), len(values), max([len(k) for k, _ in ops], default=0), NONE, 0, 0]
    return dict(result=result, ops=ops, keys=keys, values=values, key_off=key_off, val_off=val_off,
                flags=[FLAG_NIL if v is None else 0 for _, v in ops], op_rec=op_rec)


# ---- seeded corpus, by family ----------------------------------------------------------------------------

def _text(rng, n):
    alphabet = "abcdefghij klmnopéü€\U0001F600"
    return "".join(rng.choice(alphabet) for _ in range(n))


def ordinary(rng, n, keyspace=64):
    """What db.PutBytes / DeleteBytes / Put / Delete write, with empty and nil records in between."""
    out = []
    for _ in range(n):
        r = rng.random()
        key = b"key-%04d" % rng.randrange(keyspace)
        if r < 0.55:
            out.append(P.marshal_upsert(key, rng.randbytes(rng.randint(1, 40))))
        elif r < 0.70:
            out.append(P.marshal_delete(key))
        elif r < 0.82:
            out.append(P.marshal_upsert_str(_text(rng, rng.randint(0, 9)), _text(rng, rng.randint(0, 20))))
        elif r < 0.88:
            out.append(P.marshal_delete_str(_text(rng, rng.randint(0, 9))))
        elif r < 0.94:
            out.append(b"")
        else:
            out.append(None)
    return out


def merges(rng, n):
    """Members repeated and switched, fields repeated, unknown fields and other wire types at both levels."""
    def upsert_body():
        parts = []
        for _ in range(rng.randint(0, 5)):
            f = rng.choice((1, 2, 3, 4, 4, 3, 9))
            wt = rng.choice((2, 2, 2, 2, 0, 5, 1))
            if wt == 2:
                pay = _text(rng, rng.randint(0, 6)).encode() if f in (1, 2) else rng.randbytes(rng.randint(0, 6))
                parts.append(field(f, pay))
            elif wt == 0:
                parts.append(field(f, rng.randrange(1 << 40), 0))
            else:
                parts.append(field(f, rng.randbytes(8 if wt == 1 else 4), wt))
        return b"".join(parts)

    def delete_body():
        parts = []
        for _ in range(rng.randint(0, 3)):
            f = rng.choice((1, 2, 2, 5))
            pay = _text(rng, rng.randint(0, 6)).encode() if f == 1 else rng.randbytes(rng.randint(0, 6))
            parts.append(field(f, pay))
        return b"".join(parts)

    out = []
    for _ in range(n):
        parts = []
        for _ in range(rng.randint(1, 4)):
            r = rng.random()
            if r < 0.45:
                parts.append(field(1, upsert_body()))
            elif r < 0.75:
                parts.append(field(2, delete_body()))
            elif r < 0.85:
                parts.append(field(rng.choice((1, 2)), rng.randrange(1 << 20), 0))
            elif r < 0.93:
                parts.append(field(rng.choice((3, 15, 16, 2047)), rng.randbytes(rng.randint(0, 5))))
            else:
                parts.append(group(rng.choice((3, 9)), field(1, b"in a group")))
        out.append(b"".join(parts))
    return out


def malformed(rng, n):
    """Valid records cut short, with a byte changed, or with a length that leaves the record."""
    out = []
    base = ordinary(rng, n, 16) + merges(rng, n)
    for _ in range(n):
        rec = bytearray(rng.choice(base) or b"\x0a\x03\x1a\x01k")
        r = rng.random()
        if r < 0.4 and len(rec) > 1:
            del rec[rng.randrange(1, len(rec)):]
        elif r < 0.8 and rec:
            rec[rng.randrange(len(rec))] = rng.randrange(256)
        else:
            rec += field(rng.choice((1, 2)), b"abc")[:-rng.randint(1, 3)]
        out.append(bytes(rec))
    return out


def corpus(seed, n=300):
    """family -> records"""
    rng = random.Random(seed)
    return {"ordinary": ordinary(rng, n), "merges": merges(rng, n), "malformed": malformed(rng, n)}
