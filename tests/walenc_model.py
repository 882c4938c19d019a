"""Host model of rio_wal_ops_encode (csrc/rio_walenc.hip) and of wal.batch_cuts, for test_walenc_host.py and
test_gpu_wal_encode.py. An op is (key, value, nil): nil marks a delete, whose value bytes still lie in the value
arena (the op log allows a range behind a nil flag; it must be neither read nor emitted). The records come from
simpledb.proto.marshal_upsert / marshal_delete, the byte-exact model of db.go:258-265 / :312-318."""
import random

import numpy as np

from recordio import _lib as L
from simpledb import proto as P

NONE = 0xFFFFFFFFFFFFFFFF
RANGE = L.RIO_WAL_BAD_RANGE


def put(key, value):
    return (bytes(key), bytes(value), False)


def delete(key, hidden=b""):
    return (bytes(key), bytes(hidden), True)


def record(op) -> bytes:
    key, value, nil = op
    return P.marshal_delete(key) if nil else P.marshal_upsert(key, value)


def field_len(n: int) -> int:
    return 1 + len(P.put_varint(n)) + n if n else 0


def body_len(op) -> int:
    """The member message's length; checked against the marshalled record."""
    key, value, nil = op
    body = field_len(len(key)) + (0 if nil else field_len(len(value)))
    rec = record(op)
    assert len(rec) == 1 + len(P.put_varint(body)) + body and rec[1:1 + len(P.put_varint(body))] == P.put_varint(body)
    return body


def arrays(ops):
    """The op log's host arrays: keys, key_off, values, val_off, flags."""
    keys = b"".join(o[0] for o in ops)
    values = b"".join(o[1] for o in ops)
    key_off = np.cumsum([0] + [len(o[0]) for o in ops]).astype(np.int64)
    val_off = np.cumsum([0] + [len(o[1]) for o in ops]).astype(np.int64)
    flags = np.asarray([L.RIO_FLAG_NIL if o[2] else 0 for o in ops], dtype=np.uint8)
    return keys, key_off, values, val_off, flags


def expected(ops):
    """-> records, arena, rec_off and the result block of a good log."""
    recs = [record(o) for o in ops]
    rec_off = np.cumsum([0] + [len(r) for r in recs]).tolist()
    dels = sum(o[2] for o in ops)
    result = [len(ops), rec_off[-1], len(ops) - dels, dels, max([len(o[0]) for o in ops], default=0), NONE, 0, 0]
    return dict(records=recs, arena=b"".join(recs), rec_off=rec_off, result=result)


def first_bad(key_off, val_off, key_bytes, value_bytes):
    """The smallest op whose key or value range is not monotone or leaves its arena; NONE when all are good."""
    for i in range(len(key_off) - 1):
        for off, size in ((key_off, key_bytes), (val_off, value_bytes)):
            a, b = int(off[i]), int(off[i + 1])
            if a > size or b < a or b > size:
                return i
    return NONE


def corpus(seed: int, n: int):
    """Seeded ops: keys of 0-40 bytes, values of 0-300, every eighth or so a delete (some over hidden bytes)."""
    rng = random.Random(seed)
    ops = []
    for _ in range(n):
        key = rng.randbytes(rng.choice((0, 1, 5, 16, 16, 16, 40)))
        if rng.random() < 0.15:
            ops.append(delete(key, rng.randbytes(rng.choice((0, 0, 7)))))
        else:
            ops.append(put(key, rng.randbytes(rng.choice((0, 1, 20, 100, 300)))))
    return ops


def accepted_corpus(seed: int, n: int, keys: int = 200):
    """Seeded ops recovery accepts: non-empty keys (repeating), non-empty values on upserts."""
    rng = random.Random(seed)
    ops = []
    for i in range(n):
        key = b"user/%04d" % rng.randrange(keys)
        if rng.random() < 0.2:
            ops.append(delete(key))
        else:
            ops.append(put(key, rng.randbytes(rng.randint(1, 150)) + b"#%d" % i))
    return ops


def batch_cuts_loop(size0, raw_len, framed_len, max_size):
    """Appender._check_size_and_rotate (appender.go:72) record by record."""
    cuts, size = [], size0
    for i, (raw, framed) in enumerate(zip(raw_len, framed_len)):
        if size + raw > max_size:
            cuts.append(i)
            size = 8
        size += framed
    return cuts
