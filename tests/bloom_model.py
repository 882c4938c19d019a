"""Independent model of the tables' bloom filter (steakknife/bloomfilter as the reference's sstables package
uses it), restated from the format rules alone; the tests compare sstables.bloom.Filter and the device
kernels against it. It shares no code with the package.

File: one gzip member. Payload, little-endian uint64: k, n, m, k hash keys, ceil(m / 64) bit words, then the
SHA-384 of every payload byte before it. Bit i is bit i & 63 of word i >> 6. An element is FNV-1 (64 bit) of
the key: h = 0xcbf29ce484222325; per byte h = h * 0x100000001b3 mod 2^64, then h ^= byte. Probe j of a key is
bit (h ^ hash_key[j]) mod m.
"""
import gzip
import hashlib
import math
import struct

MASK = (1 << 64) - 1


def fnv1_64(key: bytes) -> int:
    h = 0xCBF29CE484222325
    for b in key:
        h = (h * 0x100000001B3) & MASK
        h ^= b
    return h


def optimal(max_n: int, p: float):
    m = math.ceil(-max_n * math.log(p) / (math.log(2) ** 2))
    k = math.ceil(math.log(2) * m / max_n)
    return m, k


class Model:
    def __init__(self, m: int, hash_keys, words=None, n: int = 0):
        self.m, self.keys, self.n = m, list(hash_keys), n
        self.words = list(words) if words is not None else [0] * ((m + 63) // 64)

    @property
    def k(self):
        return len(self.keys)

    def probes(self, key: bytes):
        h = fnv1_64(key)
        return [(h ^ hk) % self.m for hk in self.keys]

    def add(self, key: bytes):
        for i in self.probes(key):
            self.words[i >> 6] |= 1 << (i & 63)
        self.n += 1

    def contains(self, key: bytes) -> bool:
        return all((self.words[i >> 6] >> (i & 63)) & 1 for i in self.probes(key))

    def popcount(self) -> int:
        return sum(bin(w).count("1") for w in self.words)

    def payload(self) -> bytes:
        body = struct.pack(f"<3Q{self.k}Q{len(self.words)}Q", self.k, self.n, self.m, *self.keys, *self.words)
        return body + hashlib.sha384(body).digest()


def sparse_words(m: int, hash_keys, keys) -> dict:
    """{word index: word} of a filter holding `keys`, for an m whose word list would not fit a Python list."""
    f = Model(2, hash_keys)  # only probes() is used, with the real m
    f.m = m
    out = {}
    for key in keys:
        for i in f.probes(key):
            out[i >> 6] = out.get(i >> 6, 0) | (1 << (i & 63))
    return out


def words_fixed_np(m: int, hash_keys, rows):
    """The bit words (numpy uint64) of a filter holding every row of `rows` (uint8 [n, key_len]) as a key: the
    same rules in array arithmetic (uint64 arrays wrap mod 2^64), for key counts a Python loop would crawl over."""
    import numpy as np

    rows = np.asarray(rows, dtype=np.uint8)
    h = np.full(rows.shape[0], 0xCBF29CE484222325, dtype=np.uint64)
    for c in range(rows.shape[1]):
        h = (h * np.uint64(0x100000001B3)) ^ rows[:, c].astype(np.uint64)
    words = np.zeros((m + 63) // 64, dtype=np.uint64)
    for hk in hash_keys:
        idx = (h ^ np.uint64(hk)) % np.uint64(m)
        np.bitwise_or.at(words, (idx >> np.uint64(6)).astype(np.int64), np.uint64(1) << (idx & np.uint64(63)))
    return words


def parse(raw: bytes) -> Model:
    """A bloom.bf.gz image -> Model; ValueError when it is not one."""
    try:
        body = gzip.decompress(raw)
    except (OSError, EOFError) as e:
        raise ValueError(f"gzip: {e}")
    if len(body) < 24 + 48:
        raise ValueError("short payload")
    k, n, m = struct.unpack_from("<3Q", body, 0)
    nw = (m + 63) // 64
    if len(body) != 24 + 8 * k + 8 * nw + 48:
        raise ValueError("payload length does not match its header")
    if hashlib.sha384(body[:-48]).digest() != body[-48:]:
        raise ValueError("SHA-384 trailer mismatch")
    keys = struct.unpack_from(f"<{k}Q", body, 24)
    words = struct.unpack_from(f"<{nw}Q", body, 24 + 8 * k)
    return Model(m, keys, words, n)
