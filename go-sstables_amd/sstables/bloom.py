"""The tables' bloom filter: mirror of github.com/steakknife/bloomfilter as the reference's sstables package
uses it (sstable_writer.go:78-83,114-118,150-154; sstable_reader.go:49-65,343-353).

The file format and the hash are pinned by the reference's nine bloom.bf.gz fixtures (tests/golden/bloom):

- the file is one gzip member (any valid gzip reads);
- payload, all little-endian uint64: k, n, m, then k hash keys, then ceil(m / 64) bit words, then 48 bytes:
  the SHA-384 of every payload byte before them;
- bit i is bit i & 63 of word i >> 6;
- n counts Add calls and is not validated on read;
- an element is hash/fnv New64 of the key, which is FNV-1 (not FNV-1a): h = 0xcbf29ce484222325, per byte
  h = h * 0x100000001b3, then h ^= byte;
- probe j of a key is bit (h ^ hash_key[j]) mod m; Add sets all k bits, Contains needs all k;
- NewOptimal(maxN, p): m = ceil(-maxN ln p / ln^2 2), k = ceil(ln 2 m / maxN); (1000, 0.01) -> (9586, 7).

The hash keys are random per filter, so a written file is never byte-comparable with the reference's; its
membership is. Parity unpinned (the library's source was not at hand): the limits it sets on m and k and on
trailing bytes, its error texts, and the last ulp of Go's math.Log against libm away from the pinned point.

Filter is the host copy: serialisation (gzip, hashlib) and single-key Add / Contains. on_device() gives the
bits and hash keys as resident tensors with the rio_bloom_view the kernels of csrc/rio_bloom.hip take.
Functions return Go-style error values.
"""
from __future__ import annotations

import ctypes
import gzip
import hashlib
import os
import struct
import zlib

from recordio import _lib as L
from recordio.errors import GoError

_MASK = (1 << 64) - 1
_FNV_BASIS, _FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3


def fnv1_64(key: bytes) -> int:
    """hash/fnv New64 over the key (sstable_writer.go:115-116, sstable_reader.go:52-53)."""
    h = _FNV_BASIS
    for b in bytes(key):
        h = ((h * _FNV_PRIME) & _MASK) ^ b
    return h


def optimal(max_n: int, p: float):
    """(m, k) of bloomfilter.NewOptimal, computed by the library (rio_bloom_optimal); (None, None) when refused."""
    m, k = ctypes.c_uint64(), ctypes.c_uint64()
    try:
        rc = L.lib().rio_bloom_optimal(int(max_n), float(p), ctypes.byref(m), ctypes.byref(k))
    except (ctypes.ArgumentError, OverflowError):
        rc = L.RIO_ERR_ARG
    return (m.value, k.value) if rc == L.RIO_OK else (None, None)


class DeviceFilter:
    """A filter's bits (int64 words) and hash keys resident on a device, and the view the kernels take."""

    def __init__(self, bits, hash_keys, m: int, k: int):
        self.bits, self.hash_keys, self.m, self.k = bits, hash_keys, m, k
        self.view = L.BloomView(bits=bits.data_ptr(), hash_keys=hash_keys.data_ptr(), m=m, k=k)

    def ref(self):
        return ctypes.byref(self.view)


class Filter:
    def __init__(self, m: int, hash_keys, bits: bytearray | None = None, n: int = 0):
        self.m, self.keys, self.n = int(m), [int(x) & _MASK for x in hash_keys], int(n)
        self._bits = bits  # zero bits are allocated at their first use: a device build never touches them

    @property
    def bits(self) -> bytearray:
        if self._bits is None:
            self._bits = bytearray(8 * ((self.m + 63) // 64))
        return self._bits

    @property
    def k(self) -> int:
        return len(self.keys)

    def M(self) -> int:  # noqa: N802
        return self.m

    def K(self) -> int:  # noqa: N802
        return self.k

    def N(self) -> int:  # noqa: N802
        return self.n

    def _probes(self, key):
        h = fnv1_64(key)
        return [(h ^ hk) % self.m for hk in self.keys]

    def Add(self, key):  # noqa: N802
        for i in self._probes(key):
            self.bits[i >> 3] |= 1 << (i & 7)  # little-endian words: bit i & 63 of word i >> 6
        self.n += 1

    def Contains(self, key) -> bool:  # noqa: N802
        return all(self.bits[i >> 3] >> (i & 7) & 1 for i in self._probes(key))

    def payload(self) -> bytes:
        body = struct.pack(f"<3Q{self.k}Q", self.k, self.n, self.m, *self.keys) + bytes(self.bits)
        return body + hashlib.sha384(body).digest()

    def WriteFile(self, path: str):  # noqa: N802
        """bloom.bf.gz (Filter.WriteFile, sstable_writer.go:151): one gzip member around the payload."""
        try:
            with open(path, "wb") as fh:
                fh.write(gzip.compress(self.payload(), mtime=0))
        except OSError as e:
            return GoError(str(e))
        return None

    def on_device(self, device: int = 0) -> DeviceFilter:
        """The filter's current bits and hash keys as tensors on `device`."""
        import numpy as np
        import torch

        dev = f"cuda:{device}"
        bits = torch.from_numpy(np.frombuffer(bytes(self.bits), dtype=np.int64).copy()).to(dev)
        keys = torch.from_numpy(np.asarray(self.keys, dtype=np.uint64).view(np.int64).copy()).to(dev)
        return DeviceFilter(bits, keys, self.m, self.k)


def New(m: int, k: int, keys=None):  # noqa: N802
    """bloomfilter.New(m, k) -> (Filter, err). Hash keys from os.urandom unless given (then k = len(keys))."""
    if keys is not None:
        keys = list(keys)
        k = len(keys)
    if m < 2 or k < 1:
        return None, GoError(f"bloom filter: m = {m} and k = {k} are out of range (m >= 2, k >= 1)")
    if keys is None:
        keys = struct.unpack(f"<{k}Q", os.urandom(8 * k))
    return Filter(m, keys), None


def NewOptimal(max_n: int, p: float, keys=None):  # noqa: N802
    """bloomfilter.NewOptimal(maxN, p) -> (Filter, err) (sstable_writer.go:79)."""
    m, k = optimal(max_n, p)
    if m is None:
        return None, GoError(f"bloom filter: maxN = {max_n} and p = {p} are out of range (maxN > 0, 0 < p < 1)")
    if keys is not None:
        if len(keys) != k:
            return None, GoError(f"bloom filter: {len(keys)} hash keys given, {k} needed")
        return New(m, k, keys)
    return New(m, k)


def parse(raw: bytes):
    """A bloom.bf.gz image -> (Filter, err)."""
    try:
        body = gzip.decompress(raw)
    except (OSError, EOFError, zlib.error) as e:  # not gzip, a truncated member, a damaged deflate stream
        return None, GoError(f"gzip: {e}")
    if len(body) < 24 + 48:
        return None, GoError("bloom filter: payload shorter than its header and hash")
    k, n, m = struct.unpack_from("<3Q", body, 0)
    if m < 2 or k < 1:
        return None, GoError(f"bloom filter: m = {m} and k = {k} are out of range (m >= 2, k >= 1)")
    nw = (m + 63) // 64
    if len(body) != 24 + 8 * k + 8 * nw + 48:
        return None, GoError(f"bloom filter: payload of {len(body)} bytes does not match k = {k}, m = {m}")
    if hashlib.sha384(body[:-48]).digest() != body[-48:]:
        return None, GoError("bloom filter: SHA-384 hash mismatch")
    keys = struct.unpack_from(f"<{k}Q", body, 24)
    return Filter(m, keys, bytearray(body[24 + 8 * k:-48]), n), None


def ReadFile(path: str):  # noqa: N802
    """bloomfilter.ReadFile -> (Filter, err)."""
    try:
        with open(path, "rb") as fh:
            raw = fh.read()
    except OSError as e:
        return None, GoError(str(e))
    return parse(raw)


# the library's constructors and reader, also reachable through the type (bloom.Filter.NewOptimal(...))
Filter.New = staticmethod(New)
Filter.NewOptimal = staticmethod(NewOptimal)
Filter.ReadFile = staticmethod(ReadFile)
