"""The memstore's running size on the device (GPU): rio_mem_size_scan (csrc/rio_memsize.hip) and the mirror over it
(memstore.DeviceMemStore.EstimatedSizeInBytes / Apply / ApplyUntilFull).

The yardstick is tests/db_write_model.py: d_size is compared word for word with the model's estimatedSize after
every op, CUT / SIZE / KEY_END / VALUE_END with the model's. An op is (key, value), value None for a delete."""
import ctypes
import random
import struct

import numpy as np
import pytest
import torch

import db_write_model as wm
import memstore as M
import simpledb as DB
from recordio import _lib as L
from sstables.merger import on_device_stream

pytestmark = pytest.mark.gpu

_NONE = wm.NONE
NO_LIMIT = _NONE
# one full round of the new kernels' grid-stride loops (2048 blocks of 256 lanes, rio_memsize.hip) and 257 ops
GRID_ROUND = 2048 * 256


def batch_of(ops):
    b = DB.WriteBatch()
    for k, v in ops:
        assert (b.DeleteBytes(k) if v is None else b.PutBytes(k, v)) is None
    return b


def store_of(ops):
    """(DeviceMemIndex or None, ModelMemStore) of a write store that took `ops`."""
    model = wm.ModelMemStore()
    for op in ops:
        model.apply(op)
    return (M.DeviceMemIndex(batch_of(ops).upload(0)) if ops else None), model


def device_scan(index, size0, dev_ops, max_size, max_key_len=None):
    """rio_mem_size_scan -> (d_size as a list, the result words). Buffers start as ~0: a word the call leaves shows."""
    n = int(dev_ops.view.n)
    d_size = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    d_result = torch.full((L.RIO_SIZE_RESULT_WORDS,), -1, dtype=torch.int64, device="cuda")
    store = None if index is None else index.view
    bv = dev_ops.view
    bound = dev_ops.max_key_len if max_key_len is None else max_key_len
    rc = on_device_stream(0, lambda st: L.lib().rio_mem_size_scan(
        L.default_ctx(0), None if store is None else ctypes.addressof(store), size0, ctypes.addressof(bv), bound, max_size,
        d_size.data_ptr(), d_result.data_ptr(), st))
    assert rc == L.RIO_OK, rc
    torch.cuda.synchronize()
    sizes = (d_size[:n].cpu().numpy().astype(np.uint64)).tolist()
    return sizes, [x & _NONE for x in d_result.cpu().tolist()]


def check_scan(store_ops, ops, max_size=NO_LIMIT, size0=None, store=None):
    """The device's words for `ops` over a store that took `store_ops` equal the model's; -> the model's cut."""
    index, model = store if store is not None else store_of(store_ops)
    if size0 is not None:
        model = wm.ModelMemStore(model.latest, size0)
    sizes, r = device_scan(index, model.size, batch_of(ops).upload(0), max_size)
    w_sizes, w_cut, w_last = wm.scan(model, ops, max_size)
    assert r[L.RIO_SIZE_R_FIRST_BAD] == _NONE
    assert sizes == w_sizes
    end = (w_cut + 1) if w_cut != _NONE else len(ops)
    assert r[L.RIO_SIZE_R_CUT] == w_cut and r[L.RIO_SIZE_R_SIZE] == w_last
    assert r[L.RIO_SIZE_R_KEY_END] == sum(len(k) for k, _ in ops[:end])
    assert r[L.RIO_SIZE_R_VALUE_END] == sum(len(v or b"") for _, v in ops[:end])
    return w_cut


def seeded(seed, n, n_keys, key=lambda i: struct.pack(">Q", i * 0x9E3779B97F4A7C15 & wm.U64)):
    rng = random.Random(seed)
    ops = []
    for _ in range(n):
        k = key(rng.randrange(n_keys))
        ops.append((k, None) if rng.random() < 0.3 else (k, b"v" * rng.choice((0, 1, 3, 9, 30))))
    return ops


STORE = seeded(11, 600, 400)  # 8-byte keys, some tombstoned, some with empty values
_shared = {}


def shared_store():
    """One store index for the size cases, built once and left unchanged."""
    if "s" not in _shared:
        _shared["s"] = store_of(STORE)
    return _shared["s"]


# ---- 1. batch sizes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_batch_sizes(n):
    ops = seeded(n, n, 500)  # keys of the store and new ones, repeated inside the batch
    check_scan(None, ops, store=shared_store())
    check_scan([], ops)
    # a limit in the middle of the run
    if n:
        mid = wm.scan(shared_store()[1], ops, NO_LIMIT)[0][n // 2]
        check_scan(None, ops, max_size=wm.estimate(mid), store=shared_store())


def test_empty_batch_writes_the_result_block_only():
    index, model = shared_store()
    sizes, r = device_scan(index, 12345, batch_of([]).upload(0), 10)
    assert sizes == [] and r[:5] == [_NONE, 12345, 0, 0, _NONE]
    sizes, r = device_scan(None, 7, batch_of([]).upload(0), 10)
    assert r[:5] == [_NONE, 7, 0, 0, _NONE]


def test_a_full_round_of_the_grid_and_257_ops():
    n = GRID_ROUND + 257
    rng = random.Random(3)
    picks = np.asarray([rng.randrange(200000) for _ in range(n)], dtype=np.uint64)
    dels = [rng.random() < 0.3 for _ in range(n)]
    ops = [(struct.pack(">Q", int(p) * 0x9E3779B97F4A7C15 & wm.U64), None if d else b"v" * (int(p) % 7))
           for p, d in zip(picks.tolist(), dels)]
    index, model = shared_store()
    w_sizes, _, _ = wm.scan(model, ops, NO_LIMIT)
    limit = wm.estimate(w_sizes[GRID_ROUND + 100])  # a cut in the second round, or where the estimate first passes it
    dev = batch_of(ops).upload(0)
    sizes, r = device_scan(index, model.size, dev, limit)
    w_sizes, w_cut, w_last = wm.scan(model, ops, limit)
    assert sizes == w_sizes
    assert r[L.RIO_SIZE_R_CUT] == w_cut and r[L.RIO_SIZE_R_SIZE] == w_last and r[L.RIO_SIZE_R_FIRST_BAD] == _NONE
    assert r[L.RIO_SIZE_R_KEY_END] == 8 * (w_cut + 1)


# ---- 2. chains inside the batch, against the four states of the key in the store ----------------------------------

K = b"chainkey"
STATES = {
    "empty store": [],
    "key with a value": [(b"other", b"o"), (K, b"stored value")],
    "key with an empty value": [(K, b"x"), (K, b""), (b"other", b"o")],
    "key as a tombstone": [(K, b"gone"), (b"other", b"o"), (K, None)],
}
CHAINS = {
    "one key n times": [(K, b"v" * (i % 5)) if i % 3 else (K, None) for i in range(300)],
    "put delete put": [(K, b"first"), (K, None), (K, b"second!")],
    "put of an empty value": [(K, b""), (b"zz", b"1"), (K, b"after"), (K, b"")],
    "chain between other keys": [(b"a", b"1"), (K, b"abc"), (b"b", None), (K, None), (b"a", b""), (K, None), (K, b"z")],
}


@pytest.mark.parametrize("state", list(STATES))
@pytest.mark.parametrize("chain", list(CHAINS))
def test_chains(state, chain):
    check_scan(STATES[state], CHAINS[chain])


def test_deletes_of_absent_present_and_tombstoned_keys():
    store = [(b"present", b"value"), (b"dead", b"x"), (b"dead", None), (b"empty", b"")]
    ops = [(b"absent", None), (b"present", None), (b"dead", None), (b"empty", None), (b"absent", None), (b"present", None),
           (b"absent2", None), (b"absent2", b"back"), (b"", None)]
    check_scan(store, ops)
    check_scan([], ops)


def test_sort_edges():
    """The flush tests' key edges: the empty key, keys that differ only at byte 9, proper prefixes, zero-padded twins."""
    p8 = b"prefix_8"
    keys = [b"", p8 + b"a", p8 + b"b", p8, p8[:3], b"a", b"a\0", b"a\0\0", b"\0", b"\0\0", p8 + b"\0", p8 + b"a" * 40]
    rng = random.Random(9)
    store = [(rng.choice(keys), None if rng.random() < 0.3 else b"s" * rng.randrange(5)) for _ in range(40)]
    ops = [(rng.choice(keys), None if rng.random() < 0.3 else b"b" * rng.randrange(9)) for _ in range(300)]
    check_scan(store, ops)
    check_scan([], ops)
    check_scan(store, ops, max_size=wm.estimate(wm.scan(store_of(store)[1], ops, NO_LIMIT)[0][150]))


# ---- 3. cuts ----------------------------------------------------------------------------------------------------

def test_cut_at_op_0_at_the_last_op_and_nowhere():
    ops = [(b"k%d" % i, b"0123456789") for i in range(10)]  # 12 bytes each
    assert check_scan([], ops, max_size=0) == 0
    assert check_scan([], ops, max_size=wm.estimate(12 * 10) - 1) == 9
    assert check_scan([], ops, max_size=wm.estimate(12 * 10)) == _NONE
    assert check_scan([], [(b"k", None)] + ops, max_size=0) == 1  # the delete in front passes the limit and never cuts


def test_a_delete_over_the_limit_never_cuts():
    long_key = b"L" * 100
    store = [(b"big", b"B" * 80)]  # raw size 83
    limit = wm.estimate(150)
    # the delete of an absent key takes the size to 183: no cut there; the put behind it is the cut
    assert check_scan(store, [(long_key, None), (b"x", b"y")], max_size=limit) == 1
    # the put replaces the long value by a short one: 183 - 80 + 1 is under the limit again, no cut at all
    assert check_scan(store, [(long_key, None), (b"big", b"b")], max_size=limit) == _NONE
    # deletes alone never cut, however far over
    assert check_scan(store, [(long_key + b"%d" % i, None) for i in range(5)], max_size=limit) == _NONE


@pytest.mark.parametrize("target", [(1 << 24) + 1, (1 << 25) + 3, 1 << 32, (1 << 40) + (1 << 17)])
def test_float32_rule(target):
    """d_size crosses `target` one byte at a time; the limit is the model's estimate there and its neighbours."""
    ops = [(bytes([65 + i]), b"") for i in range(12)]  # every put of a new 1-byte key adds 1
    size0 = target - 6
    assert wm.scan(wm.ModelMemStore(size=size0), ops, NO_LIMIT)[0][5] == target
    est = wm.estimate(target)
    cuts = [check_scan([], ops, max_size=est + d, size0=size0) for d in (0, -1, 1)]
    assert cuts[1] != _NONE  # the estimate at the target passes est - 1: some op at or before it cuts
    lo, hi = wm.estimate(size0 + 1), wm.estimate(size0 + 12)
    for limit in sorted({lo - 1, lo, hi - 1, hi}):  # every step of the estimate inside the run
        check_scan([], ops, max_size=limit, size0=size0)


def test_sizes_wrap_mod_2_64():
    ops = [(b"k", b"long value here"), (b"k", None), (b"k", b"v")]
    check_scan([], ops, size0=wm.U64 - 3)


# ---- 4. rejections ----------------------------------------------------------------------------------------------

def test_rejections():
    ops = [(b"k%d" % i, b"v") for i in range(6)] + [(b"seven77", b"v"), (b"k8", b"v")]
    dev = batch_of(ops).upload(0)
    _, r = device_scan(None, 0, dev, NO_LIMIT, max_key_len=6)  # op 6's key is one byte over
    assert r[L.RIO_SIZE_R_FIRST_BAD] == 6
    _, r = device_scan(None, 0, dev, NO_LIMIT, max_key_len=7)
    assert r[L.RIO_SIZE_R_FIRST_BAD] == _NONE
    back = batch_of(ops).upload(0)
    back.key_off[4] = back.key_off[3] - 1  # op 3's end lies before its start
    _, r = device_scan(None, 0, back, NO_LIMIT)
    assert r[L.RIO_SIZE_R_FIRST_BAD] == 3
    # a store index that was rejected: its keys are longer than the bound it was built with
    raw = batch_of([(b"longer", b"v"), (b"k", b"v")])
    bad_store = M.DeviceMemIndex(M.upload_ops(0, raw._keys, raw._key_off, raw._values, raw._val_off, raw._flags, 1))
    assert bad_store.result_words()[L.RIO_MERGE_R_UNSORTED] == 0
    _, r = device_scan(bad_store, 0, dev, NO_LIMIT)
    assert r[L.RIO_SIZE_R_FIRST_BAD] == 0


# ---- 5. the mirror ----------------------------------------------------------------------------------------------

def rest_ops(rest):
    """The ops of a DeviceOps, read back."""
    n = rest.n
    ko, vo = rest.key_off[:n + 1].cpu().tolist(), rest.val_off[:n + 1].cpu().tolist()
    assert ko[0] == 0 and vo[0] == 0  # rebased, as rio_ops_append asks
    assert int(rest.view.key_bytes) == ko[n] and int(rest.view.value_bytes) == vo[n]
    keys, values, flags = bytes(rest.keys.cpu().numpy()), bytes(rest.values.cpu().numpy()), rest.flags.cpu().tolist()
    return [(keys[ko[i]:ko[i + 1]], None if flags[i] & L.RIO_FLAG_NIL else values[vo[i]:vo[i + 1]]) for i in range(n)]


def check_reads(store, model):
    keys = sorted(model.latest) + [b"never written"]
    want = [(None, M.KeyNotFound) if k not in model.latest else
            ((None, M.KeyTombstoned) if model.latest[k] is None else (model.latest[k], None)) for k in keys]
    assert store.GetBatch(keys) == want
    assert store.Size() == len(model.latest)
    assert store.EstimatedSizeInBytes() == model.estimated()


def test_apply_keeps_the_size_current():
    store, model = M.DeviceMemStore(0), wm.ModelMemStore()
    assert store.EstimatedSizeInBytes() == 0
    for seed in (1, 2, 3):
        ops = seeded(seed, 200, 60)
        assert store.Apply(batch_of(ops)) is None
        for op in ops:
            model.apply(op)
        assert store.EstimatedSizeInBytes() == model.estimated() and store._raw_size() == model.size
    assert store.Apply(batch_of([])) is None
    check_reads(store, model)


def test_apply_until_full_follows_the_loop_through_three_rotations():
    ops = seeded(21, 400, 80)
    whole = wm.ModelMemStore()
    for op in ops:
        whole.apply(op)
    limit = wm.estimate(whole.size) // 3  # the batch fills a memstore of this size about three times
    store, model = M.DeviceMemStore(0), wm.ModelMemStore()
    rest, a, rotations = batch_of(ops).upload(0), 0, 0
    while rest is not None:
        _, w_cut, _ = wm.scan(model, ops[a:], limit)
        k, rest = store.ApplyUntilFull(rest, limit)
        assert k == (w_cut + 1 if w_cut != _NONE else len(ops) - a)
        for op in ops[a:a + k]:
            model.apply(op)
        a += k
        if rest is not None:
            assert rest_ops(rest) == ops[a:]
        check_reads(store, model)
        if w_cut != _NONE:  # the rotation: a fresh write store
            assert ops[a - 1][1] is not None and store.EstimatedSizeInBytes() > limit
            store, model, rotations = M.DeviceMemStore(0), wm.ModelMemStore(), rotations + 1
    assert a == len(ops) and rotations >= 3
    # no cut: the whole batch, no rest; an empty batch: nothing
    assert M.DeviceMemStore(0).ApplyUntilFull(batch_of(ops), NO_LIMIT) == (len(ops), None)
    assert store.ApplyUntilFull(batch_of([]), 10) == (0, None)
