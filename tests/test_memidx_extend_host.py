"""The argument errors of rio_ops_append and rio_mem_index_extend (CPU): every refusal comes back before the context
or the device is touched, so the calls are made with placeholder handles and device pointers on a machine that may
have no GPU (the pattern of tests/test_db_get_host.py)."""
import ctypes

from recordio import _lib as L

PAD = L.RIO_DEVICE_PAD
FIELDS = [k for k, _ in L.OpsView._fields_]
ARRAYS = ("keys", "key_off", "values", "val_off", "flags")


def _view(**kw):
    d = dict(keys=64, key_off=64, values=64, val_off=64, flags=64, n=5, key_bytes=10, value_bytes=20)
    d.update(kw)
    return L.OpsView(**d)


def _without(view, field):
    kw = {k: getattr(view, k) for k in FIELDS}
    kw[field] = None
    return L.OpsView(**kw)


def test_ops_append_refuses_arguments_before_any_device_call():
    lib = L.lib()
    ctx = ctypes.c_void_p(8)
    log, batch = _view(n=7, key_bytes=100, value_bytes=200), _view(n=5, key_bytes=10, value_bytes=20)
    av = ctypes.addressof

    def append(c=ctx, lg=log, b=batch, ops_cap=12, keys_cap=110 + PAD, values_cap=220 + PAD):
        return lib.rio_ops_append(c, None if lg is None else av(lg), ops_cap, keys_cap, values_cap,
                                  None if b is None else av(b), None)

    assert append(c=None) == L.RIO_ERR_ARG
    assert append(lg=None) == L.RIO_ERR_ARG
    assert append(b=None) == L.RIO_ERR_ARG
    for field in ARRAYS:  # batch.n > 0 with a NULL array on either side
        assert append(lg=_without(log, field)) == L.RIO_ERR_ARG, field
        assert append(b=_without(batch, field)) == L.RIO_ERR_ARG, field
    # capacities one op or one byte too small, the pad included; the exact capacities pass these checks (the next
    # refusal, the op bound, shows it below)
    assert append(ops_cap=11) == L.RIO_ERR_ARG
    assert append(keys_cap=110 + PAD - 1) == L.RIO_ERR_ARG
    assert append(keys_cap=110) == L.RIO_ERR_ARG  # room for the bytes, none for the pad
    assert append(values_cap=220 + PAD - 1) == L.RIO_ERR_ARG
    assert append(keys_cap=0) == L.RIO_ERR_ARG and append(values_cap=PAD - 1) == L.RIO_ERR_ARG
    assert append(lg=_view(n=13, key_bytes=100, value_bytes=200)) == L.RIO_ERR_ARG  # the log itself exceeds ops_cap
    # 2^31 - 1 ops and more in all: every capacity suffices, the total is refused
    top = (1 << 31) - 1
    assert append(lg=_view(n=top - 5, key_bytes=100, value_bytes=200), ops_cap=top) == L.RIO_ERR_UNSUPPORTED
    assert append(lg=_view(n=top - 6, key_bytes=100, value_bytes=200), ops_cap=top - 2) == L.RIO_ERR_ARG  # capacity first
    # an empty batch is a no-op: nothing is touched, whatever the arrays and capacities
    empty = _view(n=0, key_bytes=0, value_bytes=0)
    assert append(b=empty) == L.RIO_OK
    assert append(b=L.OpsView(), lg=L.OpsView(), ops_cap=0, keys_cap=0, values_cap=0) == L.RIO_OK


def test_mem_index_extend_refuses_arguments_before_any_device_call():
    lib = L.lib()
    ctx, ptr = ctypes.c_void_p(8), ctypes.c_void_p(64)
    ops = _view()
    av = ctypes.addressof

    def extend(c=ctx, o=ops, n_old=2, max_key_len=8, order=ptr, pfx=ptr, res=ptr):
        return lib.rio_mem_index_extend(c, None if o is None else av(o), n_old, max_key_len, order, pfx, res, None)

    assert extend(c=None) == L.RIO_ERR_ARG
    assert extend(o=None) == L.RIO_ERR_ARG
    assert extend(res=None) == L.RIO_ERR_ARG
    assert extend(order=None) == L.RIO_ERR_ARG
    assert extend(pfx=None) == L.RIO_ERR_ARG
    for field in ARRAYS:
        assert extend(o=_without(ops, field)) == L.RIO_ERR_ARG, field
    assert extend(n_old=6) == L.RIO_ERR_ARG  # n_old > ops.n
    assert extend(n_old=6, max_key_len=L.RIO_FLUSH_MAX_KEY_LEN + 1) == L.RIO_ERR_ARG
    assert extend(max_key_len=L.RIO_FLUSH_MAX_KEY_LEN + 1) == L.RIO_ERR_UNSUPPORTED
    assert extend(n_old=0, max_key_len=L.RIO_FLUSH_MAX_KEY_LEN + 1) == L.RIO_ERR_UNSUPPORTED
    huge = _view(n=(1 << 31) - 1)
    assert extend(o=huge) == L.RIO_ERR_UNSUPPORTED
    assert extend(o=huge, n_old=(1 << 31) - 1) == L.RIO_ERR_UNSUPPORTED
    # n_old = ops.n leaves the index as it is: no device call, the context is not read
    assert extend(n_old=5) == L.RIO_OK
    assert extend(o=L.OpsView(), n_old=0, order=None, pfx=None) == L.RIO_OK  # an empty log needs no arrays


def test_binding_names_both_calls():
    assert {"rio_ops_append", "rio_mem_index_extend"} <= set(L.EXPORTED)
