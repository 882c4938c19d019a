"""Child process of tests/test_gpu_encode_edges.py::test_tuning_knob (needs a GPU).

librio reads RIO_ENC_LANES, RIO_ENC_LDS and RIO_ENC_GROUPS once per process, so each value is tried in
a fresh process with that variable set: this one encodes the concatenated edge families and the
8257-record launch shape on the device, compares them with the oracle and exits 0, or 1 after a
one-line reason. encode_file_arrays is also the parent's rio_encode_file wrapper."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "go-sstables_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def encode_file_arrays(blob, off, flags, comp, out_cap=None, fill=None):
    """rio_encode_file on numpy arrays: (status, out buffer [out_cap], record offsets, *out_len).
    out_cap None = rio_encode_bound; fill = byte the out buffer holds before the call."""
    from recordio import _lib as L

    n = int(off.shape[0]) - 1
    blob = np.ascontiguousarray(np.concatenate([blob, np.zeros(8, np.uint8)]))
    fl = None if flags is None else np.ascontiguousarray(np.concatenate([flags, np.zeros(8, np.uint8)]), dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    cap = int(L.lib().rio_encode_bound(n, int(off[-1] - off[0]), comp)) if out_cap is None else out_cap
    out = np.empty(cap, dtype=np.uint8) if fill is None else np.full(cap, fill, dtype=np.uint8)
    roff = np.zeros(max(n, 1), dtype=np.uint64)
    ln = ctypes.c_uint64()
    rc = L.lib().rio_encode_file(L.default_ctx(0), blob.ctypes.data, off.ctypes.data,
                                 None if fl is None else fl.ctypes.data, n, comp, out.ctypes.data, cap, roff.ctypes.data,
                                 ctypes.byref(ln))
    return rc, out, roff[:n], ln.value


def first_difference(got, want):
    if got.shape[0] != want.shape[0]:
        return f"{got.shape[0]} bytes, want {want.shape[0]}"
    bad = np.nonzero(got != want)[0]
    return None if bad.size == 0 else f"first of {bad.size} differing bytes at {int(bad[0])}"


def check(what, arrays, comp):
    import encode_cases as E

    rc, out, roff, ln = encode_file_arrays(*arrays, comp)
    if rc:
        return f"{what} comp {comp}: rio_encode_file status {rc}"
    want, want_off = E.oracle_arrays(*arrays, comp)
    d = first_difference(out[:ln], want)
    if d:
        return f"{what} comp {comp}: image {d}"
    if not np.array_equal(roff, want_off):
        return f"{what} comp {comp}: record offsets differ"
    return None


def main():
    import encode_cases as E

    knobs = " ".join(f"{k}={v}" for k, v in sorted(os.environ.items()) if k.startswith("RIO_ENC_"))
    every = E.to_arrays([r for _, _, r in E.shuffled_all()])
    for what, arrays, comp in (("families", every, 2), ("families", every, 0), ("8257 records", E.launch_global_reuse(), 2)):
        err = check(what, arrays, comp)
        if err:
            print(f"FAIL [{knobs}] {err}")
            return 1
    print(f"ok [{knobs}]")
    return 0


if __name__ == "__main__":
    sys.exit(main())
