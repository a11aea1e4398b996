"""CPU test of the ring delivery entry points' argument handling (no GPU calls)."""
import ctypes

import numpy as np
import pytest

from usnetd_amd import lib

IDS = lib.USN_MAX_ENDPOINTS + 1


def bound(L, total, slot):
    nbytes = L.usn_ringset_bytes(total, slot)
    buf = ctypes.create_string_buffer(nbytes + 256)
    base = (ctypes.addressof(buf) + 255) & ~255
    rs = lib.RingSet()
    assert L.usn_ringset_bind(base, nbytes, total, slot, ctypes.byref(rs)) == 0
    return buf, base, nbytes, rs


def host_ctx(L):
    h = ctypes.c_void_p()
    assert L.usn_ctx_create(-1, ctypes.byref(h)) == 0   # USN_HOST_ONLY
    return h


def test_ringset_layout():
    L = lib.load()
    total, slot = 1000, 64
    _, base, nbytes, rs = bound(L, total, slot)
    ptrs = [rs.frames, rs.lens, rs.src, rs.ring_off, rs.head, rs.tail, rs.first, rs.acc, rs.drop, rs.seg_acc, rs.hdr]
    assert ptrs == sorted(set(ptrs)) and all(p % 256 == 0 for p in ptrs) and ptrs[0] == base
    room = [b - a for a, b in zip(ptrs, ptrs[1:])]
    want = [total * slot, 2 * total, 4 * total, 4 * (IDS + 1)] + [4 * IDS] * 5 + [4 * 8 * IDS]
    assert all(r >= w for r, w in zip(room, want))
    # behind the header: the tile prefix and the next tails
    assert base + nbytes - rs.hdr >= ctypes.sizeof(lib.RingSetHdr) + 2 * 4 * IDS
    assert (rs.total, rs.slot, rs.ready) == (total, slot, 0) and ctypes.sizeof(lib.RingSetHdr) == 32
    assert L.usn_ringset_bind(base, nbytes - 1, total, slot, ctypes.byref(rs)) == lib.USN_ERANGE
    for t, s in [(total, 24), (total, 0), (0, slot), (1 << 32, slot)]:
        assert L.usn_ringset_bind(base, nbytes, t, s, ctypes.byref(rs)) == lib.USN_EINVAL
        assert L.usn_ringset_bytes(t, s) == 0


@pytest.mark.parametrize("sizes,n_ids,rc", [([8, 0, 16], 3, lib.USN_ENODEV), ([8, 12], 2, lib.USN_EINVAL),
                                            ([1 << 31], 1, lib.USN_EINVAL), ([512, 512], 2, lib.USN_EINVAL),
                                            ([0] * IDS, IDS, lib.USN_EINVAL)])
def test_ringset_init_checks_the_sizes(sizes, n_ids, rc):
    """valid sizes pass the checks (a host-only context then has no device); a size that is no
    power of two, one above 2^30, a sum above total and too many ids are refused"""
    L = lib.load()
    _, _, _, rs = bound(L, 1000, 64)
    h = host_ctx(L)
    arr = np.asarray(sizes, np.uint32)
    assert L.usn_ringset_init(h, ctypes.byref(rs), arr.ctypes.data, n_ids, None) == rc and rs.ready == 0
    L.usn_ctx_destroy(h)


@pytest.mark.parametrize("count,rc", [(0, lib.USN_EINVAL), (9, lib.USN_EINVAL), (1, lib.USN_ENODEV),
                                      (8, lib.USN_ENODEV)])
def test_deliver_rings_without_device(count, rc):
    L = lib.load()
    _, base, nbytes, rs = bound(L, 1000, 64)
    h = host_ctx(L)
    b, r = (lib.Batch * 9)(), (lib.Result * 9)()
    for k in range(9):
        b[k].frames = b[k].lens = r[k].index = r[k].bin_off = r[k].summary = r[k].decisions = base   # never dereferenced
        b[k].stride, b[k].n, r[k].n = 64, 16, 16
    call = lambda: L.usn_deliver_rings(h, ctypes.cast(b, ctypes.c_void_p), ctypes.cast(r, ctypes.c_void_p),
                                       count, ctypes.byref(rs), None)
    assert call() == lib.USN_EINVAL   # bound, not initialised
    rs.ready = 1
    assert call() == rc
    b[0].stride = 128   # above the slot: refused for any ring, as usn_deliver does
    assert call() == lib.USN_EINVAL
    hdr = lib.RingSetHdr()
    assert L.usn_deliver_rings_info(h, ctypes.byref(rs), None, ctypes.byref(hdr)) == lib.USN_ENODEV
    head = np.zeros(4, np.uint32)
    assert L.usn_ringset_set_head(h, ctypes.byref(rs), head.ctypes.data, 4, None) == lib.USN_ENODEV
    L.usn_ctx_destroy(h)
