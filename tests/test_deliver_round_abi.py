"""CPU test of the round delivery entry points' argument handling (no GPU calls)."""
import ctypes

import pytest

from usnetd_amd import lib

IDS = lib.USN_MAX_ENDPOINTS + 1


def bound(L, cap, slot):
    nbytes = L.usn_rdelivery_bytes(cap, slot)
    buf = ctypes.create_string_buffer(nbytes + 256)
    base = (ctypes.addressof(buf) + 255) & ~255
    d = lib.RDelivery()
    assert L.usn_rdelivery_bind(base, nbytes, cap, slot, ctypes.byref(d)) == 0
    return buf, base, nbytes, d


def test_rdelivery_layout():
    L = lib.load()
    cap, slot = 1000, 64
    _, base, nbytes, d = bound(L, cap, slot)
    ptrs = [d.frames, d.lens, d.src, d.ep_off, d.seg_off, d.hdr]
    assert ptrs == sorted(set(ptrs)) and all(p % 256 == 0 for p in ptrs) and ptrs[0] == base
    room = [b - a for a, b in zip(ptrs, ptrs[1:])]
    assert all(r >= w for r, w in zip(room, [cap * slot, 2 * cap, 4 * cap, 4 * IDS, 4 * (8 * 4096 + 1)]))
    # behind the header: usn_deliver's scratch, the tile prefix
    assert base + nbytes - d.hdr >= ctypes.sizeof(lib.DeliveryHdr) + 4 * IDS and (d.cap, d.slot) == (cap, slot)
    assert L.usn_rdelivery_bind(base, nbytes - 1, cap, slot, ctypes.byref(d)) == lib.USN_ERANGE
    assert L.usn_rdelivery_bind(base, nbytes, cap, 24, ctypes.byref(d)) == lib.USN_EINVAL
    assert L.usn_rdelivery_bind(base, nbytes, 1 << 32, slot, ctypes.byref(d)) == lib.USN_EINVAL
    assert L.usn_rdelivery_bytes(cap, 24) == 0 and L.usn_rdelivery_bytes(0, slot) == 0


@pytest.mark.parametrize("count,rc", [(0, lib.USN_EINVAL), (9, lib.USN_EINVAL), (1, lib.USN_ENODEV),
                                      (8, lib.USN_ENODEV)])
def test_deliver_round_without_device(count, rc):
    L = lib.load()
    _, base, nbytes, d = bound(L, 1000, 64)
    h = ctypes.c_void_p()
    assert L.usn_ctx_create(-1, ctypes.byref(h)) == 0   # USN_HOST_ONLY
    b, r = (lib.Batch * 9)(), (lib.Result * 9)()
    for k in range(9):
        b[k].frames = b[k].lens = r[k].index = r[k].bin_off = r[k].summary = r[k].decisions = base   # never dereferenced
        b[k].stride, b[k].n, r[k].n = 64, 16, 16
    call = lambda: L.usn_deliver_round(h, ctypes.cast(b, ctypes.c_void_p), ctypes.cast(r, ctypes.c_void_p),
                                       count, ctypes.byref(d), None)
    assert call() == rc
    b[0].stride = 128   # above the slot: refused for any ring, as usn_deliver does
    assert call() == lib.USN_EINVAL
    hdr = lib.DeliveryHdr()
    assert L.usn_deliver_round_info(h, ctypes.byref(d), None, ctypes.byref(hdr)) == lib.USN_ENODEV
    L.usn_ctx_destroy(h)
