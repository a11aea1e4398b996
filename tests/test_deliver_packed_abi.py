"""CPU test of the packed delivery entry points' argument handling (no GPU calls)."""
import ctypes

import pytest

from usnetd_amd import lib

P = lib.USN_DELIVER_TILE


def bound(L, cap, cap_bytes):
    nbytes = L.usn_pdelivery_bytes(cap, cap_bytes)
    buf = ctypes.create_string_buffer(nbytes + 256)
    base = (ctypes.addressof(buf) + 255) & ~255
    d = lib.PDelivery()
    assert L.usn_pdelivery_bind(base, nbytes, cap, cap_bytes, ctypes.byref(d)) == 0
    return buf, base, nbytes, d


def test_pdelivery_layout():
    L = lib.load()
    cap, cap_bytes = 10000, 10000 * 368
    _, base, nbytes, d = bound(L, cap, cap_bytes)
    ptrs = [d.frames, d.off16, d.lens, d.src, d.ep_off, d.ep_boff, d.hdr]
    assert ptrs == sorted(set(ptrs)) and all(p % 256 == 0 for p in ptrs) and ptrs[0] == base
    room = [b - a for a, b in zip(ptrs, ptrs[1:])]
    ids = lib.USN_MAX_ENDPOINTS + 1
    assert all(r >= w for r, w in zip(room, [cap_bytes, 4 * cap, 2 * cap, 4 * cap, 4 * ids, 8 * ids]))
    # behind the header: the tile prefix, and a 64-bit base and a 32-bit total per possible tile
    tiles = cap // P + ids
    assert base + nbytes - d.hdr >= ctypes.sizeof(lib.PDeliveryHdr) + 4 * ids + 12 * tiles
    assert (d.cap, d.cap_bytes) == (cap, cap_bytes)


@pytest.mark.parametrize("cap,cap_bytes", [(0, 4096), (1 << 32, 4096), (1000, 0), (1000, 4088),
                                           (1000, 1 << 36)])
def test_pdelivery_bad_arguments(cap, cap_bytes):
    L = lib.load()
    _, base, nbytes, d = bound(L, 1000, 4096)
    assert L.usn_pdelivery_bytes(cap, cap_bytes) == 0
    assert L.usn_pdelivery_bind(base, nbytes, cap, cap_bytes, ctypes.byref(d)) == lib.USN_EINVAL


def test_pdelivery_bind_range_and_deliver_without_device():
    L = lib.load()
    assert L.usn_pdelivery_bytes(1 << 20, (1 << 36) - 16) > (1 << 36)   # the largest region is accepted
    _, base, nbytes, d = bound(L, 1000, 4096)
    assert L.usn_pdelivery_bind(base, nbytes - 1, 1000, 4096, ctypes.byref(d)) == lib.USN_ERANGE
    h = ctypes.c_void_p()
    assert L.usn_ctx_create(-1, ctypes.byref(h)) == 0   # USN_HOST_ONLY
    b, r = lib.Batch(), lib.Result()
    b.frames = b.lens = r.index = r.bin_off = r.summary = r.decisions = base   # never dereferenced
    b.stride, b.n, r.n = 2048, 16, 16
    assert L.usn_deliver_packed(h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(d), None) == lib.USN_ENODEV
    assert L.usn_deliver_packed(h, ctypes.byref(b), None, ctypes.byref(d), None) == lib.USN_EINVAL
    b.stride = 2040   # no multiple of 16
    assert L.usn_deliver_packed(h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(d), None) == lib.USN_EINVAL
    hdr = lib.PDeliveryHdr()
    assert L.usn_deliver_packed_info(h, ctypes.byref(d), None, ctypes.byref(hdr)) == lib.USN_ENODEV
    L.usn_ctx_destroy(h)
