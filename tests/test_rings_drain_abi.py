"""CPU test of the ring drain entry points' argument handling (no GPU calls)."""
import ctypes

import numpy as np

from usnetd_amd import lib
from test_deliver_rings_abi import bound as bound_rings, host_ctx

IDS = lib.USN_MAX_ENDPOINTS + 1


def bound(L, cap, cap_bytes):
    nbytes = L.usn_drain_bytes(cap, cap_bytes)
    buf = ctypes.create_string_buffer(nbytes + 256)
    base = (ctypes.addressof(buf) + 255) & ~255
    d = lib.Drain()
    assert L.usn_drain_bind(base, nbytes, cap, cap_bytes, ctypes.byref(d)) == 0
    return buf, base, nbytes, d


def test_drain_layout():
    L = lib.load()
    cap, cb = 1000, 48000
    _, base, nbytes, d = bound(L, cap, cb)
    ptrs = [d.frames, d.off16, d.lens, d.src, d.ep_off, d.ep_boff, d.budget, d.from_, d.take, d.left, d.hdr]
    assert ptrs == sorted(set(ptrs)) and all(p % 256 == 0 for p in ptrs) and ptrs[0] == base
    room = [b - a for a, b in zip(ptrs, ptrs[1:])]
    want = [cb, 4 * cap, 2 * cap, 4 * cap, 4 * (IDS + 1), 8 * (IDS + 1)] + [4 * IDS] * 4
    assert all(r >= w for r, w in zip(room, want))
    # behind the header: the tile prefix, the next heads, and 12 bytes per possible tile
    tiles = cap // lib.USN_DELIVER_TILE + IDS
    assert base + nbytes - d.hdr >= 256 + 2 * 4 * IDS + 12 * tiles
    assert (d.cap, d.cap_bytes) == (cap, cb) and ctypes.sizeof(lib.DrainHdr) == 32
    assert L.usn_drain_bind(base, nbytes - 1, cap, cb, ctypes.byref(d)) == lib.USN_ERANGE
    assert L.usn_drain_bind(base + 8, nbytes, cap, cb, ctypes.byref(d)) == lib.USN_EINVAL
    for c, b in [(0, cb), (1 << 32, cb), (cap, 0), (cap, 24), (cap, 1 << 36)]:
        assert L.usn_drain_bind(base, nbytes, c, b, ctypes.byref(d)) == lib.USN_EINVAL
        assert L.usn_drain_bytes(c, b) == 0
    assert L.usn_drain_bytes(1, (1 << 36) - 16) > 1 << 36


def test_drain_without_device():
    L = lib.load()
    keep = bound_rings(L, 1000, 64), bound(L, 1000, 64000)
    rs, d = keep[0][3], keep[1][3]
    h = host_ctx(L)
    call = lambda: L.usn_rings_drain(h, ctypes.byref(rs), ctypes.byref(d), None)
    assert call() == lib.USN_EINVAL   # bound, not initialised
    rs.ready = 1
    assert call() == lib.USN_ENODEV
    assert L.usn_rings_drain(h, ctypes.byref(rs), ctypes.byref(lib.Drain()), None) == lib.USN_EINVAL   # not bound
    assert L.usn_rings_drain(h, None, ctypes.byref(d), None) == lib.USN_EINVAL
    budget = np.ones(4, np.uint32)
    assert L.usn_drain_set_budget(h, ctypes.byref(d), budget.ctypes.data, 4, None) == lib.USN_ENODEV
    assert L.usn_drain_set_budget(h, ctypes.byref(d), budget.ctypes.data, IDS, None) == lib.USN_EINVAL
    hdr = lib.DrainHdr()
    assert L.usn_rings_drain_info(h, ctypes.byref(d), None, ctypes.byref(hdr)) == lib.USN_ENODEV
    L.usn_ctx_destroy(h)
