"""CPU test of the byte-ring delivery entry points' argument handling (no GPU calls)."""
import ctypes

import numpy as np
import pytest

from usnetd_amd import lib

IDS = lib.USN_MAX_ENDPOINTS + 1
P = lib.USN_DELIVER_TILE


def bound(L, desc, units):
    nbytes = L.usn_bringset_bytes(desc, units)
    buf = ctypes.create_string_buffer(nbytes + 256)
    base = (ctypes.addressof(buf) + 255) & ~255
    rs = lib.BRingSet()
    assert L.usn_bringset_bind(base, nbytes, desc, units, ctypes.byref(rs)) == 0
    return buf, base, nbytes, rs


def host_ctx(L):
    h = ctypes.c_void_p()
    assert L.usn_ctx_create(-1, ctypes.byref(h)) == 0   # USN_HOST_ONLY
    return h


def test_bringset_layout():
    L = lib.load()
    desc, units = 1000, 5000
    _, base, nbytes, rs = bound(L, desc, units)
    ptrs = [rs.frames, rs.lens, rs.src, rs.pos16, rs.desc_off, rs.unit_off, rs.head, rs.tail, rs.btail, rs.first,
            rs.bfirst, rs.acc, rs.drop, rs.acc_units, rs.seg_acc, rs.hdr]
    assert ptrs == sorted(set(ptrs)) and all(p % 256 == 0 for p in ptrs) and ptrs[0] == base
    room = [b - a for a, b in zip(ptrs, ptrs[1:])]
    want = [16 * units, 2 * desc, 4 * desc, 4 * desc] + [4 * (IDS + 1)] * 2 + [4 * IDS] * 8 + [4 * 8 * IDS]
    assert all(r >= w for r, w in zip(room, want))
    # behind the header: the per-id scratch, 6 bytes of staging per descriptor, three words per tile
    tiles = desc // P + lib.USN_MAX_ENDPOINTS + 2
    assert base + nbytes - rs.hdr >= ctypes.sizeof(lib.BRingSetHdr) + (4 * 4 + 4 * 8 + 8) * IDS + 6 * desc + 12 * tiles
    assert (rs.total_desc, rs.total_units, rs.ready) == (desc, units, 0) and ctypes.sizeof(lib.BRingSetHdr) == 40
    assert lib.HAS_DELIVER_BRINGS == 1
    assert L.usn_bringset_bind(base, nbytes - 1, desc, units, ctypes.byref(rs)) == lib.USN_ERANGE
    assert L.usn_bringset_bind(base + 8, nbytes, desc, units, ctypes.byref(rs)) == lib.USN_EINVAL
    for d, u in [(0, units), (desc, 0), (1 << 32, units), (desc, 1 << 32)]:
        assert L.usn_bringset_bind(base, nbytes, d, u, ctypes.byref(rs)) == lib.USN_EINVAL
        assert L.usn_bringset_bytes(d, u) == 0


@pytest.mark.parametrize("D,B,n_ids,rc", [
    ([8, 0, 16], [64, 0, 128], 3, lib.USN_ENODEV), ([8, 12], [64, 64], 2, lib.USN_EINVAL),
    ([8, 8], [64, 48], 2, lib.USN_EINVAL), ([8, 0], [64, 64], 2, lib.USN_EINVAL), ([8, 8], [64, 0], 2, lib.USN_EINVAL),
    ([1 << 31], [64], 1, lib.USN_EINVAL), ([8], [1 << 29], 1, lib.USN_EINVAL), ([512, 512], [64, 64], 2, lib.USN_EINVAL),
    ([8, 8], [4096, 4096], 2, lib.USN_EINVAL), ([0] * IDS, [0] * IDS, IDS, lib.USN_EINVAL)])
def test_bringset_init_checks_the_sizes(D, B, n_ids, rc):
    """valid sizes pass the checks (a host-only context then has no device); a size that is no power of
    two, a pair with one zero, a D above 2^30, a B above 2^28, sums above the totals and too many ids are refused"""
    L = lib.load()
    _, _, _, rs = bound(L, 1000, 5000)
    h = host_ctx(L)
    d, b = np.asarray(D, np.uint32), np.asarray(B, np.uint32)
    assert L.usn_bringset_init(h, ctypes.byref(rs), d.ctypes.data, b.ctypes.data, n_ids, None) == rc and rs.ready == 0
    L.usn_ctx_destroy(h)


@pytest.mark.parametrize("count,rc", [(0, lib.USN_EINVAL), (9, lib.USN_EINVAL), (1, lib.USN_ENODEV),
                                      (8, lib.USN_ENODEV)])
def test_deliver_brings_without_device(count, rc):
    L = lib.load()
    _, base, nbytes, rs = bound(L, 1000, 5000)
    h = host_ctx(L)
    b, r = (lib.Batch * 9)(), (lib.Result * 9)()
    for k in range(9):
        b[k].frames = b[k].lens = r[k].index = r[k].bin_off = r[k].summary = r[k].decisions = base   # never dereferenced
        b[k].stride, b[k].n, r[k].n = 2048, 16, 16   # no slot rule: any stride passes
    call = lambda: L.usn_deliver_brings(h, ctypes.cast(b, ctypes.c_void_p), ctypes.cast(r, ctypes.c_void_p),
                                        count, ctypes.byref(rs), None)
    assert call() == lib.USN_EINVAL   # bound, not initialised
    rs.ready = 1
    assert call() == rc
    b[0].n = 0   # what usn_deliver refuses for any ring
    assert call() == lib.USN_EINVAL
    hdr = lib.BRingSetHdr()
    assert L.usn_deliver_brings_info(h, ctypes.byref(rs), None, ctypes.byref(hdr)) == lib.USN_ENODEV
    head = np.zeros(4, np.uint32)
    assert L.usn_bringset_set_head(h, ctypes.byref(rs), head.ctypes.data, 4, None) == lib.USN_ENODEV
    L.usn_ctx_destroy(h)
