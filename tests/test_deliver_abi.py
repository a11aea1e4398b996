"""CPU test of the delivery entry points' argument handling (no GPU calls)."""
import ctypes

from usnetd_amd import lib


def test_delivery_layout_and_errors():
    L = lib.load()
    cap, slot = 1000, 64
    nbytes = L.usn_delivery_bytes(cap, slot)
    buf = ctypes.create_string_buffer(nbytes + 256)
    base = (ctypes.addressof(buf) + 255) & ~255
    d = lib.Delivery()
    assert L.usn_delivery_bind(base, nbytes, cap, slot, ctypes.byref(d)) == 0
    ptrs = [d.frames, d.lens, d.src, d.ep_off, d.hdr]
    assert ptrs == sorted(set(ptrs)) and all(p % 256 == 0 for p in ptrs)
    assert ptrs[0] == base and d.hdr + ctypes.sizeof(lib.DeliveryHdr) <= base + nbytes
    assert d.lens - d.frames >= cap * slot and d.src - d.lens >= 2 * cap and d.ep_off - d.src >= 4 * cap
    assert d.hdr - d.ep_off >= 4 * (lib.USN_MAX_ENDPOINTS + 1) and (d.cap, d.slot) == (cap, slot)
    assert L.usn_delivery_bind(base, nbytes - 1, cap, slot, ctypes.byref(d)) == lib.USN_ERANGE
    assert L.usn_delivery_bind(base, nbytes, cap, 24, ctypes.byref(d)) == lib.USN_EINVAL
    assert L.usn_delivery_bytes(cap, 24) == 0
    # usn_deliver: no device behind a registry-only context; a slot of 24 bytes is refused anywhere
    h = ctypes.c_void_p()
    assert L.usn_ctx_create(-1, ctypes.byref(h)) == 0   # USN_HOST_ONLY
    assert L.usn_delivery_bind(base, nbytes, cap, slot, ctypes.byref(d)) == 0
    b, r = lib.Batch(), lib.Result()
    b.frames = b.lens = r.index = r.bin_off = r.summary = r.decisions = base   # never dereferenced
    b.stride, b.n, r.n = 64, 16, 16
    assert L.usn_deliver(h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(d), None) == lib.USN_ENODEV
    assert L.usn_deliver(h, ctypes.byref(b), None, ctypes.byref(d), None) == lib.USN_EINVAL
    d.slot = 24
    assert L.usn_deliver(h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(d), None) == lib.USN_EINVAL
    L.usn_ctx_destroy(h)
