"""CPU test of the byte-ring drain entry points' argument handling (no GPU calls)."""
import ctypes

from usnetd_amd import lib
from test_deliver_brings_abi import bound as bound_brings, host_ctx
from test_rings_drain_abi import bound


def test_the_drain_region_is_the_ring_drain_s():
    L = lib.load()
    assert L.usn_drain_bytes(1000, 48000) == 256000   # what it returned before usn_brings_drain
    assert (lib.DR_BADDESC, lib.USN_BDRAIN_UTILE) == (64, 4096)


def test_brings_drain_without_device():
    L = lib.load()
    keep = bound_brings(L, 1000, 5000), bound(L, 1000, 64000)
    rs, d = keep[0][3], keep[1][3]
    h = host_ctx(L)
    call = lambda: L.usn_brings_drain(h, ctypes.byref(rs), ctypes.byref(d), None)
    assert call() == lib.USN_EINVAL   # bound, not initialised
    rs.ready = 1
    assert call() == lib.USN_ENODEV
    assert L.usn_brings_drain(h, ctypes.byref(rs), ctypes.byref(lib.Drain()), None) == lib.USN_EINVAL   # not bound
    assert L.usn_brings_drain(h, None, ctypes.byref(d), None) == lib.USN_EINVAL
    assert L.usn_brings_drain(h, ctypes.byref(rs), None, None) == lib.USN_EINVAL
    hdr = lib.DrainHdr()
    assert L.usn_brings_drain_info(h, ctypes.byref(d), None, ctypes.byref(hdr)) == lib.USN_ENODEV
    assert L.usn_brings_drain_info(h, ctypes.byref(d), None, None) == lib.USN_EINVAL
    L.usn_ctx_destroy(h)
